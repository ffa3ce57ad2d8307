// Event-frame layer of the 2-D convolutions (gfx950), forward and weight gradient; launched from conv_gather.hip and
// conv_wgrad.hip through the declarations in conv_common.h.
//
// The convolution over the 2-channel event frames (Cin = 2, 3x3: K = 18) does not belong on the matrix pipe
// (SURVEY 8d): its cost is writing y (forward) / reading dy (weight gradient).  Direct kernels: a thread owns 4
// output channels with their 4 x 18 weights (forward) or 4 x 18 gradient accumulators (backward) in registers and
// walks output pixels; the 16 threads of a pixel read the same 9 input positions (one broadcast access each).
// (Skipping the taps whose input is 0 - event frames are sparse - was measured and does not pay: the 18 divergent
// branches per pixel cost more issue slots than the 72 fmaf they save.)
// Arithmetic: fp32 fmaf chain over (kh, kw, ci) in order, for every precision mode.
#include "conv_common.h"

namespace {

// One block walks output ROWS (block-uniform row index: the image / row split and the vertical bounds are scalar
// work), its PP pixel lanes walk the row; per pixel all nine input positions are loaded before any is tested.
// SB (bf16-storage mode): the wide tensors - y (forward), dy / gx and the saved y (weight gradient) - are bf16; the event
// frames x stay fp32.
// (the weight gradient's grid is four blocks per CU - snn_conv2d_wgrad_splitk - so its instances are held to four waves per
// SIMD: the BatchNorm-apply form needed 138 registers, three waves, and ran a quarter of its blocks in a second round)
template <int CIN, int KS, bool WGRAD, bool BNAPPLY = false, bool SB = false>
__global__ __launch_bounds__(kThreads, WGRAD ? 4 : 1) void k_conv_first(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ dy, float* __restrict__ out,
                                                         FirstGeom g) {
    static_assert(CIN == 2, "float2 input pixels");
    typedef SnnStore<SB> St;
    constexpr int KT = KS * KS * CIN;
    __shared__ float red[WGRAD ? kThreads : 1][KT + 1];
    __shared__ double sred[WGRAD ? 1 : kThreads][9];               // statistics of the forward pass (8 used: odd pitch)
    extern __shared__ __attribute__((aligned(16))) float2 srow[];   // [KS][W + 2 pad] input rows of the current output row
    const int cgs = g.Cout / 4;                       // channel groups: a power of two <= 64
    const int cg = threadIdx.x % cgs, pl = threadIdx.x / cgs, PP = kThreads / cgs;
    float wr[4][KT];                                  // forward: weights; weight gradient: accumulators
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < KT; ++k) wr[c][k] = WGRAD ? 0.f : w[(cg * 4 + c) * KT + k];
    const int ldx = (int)g.ldx, ldy = (int)g.ldy;
    const int grp = blockIdx.x / g.group_blocks, grp_j = blockIdx.x - grp * g.group_blocks;
    const int r_end = (grp + 1) * g.group_rows < g.rows ? (grp + 1) * g.group_rows : g.rows;
    // BatchNorm partials of the forward pass: a thread sums the <= ceil(Wo / PP) pixels it owns of ONE row in fp32
    // (per-pixel fp64 work cost this kernel 30 %), the rows and everything above in fp64
    // (the fp64 sums live in the thread's own LDS slot: in registers they cost the kernel a wave of occupancy)
    const bool stats = !WGRAD && g.bn_partial != nullptr;
    if (!WGRAD && stats) {
#pragma unroll
        for (int c = 0; c < 8; ++c) sred[threadIdx.x][c] = 0.0;
    }
    // The KS input rows of an output row (with their zero padding) go through LDS: the 16 lanes of a pixel read the same nine
    // positions, and same-address lanes of a global load are separate accesses for the texture addresser.  A block stages
    // the input rows of g.rs of its output rows at once - ONE pair of barriers and ONE exposed memory latency per g.rs rows,
    // and the staging loads of a thread are all requested before the first is written to LDS (four at a time, addresses
    // clamped instead of branched around: the loop used to wait for every single load, six dependent round trips per row).
    const int LW = g.W + 2 * g.pad;
    const int stage_elems = KS * LW;                   // float2 elements of one output row's input rows
    for (int r0 = grp * g.group_rows + grp_j; r0 < r_end; r0 += g.group_blocks * g.rs) {
        int nrows = (r_end - r0 + g.group_blocks - 1) / g.group_blocks;   // block-uniform
        nrows = nrows < g.rs ? nrows : g.rs;
        const int total = nrows * stage_elems;
        __syncthreads();
        for (int e0 = threadIdx.x; e0 < total; e0 += 4 * kThreads) {
            float2 t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u * kThreads;
                const int ec = e < total ? e : total - 1;
                const int jk = ec / LW, ixp = ec - jk * LW;       // (row of the stage) * KS + kh, padded column
                const int j = jk / KS, kh = jk - j * KS;
                const int r = r0 + j * g.group_blocks;
                const int img = r / g.Ho, oy = r - img * g.Ho;
                const int iy = oy * g.stride - g.pad + kh, ix = ixp - g.pad;
                const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                const float2 v = *reinterpret_cast<const float2*>(
                    x + ((int64_t)img * g.H + (ok ? iy : 0)) * g.W * g.ldx + (ok ? ix * ldx : 0));
                t[u] = ok ? v : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u * kThreads;
                if (e < total) srow[e] = t[u];
            }
        }
        __syncthreads();
      for (int jrow = 0; jrow < nrows; ++jrow) {
        const int r = r0 + jrow * g.group_blocks;
        const int img = r / g.Ho;
        const float2* srow_r = srow + jrow * stage_elems;
        const int64_t dyrow = (int64_t)r * g.Wo * g.ldy + cg * 4;   // element index of the row's first pixel in dy / out
        int64_t byrow = 0;
        f32x4 ca = {0.f, 0.f, 0.f, 0.f}, cb = ca, cc = ca;
        if constexpr (WGRAD && BNAPPLY) {   // the row's timestep is block-uniform: three coefficient quads per row
            byrow = (int64_t)r * g.Wo * g.bn_ldy + cg * 4;
            const float* cf = g.bn_coef + (int64_t)(img / g.bn_fps) * g.Cout + cg * 4;
            ca = *reinterpret_cast<const f32x4*>(cf);
            cb = *reinterpret_cast<const f32x4*>(cf + g.bn_tc);
            cc = *reinterpret_cast<const f32x4*>(cf + 2 * (int64_t)g.bn_tc);
        }
        float row_s[4] = {0.f, 0.f, 0.f, 0.f}, row_q[4] = {0.f, 0.f, 0.f, 0.f};
        // weight gradient: the dy (gx, y) quads of a pixel are requested one pixel AHEAD of their use.  With the loads in
        // front of the 72 fmaf that consume them a wave had two 16-byte accesses in flight and then none: 2.2 TB/s for a
        // kernel that runs alone at the end of the backward pass (the step's tail).  The index of the pixel after the
        // row's last is clamped (its quads are loaded and dropped): no branch around the loads.
        [[maybe_unused]] f32x4 gv_next = {0.f, 0.f, 0.f, 0.f}, yv_next = gv_next;
        if (WGRAD && pl < g.Wo) {
            gv_next = St::ld4_last(dy, dyrow + pl * ldy);
            if constexpr (BNAPPLY) yv_next = St::ld4_last(g.bn_y, byrow + pl * (int)g.bn_ldy);
        }
        for (int ox = pl; ox < g.Wo; ox += PP) {
            float2 taps[KS][KS];
#pragma unroll
            for (int kh = 0; kh < KS; ++kh)
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) taps[kh][kw] = srow_r[kh * LW + ox * g.stride + kw];
            f32x4 gv = {0.f, 0.f, 0.f, 0.f};
            if (WGRAD) {
                gv = gv_next;
                const int oxn = ox + PP < g.Wo ? ox + PP : ox;
                gv_next = St::ld4_last(dy, dyrow + oxn * ldy);
                if constexpr (BNAPPLY) {   // the statement of k_bn_bwd_apply (bn_bwd.hip): same roundings
                    const f32x4 yv = yv_next;
                    yv_next = St::ld4_last(g.bn_y, byrow + oxn * (int)g.bn_ldy);
#pragma unroll
                    for (int c = 0; c < 4; ++c) gv[c] = ca[c] * gv[c] + cb[c] * yv[c] + cc[c];
                }
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kh = 0; kh < KS; ++kh)
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const float2 v = taps[kh][kw];
                    const int k0 = (kh * KS + kw) * CIN;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (WGRAD) {
                            wr[c][k0] = fmaf(gv[c], v.x, wr[c][k0]);
                            wr[c][k0 + 1] = fmaf(gv[c], v.y, wr[c][k0 + 1]);
                        } else {
                            acc[c] = fmaf(v.x, wr[c][k0], acc[c]);
                            acc[c] = fmaf(v.y, wr[c][k0 + 1], acc[c]);
                        }
                    }
                }
            if (!WGRAD) {
                f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
                St::st4(out, dyrow + ox * ldy, o);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    row_s[c] += acc[c];
                    row_q[c] = fmaf(acc[c], acc[c], row_q[c]);
                }
            }
        }
        if (!WGRAD && stats) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sred[threadIdx.x][c] += (double)row_s[c];
                sred[threadIdx.x][4 + c] += (double)row_q[c];
            }
        }
      }
    }
    if (!WGRAD && stats) {
        // block sum over the PP pixel lanes of every channel, in lane order
        __syncthreads();
        if ((int)threadIdx.x < g.Cout) {
            const int gq = threadIdx.x >> 2, c = threadIdx.x & 3;
            double ss = 0.0, qq = 0.0;
            for (int q = 0; q < PP; ++q) {
                ss += sred[q * cgs + gq][c];
                qq += sred[q * cgs + gq][4 + c];
            }
            double* dst = g.bn_partial + snn_bn_partial_index(grp, grp_j, threadIdx.x, g.group_blocks, g.Cout);
            dst[0] = ss;
            dst[1] = qq;
        }
    }
    if (WGRAD) {
        // block sum over the PP pixel lanes of every channel group, in lane order; out = workspace, one slab
        // [Cout][KT] per block, summed in fixed order by k_wgrad_reduce
        float* slab = out + (int64_t)blockIdx.x * g.Cout * KT;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int k = 0; k < KT; ++k) red[threadIdx.x][k] = wr[c][k];
            __syncthreads();
            for (int e = threadIdx.x; e < cgs * KT; e += kThreads) {
                const int gq = e / KT, k = e - gq * KT;
                float sum = 0.f;
                for (int q = 0; q < PP; ++q) sum += red[q * cgs + gq][k];
                slab[(gq * 4 + c) * KT + k] = sum;
            }
            __syncthreads();
        }
    }
}

}  // namespace

// the shapes the two kernels above take: the caller checks alignment of its buffers on top
bool snn_first_layer_shape(int Cin, int Cout, int KH, int KW) {
    static const bool off = snn_tuning_env("SNN_CONV_NO_FIRST") != nullptr;  // tuning / bisecting aid
    if (off || Cin != 2 || KH != 3 || KW != 3 || Cout % 4 != 0 || Cout > 256) return false;
    const int cgs = Cout / 4;
    return (cgs & (cgs - 1)) == 0;
}

// output rows a block stages at once: as many as fit 20 KiB of LDS - next to the 19 KiB of reduction scratch both forms
// carry, four blocks per CU stay resident (with 29 KiB the weight gradient fell to three and lost a fifth) - at most 4
static int first_layer_rs(int W, int pad) {
    const int per_row = 3 * (W + 2 * pad) * (int)sizeof(float2);
    int rs = (20 << 10) / per_row;
    return rs < 1 ? 1 : (rs > 4 ? 4 : rs);
}
int snn_first_layer_blocks(int64_t rows, int num_cu) {  // grid of the weight gradient = its slabs
    if (num_cu <= 0) num_cu = snn_num_cu();
    int64_t b = rows < 4 * num_cu ? rows : 4 * num_cu;
    return b < 1 ? 1 : (int)b;
}

// Forward with statistics partials: a group is one timestep, dealt to `blocks` blocks of at most `per_block` rows each
// (about 8 blocks per CU over all timesteps; at least one per timestep)
struct FirstGroups { int rows, blocks; };
static FirstGroups first_layer_groups(int rows_per_step, int steps, int num_cu) {
    int target = 8 * num_cu / (steps > 0 ? steps : 1);
    if (target < 1) target = 1;
    if (target > rows_per_step) target = rows_per_step;
    const int per_block = (rows_per_step + target - 1) / target;
    return {rows_per_step, (rows_per_step + per_block - 1) / per_block};
}

FirstPlan snn_first_layer_plan(int64_t N, int H, int W, int Ho, int Wo, int Cout, int stride, int pad,
                               int frames_per_step, bool wgrad, int num_cu) {
    FirstPlan p = {};
    if (num_cu <= 0) num_cu = snn_num_cu();
    if (!snn_first_layer_shape(2, Cout, 3, 3) || N <= 0 || stride <= 0 || pad < 0 || Ho <= 0 || Wo <= 0 ||
        Ho != (H + 2 * pad - 3) / stride + 1 || Wo != (W + 2 * pad - 3) / stride + 1 || N * (int64_t)Ho >= 0x7fffffffLL ||
        W + 2 * pad > 1408 || (Wo - 1) * stride + 3 > W + 2 * pad)
        return p;
    if (!wgrad && frames_per_step > 0 && N % frames_per_step != 0) return p;
    const int rows = (int)(N * Ho);
    p.rs = first_layer_rs(W, pad);
    p.LW = W + 2 * pad;
    p.cgs = Cout / 4;
    p.PP = kThreads / p.cgs;
    p.lds = (size_t)p.rs * 3 * p.LW * sizeof(float2);
    p.group_rows = rows;
    if (wgrad) {
        p.blocks = p.group_blocks = snn_first_layer_blocks(rows, num_cu);
    } else if (frames_per_step > 0) {
        const int steps = (int)(N / frames_per_step);
        const FirstGroups g = first_layer_groups(frames_per_step * Ho, steps, num_cu);
        p.group_rows = g.rows;
        p.group_blocks = g.blocks;
        p.blocks = steps * g.blocks;
    } else {
        p.blocks = p.group_blocks = rows < 8 * num_cu ? rows : 8 * num_cu;
    }
    // block 0 of a group walks its rows 0, group_blocks, ...: the most of any block; stages of rs rows, the last one partial
    p.max_rows = (p.group_rows + p.group_blocks - 1) / p.group_blocks;
    p.last_stage_rows = (p.max_rows - 1) % p.rs + 1;
    p.ok = 1;
    return p;
}

// the one launch of k_conv_first: the forward (out = y), the weight gradient (out = its slabs; bf16 dy with sb) and the
// weight gradient that applies the BatchNorm backward to its dy operand on the way (fp32 only)
int snn_launch_first(bool wgrad, bool bnapply, bool sb, int blocks, size_t lds, const float* x, const float* w,
                     const float* dy, float* out, const FirstGeom& fg, void* stream, const char* name) {
    dispatch(
        [&](auto WGRAD, auto BNAPPLY, auto SB) {
            if constexpr (!BNAPPLY() || (WGRAD() && !SB())) {
                hipLaunchKernelGGL((k_conv_first<2, 3, WGRAD(), BNAPPLY(), SB()>), dim3((unsigned)blocks), dim3(kThreads), lds,
                                   (hipStream_t)stream, x, w, dy, out, fg);
            }
            return true;
        },
        Flag{wgrad}, Flag{bnapply}, Flag{sb});
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_conv_first_plan(int64_t N, int H, int W, int Ho, int Wo, int Cout, int stride, int pad,
                                   int frames_per_step, int wgrad, int num_cu, int* out) {
    if (!out) return 1;
    const FirstPlan p = snn_first_layer_plan(N, H, W, Ho, Wo, Cout, stride, pad, frames_per_step, wgrad != 0, num_cu);
    const int v[10] = {p.ok, p.rs, p.LW, p.cgs, p.PP, p.blocks, p.group_rows, p.group_blocks, p.max_rows,
                       p.last_stage_rows};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return p.ok ? 0 : 1;
}
