// Depthwise convolution (gfx950): Conv2d(C, C, K, stride, padding = K / 2, groups = C, bias = False) over channels-last
// frames [N = T*B][H][W][ld >= C], K in {3, 5}, stride in {1, 2}, any C >= 1.  2 K^2 flops per 8 bytes moved: a stencil
// bound by its reads and writes, so fp32 storage, exact fp32 products (fmaf) and no MFMA, no operand split, no LDS in the
// forward / data-gradient kernels.  It shares nothing with the implicit-GEMM or halo-resident kernels.
//
// Weight operand of forward and data gradient: the TAP-MAJOR image wt[K*K][C] (wt[kh*K + kw][c] = weight[c][0][kh][kw]) -
// for an (C,1,K,K) parameter exactly what the batched transpose leaves in FlatTrainer.flat_wt.  Consecutive lanes then
// read consecutive channels of one tap.  The weight gradient is written in the PARAMETER's order dw[C][K*K].
//
// A lane owns 4 consecutive channels (the weight gradient for K = 5: 2, see k_dw_wgrad) and uses one 16-byte access per
// pixel when the slice is 16-byte aligned and the pixel stride a multiple of 4; every other layout and the C % 4 tail go
// through guarded scalar accesses with the same arithmetic order (ldv / stv below).
#include "snn_common.h"
#include <algorithm>

namespace {

constexpr int kThreads = 256;

// CPL consecutive channels from channel c of one pixel (p points at channel c); channels >= C read as zero
template <int CPL, bool VEC> __device__ __forceinline__ f32x4 ldv(const float* __restrict__ p, int c, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC && c + CPL <= C) {
        if constexpr (CPL == 4) {
            v = *reinterpret_cast<const f32x4*>(p);
        } else {
            const snn_f32x2 h = *reinterpret_cast<const snn_f32x2*>(p);
            v[0] = h[0];
            v[1] = h[1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (c + j < C) v[j] = p[j];
    }
    return v;
}
// the weight image may start on any float of a flat buffer: its own (wave-uniform) switch
__device__ __forceinline__ f32x4 ldw(const float* __restrict__ p, int c, int C, int wvec) {
    return wvec ? ldv<4, true>(p, c, C) : ldv<4, false>(p, c, C);
}
template <bool VEC> __device__ __forceinline__ void stv(float* __restrict__ p, int c, int C, f32x4 v) {
    if (VEC && c + 4 <= C) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C) p[j] = v[j];
    }
}
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = fmaf(a[j], b[j], c[j]);
    return r;
}

// ---------------------------------------------------------------------------------------------------- forward / dgrad s1
// out[n][ho][wo][c] = sum_kh sum_kw in[n][ho*S - K/2 + kh][wo*S - K/2 + kw][c] * wt[tap(kh, kw)][c], taps in kh-major
// order, one fmaf chain per element.  MIRROR (tap = K*K - 1 - (kh*K + kw)) with S = 1 is the data gradient of the
// stride-1 layer.  A lane produces RUN output pixels along W for its 4 channels: each input row's (RUN-1)*S + K columns
// are loaded once and reused from registers; the K row re-reads come from L1 / L2.  Work items: (row = n*Ho + ho, run,
// channel group), channel group fastest - the lanes of a wave read consecutive 16-byte pieces of a pixel.
template <int K, int S, bool MIRROR, bool VEC>
__global__ __launch_bounds__(kThreads) void k_dw_fwd(const float* __restrict__ x, int64_t ldx, const float* __restrict__ wt,
                                                      int wvec, float* __restrict__ y, int64_t ldy, int H, int W, int Ho,
                                                      int Wo, int C, int CG, int WR, int64_t total) {
    constexpr int RUN = S == 1 ? 4 : 2;
    constexpr int COLS = (RUN - 1) * S + K;
    constexpr int PAD = K / 2;
    const int per_row = WR * CG;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / per_row;
        const int it = (int)(idx - row * per_row);
        const int wr = it / CG;
        const int c = (it - wr * CG) * 4;
        const int64_t n = row / Ho;
        const int ho = (int)(row - n * Ho);
        const int wo0 = wr * RUN;
        const int wi0 = wo0 * S - PAD;
        f32x4 acc[RUN];
#pragma unroll
        for (int r = 0; r < RUN; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const int hi = ho * S - PAD + kh;
            if (hi < 0 || hi >= H) continue;
            f32x4 wv[K];
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const int tap = MIRROR ? K * K - 1 - (kh * K + kw) : kh * K + kw;
                wv[kw] = ldw(wt + (int64_t)tap * C + c, c, C, wvec);
            }
            const float* xr = x + ((n * H + hi) * W) * ldx + c;
            f32x4 col[COLS];
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int wi = wi0 + j;
                col[j] = (wi >= 0 && wi < W) ? ldv<4, VEC>(xr + (int64_t)wi * ldx, c, C) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < RUN; ++r)
#pragma unroll
                for (int kw = 0; kw < K; ++kw) acc[r] = fma4(col[r * S + kw], wv[kw], acc[r]);
        }
        float* yr = y + ((n * Ho + ho) * Wo) * ldy + c;
#pragma unroll
        for (int r = 0; r < RUN; ++r)
            if (wo0 + r < Wo) stv<VEC>(yr + (int64_t)(wo0 + r) * ldy, c, C, acc[r]);
    }
}

// ---------------------------------------------------------------------------------------------------- dgrad, stride 2
// dx[n][h][w][c] = sum over the taps whose phase matches: kh = (h + K/2) mod 2, + 2, ..., ho = (h + K/2 - kh) / 2 inside
// [0, Ho) (kw alike): a gather - one pass over dy, no atomics, every dx element written exactly once (a pixel no tap
// reaches gets zero).  One dx pixel x 4 channels per lane.
template <int K, bool VEC>
__global__ __launch_bounds__(kThreads) void k_dw_dgrad_s2(const float* __restrict__ dy, int64_t lddy,
                                                           const float* __restrict__ wt, int wvec, float* __restrict__ dx,
                                                           int64_t lddx, int H, int W, int Ho, int Wo, int C, int CG,
                                                           int64_t total) {
    constexpr int PAD = K / 2;
    constexpr int NT = (K + 1) / 2;   // taps of one phase per dimension, at the most
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t pix64 = idx / CG;
        const int c = (int)(idx - pix64 * CG) * 4;
        const unsigned pix = (unsigned)pix64;   // N*H*W < 2^31 (snn_dwconv_supported)
        const unsigned nh = pix / (unsigned)W;
        const int w = (int)(pix - nh * (unsigned)W);
        const unsigned n = nh / (unsigned)H;
        const int h = (int)(nh - n * (unsigned)H);
        const int kh0 = (h + PAD) & 1, kw0 = (w + PAD) & 1;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int kh = kh0 + 2 * a;
            const int ho = (h + PAD - kh) >> 1;
            if (kh >= K || h + PAD - kh < 0 || ho >= Ho) continue;
            const float* dr = dy + (((int64_t)n * Ho + ho) * Wo) * lddy + c;
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const int kw = kw0 + 2 * b;
                const int wo = (w + PAD - kw) >> 1;
                if (kw >= K || w + PAD - kw < 0 || wo >= Wo) continue;
                const f32x4 g = ldv<4, VEC>(dr + (int64_t)wo * lddy, c, C);
                const f32x4 wv = ldw(wt + (int64_t)(kh * K + kw) * C + c, c, C, wvec);
                acc = fma4(g, wv, acc);
            }
        }
        stv<VEC>(dx + (int64_t)pix * lddx + c, c, C, acc);
    }
}

// ---------------------------------------------------------------------------------------------------- weight gradient
// dw[c][tap] = sum over the P = N*Ho*Wo output pixels of x[n][ho*S - K/2 + kh][wo*S - K/2 + kw][c] * dy[n][ho][wo][c].
// Grid: pixel chunks (x) by blocks of BC channel groups (y); in a block BC lanes lie side by side over the channels and
// PL = 256 / BC lanes over the pixels.  A lane keeps K*K x CPL fp32 accumulators over at most kLaneTerms of its pixels
// (fmaf chain: error <= kLaneTerms * 2^-24 of the sum of |products| = the 2^-19 of the per-element tests), then the block
// adds the PL lanes of every (channel, tap) through LDS in fp64, in lane order, into fp64 registers that live for the
// whole chunk - everything above kLaneTerms products is summed in fp64.  One slab row [C][K*K] (fp64) per chunk; k_dw_wgrad_sum
// adds the rows in fixed order.  No atomics: the same call gives the same bits.
// CPL: channels per lane.  4 for K = 3 (36 accumulators, 36 KiB of LDS); K = 5 takes 2 (50 accumulators, 50 KiB: three
// blocks per CU) - with 4 it would hold 100 accumulators beside its operands and 100 KiB.
constexpr int kLaneTerms = 32;
constexpr int kMaxBC = 64;

template <int K, int S, int CPL, bool VEC>
__global__ __launch_bounds__(kThreads) void k_dw_wgrad(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ dy, int64_t lddy,
                                                        double* __restrict__ slab, int64_t P, int H, int W, int Ho, int Wo,
                                                        int C, int bc_log2, int64_t chunk_len) {
    constexpr int KK = K * K, NA = KK * CPL, PAD = K / 2;
    constexpr int MAXO = (kMaxBC * NA + kThreads - 1) / kThreads;
    __shared__ float red[NA * kThreads];
    const int tid = threadIdx.x;
    const int bc = 1 << bc_log2, pl = kThreads >> bc_log2;
    const int cgl = tid & (bc - 1), q = tid >> bc_log2;
    const int c = (int)((blockIdx.y * bc + cgl) * CPL);
    const int64_t p0 = (int64_t)blockIdx.x * chunk_len;
    const int64_t p1 = p0 + chunk_len < P ? p0 + chunk_len : P;
    double tot[MAXO];
#pragma unroll
    for (int i = 0; i < MAXO; ++i) tot[i] = 0.0;
    for (int64_t sub = p0; sub < p1; sub += (int64_t)kLaneTerms * pl) {   // (block-uniform trip count: barriers inside)
        float acc[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[a] = 0.f;
        if (c < C) {
            for (int it = 0; it < kLaneTerms; ++it) {
                const int64_t p64 = sub + (int64_t)it * pl + q;
                if (p64 >= p1) break;
                const unsigned p = (unsigned)p64;   // P < 2^31 (snn_dwconv_supported)
                const unsigned nh = p / (unsigned)Wo;
                const int wo = (int)(p - nh * (unsigned)Wo);
                const unsigned n = nh / (unsigned)Ho;
                const int ho = (int)(nh - n * (unsigned)Ho);
                const f32x4 g = ldv<CPL, VEC>(dy + (int64_t)p * lddy + c, c, C);
#pragma unroll
                for (int kh = 0; kh < K; ++kh) {
                    const int hi = ho * S - PAD + kh;
                    if (hi < 0 || hi >= H) continue;
                    const float* xr = x + (((int64_t)n * H + hi) * W) * ldx + c;
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) {
                        const int wi = wo * S - PAD + kw;
                        if (wi < 0 || wi >= W) continue;
                        const f32x4 v = ldv<CPL, VEC>(xr + (int64_t)wi * ldx, c, C);
#pragma unroll
                        for (int j = 0; j < CPL; ++j)
                            acc[(kh * K + kw) * CPL + j] = fmaf(v[j], g[j], acc[(kh * K + kw) * CPL + j]);
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) red[a * kThreads + tid] = acc[a];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MAXO; ++i) {
            const int o = tid + i * kThreads;   // (accumulator a, channel lane l) of the block, l fastest
            if (o < bc * NA) {
                const int a = o >> bc_log2, l = o & (bc - 1);
                double s = 0.0;
                for (int qq = 0; qq < pl; ++qq) s += (double)red[a * kThreads + qq * bc + l];
                tot[i] += s;
            }
        }
        __syncthreads();
    }
    double* row = slab + (int64_t)blockIdx.x * C * KK;
#pragma unroll
    for (int i = 0; i < MAXO; ++i) {
        const int o = tid + i * kThreads;
        if (o < bc * NA) {
            const int a = o >> bc_log2, l = o & (bc - 1);
            const int co = (int)((blockIdx.y * bc + l) * CPL) + a % CPL;
            if (co < C) row[(int64_t)co * KK + a / CPL] = tot[i];
        }
    }
}

// dw[o] (+)= sum over the chunks of slab[chunk][o], o over C*K*K: 8 outputs x 32 chunk lanes per block, each lane adds
// every 32nd row, the 32 partial sums are added in lane order - fp64 throughout, one rounding to fp32 at the end.
__global__ __launch_bounds__(kThreads) void k_dw_wgrad_sum(const double* __restrict__ slab, float* __restrict__ dw,
                                                            int n_out, int chunks, int accumulate) {
    __shared__ double sh[kThreads];
    const int ol = threadIdx.x & 7, ql = threadIdx.x >> 3;
    const int o = blockIdx.x * 8 + ol;
    double s = 0.0;
    if (o < n_out)
        for (int ch = ql; ch < chunks; ch += 32) s += slab[(int64_t)ch * n_out + o];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (ql == 0 && o < n_out) {
        double t = accumulate ? (double)dw[o] : 0.0;
        for (int qq = 0; qq < 32; ++qq) t += sh[qq * 8 + ol];
        dw[o] = (float)t;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static bool dw_supported(int64_t N, int H, int W, int C, int K, int stride, int pad) {
    if (!(K == 3 || K == 5) || !(stride == 1 || stride == 2) || pad != K / 2) return false;
    if (N < 1 || H < 1 || W < 1 || C < 1) return false;
    // pixel indices are 32-bit in the kernels (element offsets are 64-bit)
    return N <= (int64_t)0x7fffffff / ((int64_t)H * W);
}
static int out_size(int n, int K, int stride) { return (n + 2 * (K / 2) - K) / stride + 1; }

struct DwWgradPlan {
    int cpl, bc_log2, gy, chunks;
    int64_t chunk_len, P;
};
constexpr int kMaxChunks = 1 << 20;
constexpr int kTargetBlocks = 1024;   // four 256-thread blocks per CU on 256 CUs; a constant: the plan needs no device

static DwWgradPlan dw_wgrad_plan(int64_t N, int H, int W, int C, int K, int stride, int chunks) {
    DwWgradPlan p;
    p.cpl = K == 3 ? 4 : 2;
    const int cgn = (C + p.cpl - 1) / p.cpl;
    p.bc_log2 = 0;
    while ((1 << p.bc_log2) < cgn && (1 << p.bc_log2) < kMaxBC) ++p.bc_log2;
    const int bc = 1 << p.bc_log2;
    p.gy = (cgn + bc - 1) / bc;
    p.P = N * out_size(H, K, stride) * out_size(W, K, stride);
    if (chunks <= 0) {
        const int64_t by_work = snn_ceil_div(p.P, (int64_t)kLaneTerms * (kThreads / bc));
        chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(1, kTargetBlocks / p.gy), by_work));
    }
    p.chunks = chunks;
    p.chunk_len = snn_ceil_div(p.P, chunks);
    return p;
}

}  // namespace

extern "C" int snn_dwconv_supported(int64_t N, int H, int W, int C, int K, int stride, int pad) {
    return dw_supported(N, H, W, C, K, stride, pad) ? 1 : 0;
}

// forward (mirror = false) and the stride-1 data gradient (mirror = true, in / out of one size)
static int dw_stencil(const char* fn, bool mirror, const float* in, int64_t ldi, const float* wt, float* out, int64_t ldo,
                      int64_t N, int H, int W, int C, int K, int stride, hipStream_t st) {
    const int Ho = out_size(H, K, stride), Wo = out_size(W, K, stride);
    const int run = stride == 1 ? 4 : 2;
    const int CG = (C + 3) / 4, WR = (Wo + run - 1) / run;
    SNN_REQUIRE((int64_t)WR * CG <= 0x7fffffff, "%s: a row of %d pixels x %d channels is too long", fn, Wo, C);
    const int64_t total = N * Ho * WR * CG;
    const bool vec = aligned(16, {in, out}) && multiples(4, {ldi, ldo});
    const int wvec = aligned(16, {wt}) && C % 4 == 0;
    const bool launched = dispatch(
        [&](auto KC, auto SC, auto MI, auto VEC) {
            if constexpr (!(MI() && SC() == 2)) {
                hipLaunchKernelGGL((k_dw_fwd<KC(), SC(), MI(), VEC()>), dim3(snn_grid_for(total, kThreads)), dim3(kThreads),
                                   0, st, in, ldi, wt, wvec, out, ldo, H, W, Ho, Wo, C, CG, WR, total);
                return true;
            }
            return false;
        },
        OneOf<3, 5>{K}, OneOf<1, 2>{stride}, Flag{mirror}, Flag{vec});
    SNN_REQUIRE(launched, "%s: no kernel instance (K %d, stride %d)", fn, K, stride);
    SNN_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int snn_dwconv_fwd(const float* x, int64_t ldx, const float* wt, float* y, int64_t ldy, int64_t N, int H, int W,
                              int C, int K, int stride, int pad, void* stream) {
    SNN_REQUIRE(x && wt && y, "snn_dwconv_fwd: null pointer");
    SNN_REQUIRE(dw_supported(N, H, W, C, K, stride, pad),
                "snn_dwconv_fwd: not covered (N %lld, %dx%d, C %d, K %d, stride %d, pad %d): K in {3, 5}, stride in {1, 2}, "
                "pad = K / 2", (long long)N, H, W, C, K, stride, pad);
    SNN_REQUIRE(ldx >= C && ldy >= C, "snn_dwconv_fwd: pixel strides %lld / %lld below the %d channels", (long long)ldx,
                (long long)ldy, C);
    return dw_stencil("snn_dwconv_fwd", false, x, ldx, wt, y, ldy, N, H, W, C, K, stride, (hipStream_t)stream);
}

extern "C" int snn_dwconv_dgrad(const float* dy, int64_t lddy, const float* wt, float* dx, int64_t lddx, int64_t N, int H,
                                int W, int C, int K, int stride, int pad, void* stream) {
    SNN_REQUIRE(dy && wt && dx, "snn_dwconv_dgrad: null pointer");
    SNN_REQUIRE(dw_supported(N, H, W, C, K, stride, pad),
                "snn_dwconv_dgrad: not covered (N %lld, %dx%d, C %d, K %d, stride %d, pad %d): K in {3, 5}, stride in "
                "{1, 2}, pad = K / 2", (long long)N, H, W, C, K, stride, pad);
    SNN_REQUIRE(lddy >= C && lddx >= C, "snn_dwconv_dgrad: pixel strides %lld / %lld below the %d channels",
                (long long)lddy, (long long)lddx, C);
    hipStream_t st = (hipStream_t)stream;
    if (stride == 1)   // Ho = H, Wo = W: the forward stencil over dy with mirrored taps
        return dw_stencil("snn_dwconv_dgrad", true, dy, lddy, wt, dx, lddx, N, H, W, C, K, 1, st);
    const int Ho = out_size(H, K, 2), Wo = out_size(W, K, 2);
    const int CG = (C + 3) / 4;
    const int64_t total = N * H * W * CG;
    const bool vec = aligned(16, {dy, dx}) && multiples(4, {lddy, lddx});
    const int wvec = aligned(16, {wt}) && C % 4 == 0;
    const bool launched = dispatch(
        [&](auto KC, auto VEC) {
            hipLaunchKernelGGL((k_dw_dgrad_s2<KC(), VEC()>), dim3(snn_grid_for(total, kThreads)), dim3(kThreads), 0, st, dy,
                               lddy, wt, wvec, dx, lddx, H, W, Ho, Wo, C, CG, total);
            return true;
        },
        OneOf<3, 5>{K}, Flag{vec});
    SNN_REQUIRE(launched, "snn_dwconv_dgrad: no kernel instance (K %d)", K);
    SNN_CHECK_LAUNCH("snn_dwconv_dgrad");
    return 0;
}

extern "C" size_t snn_dwconv_wgrad_workspace_size(int64_t N, int H, int W, int C, int K, int stride, int pad, int chunks) {
    if (!dw_supported(N, H, W, C, K, stride, pad) || chunks < 0 || chunks > kMaxChunks) return 0;
    const DwWgradPlan p = dw_wgrad_plan(N, H, W, C, K, stride, chunks);
    return (size_t)p.chunks * C * K * K * sizeof(double);
}

extern "C" int snn_dwconv_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, int64_t N, int H,
                                int W, int C, int K, int stride, int pad, int accumulate, void* workspace, int chunks,
                                void* stream) {
    SNN_REQUIRE(x && dy && dw && workspace, "snn_dwconv_wgrad: null pointer");
    SNN_REQUIRE(dw_supported(N, H, W, C, K, stride, pad),
                "snn_dwconv_wgrad: not covered (N %lld, %dx%d, C %d, K %d, stride %d, pad %d): K in {3, 5}, stride in "
                "{1, 2}, pad = K / 2", (long long)N, H, W, C, K, stride, pad);
    SNN_REQUIRE(ldx >= C && lddy >= C, "snn_dwconv_wgrad: pixel strides %lld / %lld below the %d channels", (long long)ldx,
                (long long)lddy, C);
    SNN_REQUIRE(chunks >= 0 && chunks <= kMaxChunks, "snn_dwconv_wgrad: %d chunks (0 = the kernel's plan, at most %d)",
                chunks, kMaxChunks);
    SNN_REQUIRE(aligned(8, {workspace}), "snn_dwconv_wgrad: the workspace holds doubles (8-byte aligned)");
    SNN_REQUIRE((int64_t)C * K * K <= 0x7fffffff, "snn_dwconv_wgrad: %d channels are too many", C);
    hipStream_t st = (hipStream_t)stream;
    const DwWgradPlan p = dw_wgrad_plan(N, H, W, C, K, stride, chunks);
    SNN_REQUIRE(p.gy <= 65535, "snn_dwconv_wgrad: %d channels are too many", C);
    const int Ho = out_size(H, K, stride), Wo = out_size(W, K, stride);
    const size_t ab = p.cpl * sizeof(float);   // a lane's access
    const bool vec = aligned(ab, {x, dy}) && multiples(p.cpl, {ldx, lddy});
    double* slab = static_cast<double*>(workspace);
    const bool launched = dispatch(
        [&](auto KC, auto SC, auto VEC) {
            constexpr int CPL = KC() == 3 ? 4 : 2;
            hipLaunchKernelGGL((k_dw_wgrad<KC(), SC(), CPL, VEC()>), dim3((unsigned)p.chunks, (unsigned)p.gy),
                               dim3(kThreads), 0, st, x, ldx, dy, lddy, slab, p.P, H, W, Ho, Wo, C, p.bc_log2, p.chunk_len);
            return true;
        },
        OneOf<3, 5>{K}, OneOf<1, 2>{stride}, Flag{vec});
    SNN_REQUIRE(launched, "snn_dwconv_wgrad: no kernel instance (K %d, stride %d)", K, stride);
    SNN_CHECK_LAUNCH("snn_dwconv_wgrad");
    const int n_out = C * K * K;
    hipLaunchKernelGGL(k_dw_wgrad_sum, dim3((unsigned)snn_ceil_div(n_out, 8)), dim3(kThreads), 0, st, slab, dw, n_out,
                       p.chunks, accumulate);
    SNN_CHECK_LAUNCH("snn_dwconv_wgrad");
    return 0;
}
