// Implicit-GEMM weight gradient of the 2-D convolutions on the gfx950 matrix cores (see conv_gather.hip for the forward /
// data gradient and the precision modes; conv_common.h for what the two share).
//
//   weight-gradient:
//       dw[co][kc] = sum_pix dy[pix][co] * xg[pix][kc],  kc = (tap, ci)
//     block tile up to 128 x 128 over (co, kc) (six variants, least padding wins), K = pixels, split over
//     pixel ranges sized to ONE resident wave of blocks, splits pinned to XCDs (L2 reuse of dy / x),
//     workspace slabs reduced in fixed order by k_wgrad_reduce (bitwise reproducible).
//
//
// The event-frame layer (Cin = 2) and the 3x3 layers with whole 32-channel tiles go to their own kernels from here:
// k_conv_first (conv_first.hip) and k_conv_wgrad_halo (wgrad_halo.hip); all three write slabs the reducers below sum.
#include <stdlib.h>
#include <type_traits>
#include "conv_common.h"

namespace {

// ------------------------------------------------------------------------------------------ wgrad
constexpr int WB_K = 32;   // pixels per LDS stage

struct WgradGeom {
    int64_t Mtot;  // N * Ho * Wo
    int H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int64_t ldx, lddy;
    int Ktot;
    int64_t pix_per_split;
    int tiles_m, tiles_n, splitk;
    int nimg;
    float x_th;    // XSP kernels: x holds saved LIF potentials, the operand is z = (v_dec > x_th)
};

// Block tile (32*TM*WM) out-channels x (32*TN*WN) (tap,ci) columns; each wave owns TM x TN accumulators of
// 32x32.  K = pixels, 32 per LDS stage; the decode pixel -> (image base, y0, x0) of a stage is done by 32
// lanes and published through LDS one stage ahead.  Blocks of one pixel split are mapped to one XCD
// (block ids congruent mod 8) so the dy / x tiles they share are served from that XCD's L2.
template <int TM, int TN, int WM, int WN, bool VEC>
__global__ __launch_bounds__(kThreads, SNN_CONV_MIN_WAVES) void k_conv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ ws, WgradGeom g) {
    static_assert(WM * WN == 4, "4 waves");
    constexpr int BMc = 32 * TM * WM, BNk = 32 * TN * WN;
    constexpr int DG = BMc / 4, XG = BNk / 4;       // float4 groups per pixel row
    constexpr int DP = kThreads / DG, XP = kThreads / XG;  // pixel rows per pass
    constexpr int DJ = WB_K / DP, XJ = WB_K / XP;   // passes per stage
    static_assert(DJ >= 1 && XJ >= 1, "tile too narrow");
    __shared__ __attribute__((aligned(16))) float Ds[WB_K * BMc];
    __shared__ __attribute__((aligned(16))) float Xs[WB_K * BNk];
    __shared__ int Pinfo[2][WB_K][4];  // {image base pixel, y0, x0, valid}

    const int tid = threadIdx.x;
    const int lane_id = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane_id & 31, h = lane_id >> 5;

    // ---- block -> (tile, split): blocks L, L+8, L+16, ... (one XCD) walk the tiles of one split
    const int tiles = g.tiles_m * g.tiles_n;
    int L = blockIdx.x, z, tile;
    if (g.splitk % 8 == 0) {
        z = (L % 8) + 8 * (L / (8 * tiles));
        tile = (L / 8) % tiles;
    } else {
        z = L / tiles;
        tile = L % tiles;
    }
    const int co0 = (tile % g.tiles_m) * BMc;
    const int kc0 = (tile / g.tiles_m) * BNk;
    const int64_t p_lo = (int64_t)z * g.pix_per_split;
    int64_t p_hi = p_lo + g.pix_per_split;
    if (p_hi > g.Mtot) p_hi = g.Mtot;

    // ---- loader geometry
    const int d_cq = (tid % DG) * 4, d_pr = tid / DG;
    const int x_cq = (tid % XG) * 4, x_pr = tid / XG;
    int x_kh[4], x_kw[4], x_ci[4];
    bool x_ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int kc = kc0 + x_cq + e;
        x_ok[e] = kc < g.Ktot;
        int kcc = x_ok[e] ? kc : 0;
        int tap = kcc / g.Cin;
        x_ci[e] = kcc - tap * g.Cin;
        x_kh[e] = tap / g.KW;
        x_kw[e] = tap - x_kh[e] * g.KW;
    }
    const bool d_ok = (co0 + d_cq) < g.Cout;

    // Pixel decode (image, oy, ox) of the 32 pixels of a stage: lane t < 32 owns pixel p0 + t, decodes it ONCE
    // with a division and then walks forward 32 pixels per stage with carries (no division in the loop).
    int d_img = 0, d_oy = 0, d_ox = 0;
    int64_t d_p = p_lo + tid;
    if (tid < WB_K) {
        int64_t pp = d_p < g.Mtot ? d_p : 0;
        d_ox = (int)(pp % g.Wo);
        int64_t t = pp / g.Wo;
        d_oy = (int)(t % g.Ho);
        d_img = (int)(t / g.Ho);
    }
    auto decode = [&](int slot) {  // publish the current stage's pixels, then advance to the next stage
        if (tid < WB_K) {
            Pinfo[slot][tid][0] = d_p < p_hi ? d_img * g.H * g.W : 0;  // invalid pixels read (and discard) image 0
            Pinfo[slot][tid][1] = d_oy * g.stride - g.pad;
            Pinfo[slot][tid][2] = d_ox * g.stride - g.pad;
            Pinfo[slot][tid][3] = d_p < p_hi ? 1 : 0;
            d_p += WB_K;
            d_ox += WB_K;
            while (d_ox >= g.Wo) {
                d_ox -= g.Wo;
                if (++d_oy == g.Ho) {
                    d_oy = 0;
                    ++d_img;
                }
            }
        }
    };

    f32x4 rd[DJ], rx[XJ];
    auto load_tiles = [&](int64_t p0, int slot) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            const int row = d_pr + DP * j;
            const int64_t p = p0 + row;
            const bool ok = p < p_hi;
            const int64_t pc = ok ? p : 0;  // clamped address: always load, mask afterwards (no branch)
            f32x4 v = zero;
            if (VEC) {
                v = *reinterpret_cast<const f32x4*>(dy + pc * g.lddy + (d_ok ? co0 + d_cq : 0));
                v = (ok & d_ok) ? v : zero;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ok && co0 + d_cq + e < g.Cout) v[e] = dy[p * g.lddy + co0 + d_cq + e];
            }
            rd[j] = v;
        }
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int row = x_pr + XP * j;
            const int ibase = Pinfo[slot][row][0], y0 = Pinfo[slot][row][1], x0 = Pinfo[slot][row][2];
            const bool pok = Pinfo[slot][row][3] != 0;
            f32x4 v = zero;
            if (VEC) {
                const int iy = y0 + x_kh[0], ix = x0 + x_kw[0];
                const bool ok = pok & x_ok[0] & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
                const int iyc = min(max(iy, 0), g.H - 1), ixc = min(max(ix, 0), g.W - 1);
                v = *reinterpret_cast<const f32x4*>(x + (int64_t)(ibase + iyc * g.W + ixc) * g.ldx + x_ci[0]);
                v = ok ? v : zero;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int iy = y0 + x_kh[e], ix = x0 + x_kw[e];
                    if (pok && x_ok[e] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
                        v[e] = x[(int64_t)(ibase + iy * g.W + ix) * g.ldx + x_ci[e]];
                }
            }
            rx[j] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int j = 0; j < DJ; ++j) *reinterpret_cast<f32x4*>(&Ds[(d_pr + DP * j) * BMc + d_cq]) = rd[j];
#pragma unroll
        for (int j = 0; j < XJ; ++j) *reinterpret_cast<f32x4*>(&Xs[(x_pr + XP * j) * BNk + x_cq]) = rx[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    decode(0);
    __syncthreads();
    load_tiles(p_lo, 0);
    decode(1);
    store_tiles();
    __syncthreads();

    int slot = 1;
#pragma unroll 1
    for (int64_t p0 = p_lo; p0 < p_hi; p0 += WB_K) {
        load_tiles(p0 + WB_K, slot);  // rows past p_hi load zeros
        decode(slot ^ 1);             // pixels of stage p0 + 2*WB_K; slot^1 was last read before a barrier
#pragma unroll
        for (int ks = 0; ks < WB_K / 2; ++ks) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Ds[(ks * 2 + h) * BMc + (wm * TM + i) * 32 + r];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Xs[(ks * 2 + h) * BNk + (wn * TN + j) * 32 + r];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        store_tiles();
        __syncthreads();
        slot ^= 1;
    }

    float* slab = ws + (int64_t)z * g.Cout * (int64_t)g.Ktot;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int kc = kc0 + (wn * TN + j) * 32 + r;
            if (kc >= g.Ktot) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (co < g.Cout) slab[(int64_t)co * g.Ktot + kc] = acc[i][j][e];
            }
        }
}

// bf16 x 3 weight gradient (see k_conv_gather<..., SPLIT>): both operands are split into bf16 hi / lo on the way into
// LDS.  K = pixels must be contiguous per lane for the bf16 MFMA, so every loader thread takes FOUR consecutive
// pixels of its 4-channel group, transposes the 4x4 block in registers and writes [column][pixel] images.
// Host-checked: one pixel split of x spans < 2 GiB, so 32-bit byte offsets relative to the split's first image
// address every gathered pixel (larger problems take the exact-fp32 kernel above).  Pipelined like k_conv_gather:
//   * raw buffer loads with hardware range checking (offset 0xFFFFFFFF -> zeros): no clamps, selects or 64-bit
//     address arithmetic; dy rows past the split's last pixel fall off the end of the buffer resource;
//   * tile k+1 is converted to its bf16 pieces in the shadow of tile k's MFMAs and the loads of tile k+2 are
//     issued before the barrier; between the two barriers only the LDS writes remain.
// SB (ONE only; bf16-storage mode): x and dy are bf16 tensors - 8-byte loads, the 4 x 4 transposition to "4 pixels of a
// channel" is bit shuffling, nothing is converted.
// XSP (bf16 x 3 only; snn_conv1x1_spikes_wgrad): x holds the saved potentials v_dec of a LIF layer that wrote no spike tensor
// (see k_conv_gather XSP); the operand z = (v_dec > x_th) is formed in the conversion - one exact bf16 piece (0x3F80 or 0),
// no low image, and the product high(dy) * low(x) is not issued: two MFMA products per multiply-add.
// XM (XSP only; snn_conv1x1_mask_wgrad, 1x1 / stride 1): x is the spike BIT MASK of the scan (SNN_SCAN_SPIKE_MASK): uint32
// [pixel][ldx], bit ci & 31 of word ci >> 5.  A stage's x operand is WBK words per 32-column group - ONE 4-byte load per
// thread (at most one load instruction per wave and stage, against 4 * XQ 16-byte ones), staged as words (Xw[group][pixel]);
// lane (r, h) reads the 8 words of its 8 pixels (two broadcast ds_read_b128) and takes bit r of each as a bf16 1.0 / 0.  The
// MFMAs, their operands' bits and their order are those of XSP.
// DX (bf16 x 3, 1x1 / stride 1, the block owns every output channel: tiles_m == 1; snn_conv1x1_bwd / snn_conv1x1_mask_bwd): the
// kernel also writes the DATA gradient of its stage pixels and its column tile, dx[pixel][kc0 ..] = sum_co dy[pixel][co] *
// wt[ci][co] (+ up to two addends), so dy is read from HBM once for both gradients.  dx contracts over co, the ROW index of
// the dy images the weight gradient reads by rows: the same images are read with the transposing LDS read
// (ds_read_b64_tr_b16, 4 co x 16 pixels per 16-lane group) - no second image, no register transposition.  Each wave owns
// one 32-ci x 32-pixel tile of the stage; its wt rows (all co chunks, bf16 hi / lo) are loaded and split ONCE per block
// and stay in registers.  wt is the A operand (rows = ci), dy the B operand (columns = pixels): the accumulator of a lane
// then holds 4 x 4 CONSECUTIVE ci of one pixel - 16-byte addend loads and dx stores straight from the registers, no
// staging through LDS - and the sums are those of k_conv_gather<DGRAD> (dy as A, wt as B): per 16-wide co chunk in
// ascending order dy_lo * w_hi, dy_hi * w_lo, dy_hi * w_hi, the k slots of a chunk in the same order.  The slabs are
// untouched: same splits, stages and k slots as the kernel without DX.
struct WgradDx {
    const float* wt;       // [Cin][Cout]
    float* dx;
    const float* add1;     // nullptr: none
    const float* add2;
    int64_t lddx, ld_add1, ld_add2;
};
typedef short s16x4 __attribute__((ext_vector_type(4)));
template <int TM, int TN, int WM, int WN, int WBK, bool ONE, bool SB = false, bool XSP = false, bool XM = false, bool DX = false>   // ONE: bf16 x 1 (hi pieces only, one product)
// (DX on the 128 x 128 tile with fp32 x - 64 accumulator, 64 wt-fragment and 64 operand-pipeline registers - spills at two
// waves per SIMD: that one instance is compiled for one)
__global__ __launch_bounds__(kThreads, (DX && TM * TN == 4 && !XM) ? 1 : 2) void k_conv_wgrad_pipe(const float* __restrict__ x,
                                                                 const float* __restrict__ dy,
                                                                 float* __restrict__ ws, WgradGeom g, WgradDx d) {
    static_assert(WM * WN == 4, "4 waves");
    constexpr int BMc = 32 * TM * WM, BNk = 32 * TN * WN;
    static_assert(!DX || (!ONE && !SB && XSP == XM), "fused data gradient: bf16 x 3 on fp32 x or on the spike bit mask");
    static_assert(!DX || (BNk / 32) * (WBK / 32) == 4, "fused data gradient: one 32 x 32 dx tile per wave and stage");
    constexpr int DG = BMc / 4, XG = BNk / 4;
    // WBK pixels per LDS stage: 32 for the large tiles; 64 for the small ones, whose 6-MFMA stages were shorter than
    // the memory latency they have to cover (PMC: 58 % of the wave cycles parked in s_waitcnt / barriers)
    static_assert(WBK == 32 || WBK == 64, "stage length");
    static_assert(!SB || ONE, "bf16 storage: one product");
    static_assert(!XSP || (!ONE && !SB), "spikes from potentials: the bf16 x 3 kernel");
    static_assert(!XM || XSP, "spike bit mask: an instance of the spikes-from-potentials kernel");
    constexpr int XW = ((BNk / 32) * WBK + kThreads - 1) / kThreads;   // XM: mask words per thread and stage (1, 2 for the widest tile)
    constexpr int ES = SB ? 2 : 4;   // bytes per activation element in HBM
    constexpr int LDW = WBK + 8;      // bf16 row pitch: 80 / 144 bytes, conflict-free ds_read_b128 fragments
    constexpr int NQ = WBK / 4;       // pixel quads per stage
    constexpr int GPP = kThreads / NQ;
    constexpr int DQ = (DG + GPP - 1) / GPP, XQ = (XG + GPP - 1) / GPP;
    __shared__ __attribute__((aligned(16))) __bf16 Dh[BMc * LDW];
    __shared__ __attribute__((aligned(16))) __bf16 Dl[ONE ? 8 : BMc * LDW];
    __shared__ __attribute__((aligned(16))) __bf16 Xh[XM ? 8 : BNk * LDW];
    __shared__ __attribute__((aligned(16))) __bf16 Xl[(ONE || XSP) ? 8 : BNk * LDW];
    __shared__ __attribute__((aligned(16))) unsigned Xw[XM ? XW * kThreads : 4];   // XM: [32-column group][WBK pixels] = [tid + kThreads * k]
    __shared__ __attribute__((aligned(16))) int Pinfo[2][WBK][4];  // {byte offset of the pixel origin, y0, x0, valid}

    const int tid = threadIdx.x;
    const int lane_id = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane_id & 31, h = lane_id >> 5;

    const int tiles = g.tiles_m * g.tiles_n;
    int L = blockIdx.x, z, tile;
    if (g.splitk % 8 == 0) {
        z = (L % 8) + 8 * (L / (8 * tiles));
        tile = (L / 8) % tiles;
    } else {
        z = L / tiles;
        tile = L % tiles;
    }
    const int co0 = (tile % g.tiles_m) * BMc;
    const int kc0 = (tile / g.tiles_m) * BNk;
    const unsigned p_lo = (unsigned)((int64_t)z * g.pix_per_split);
    unsigned p_hi = p_lo + (unsigned)g.pix_per_split;
    if (p_hi > (unsigned)g.Mtot) p_hi = (unsigned)g.Mtot;
    if (p_lo >= p_hi) p_hi = p_lo;  // an empty split still writes its (zero) slab

    // ---- buffer resources: dy rows of this split, x from the split's first image on
    const unsigned opix = (unsigned)(g.Ho * g.Wo), ipix = (unsigned)(g.H * g.W);
    const unsigned img_lo = p_lo / opix;
    __amdgpu_buffer_rsrc_t rs_d, rs_x;
    {
        const int64_t dbytes = p_hi > p_lo ? (((int64_t)(p_hi - p_lo) - 1) * g.lddy + g.Cout) * ES : 0;
        rs_d = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(dy) + (int64_t)p_lo * g.lddy * ES), 0, (int)dbytes, 0x00020000);
        const int64_t xbytes = ((((int64_t)g.nimg - img_lo) * ipix - 1) * g.ldx + g.Cin) * ES;
        rs_x = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(x) + (int64_t)img_lo * ipix * g.ldx * ES), 0,
                                                 xbytes > 0x7fffffffLL ? 0x7fffffff : (xbytes < 0 ? 0 : (int)xbytes), 0x00020000);
    }

    // ---- loader geometry: 4 consecutive lanes take 4 consecutive channel groups (64 contiguous bytes) of one pixel
    // quad, the next 4 lanes the next quad: thread -> (group = tid % 4 + 4 * (tid / (4 NQ)) + GPP * pass, quad =
    // (tid / 4) % NQ).  The vector memory path then sees 64-byte accesses (with one lane per pixel it handled 64
    // separate 16-byte accesses per load instruction: TA busy 75 % of the kernel on the 32-channel layers), and the
    // LDS stores of a half-wave still fall on 32 distinct bank pairs: (16 g + 2 quad + const) mod 64, g < 4, quad < 8.
    // (ALL lanes on consecutive channel groups collide - 75 % of the LDS cycles were bank conflicts.)
    const int quad = (tid >> 2) % NQ, grp0 = (tid & 3) + 4 * (tid / (4 * NQ));
    int d_off[DQ];       // byte offset of (pixel quad*4, channel group) inside a stage; -1: channels past Cout
    int x_tapoff[XQ];    // byte offset of (tap, ci) relative to a pixel origin
    int x_kh[XQ], x_kw[XQ], x_cq[XQ], d_cq[DQ];
    bool x_ok[XQ];
#pragma unroll
    for (int q = 0; q < DQ; ++q) {
        d_cq[q] = (grp0 + GPP * q) * 4;
        const bool ok = (grp0 + GPP * q) < DG && (co0 + d_cq[q]) < g.Cout;
        d_off[q] = ok ? ((quad * 4) * (int)g.lddy + co0 + d_cq[q]) * ES : -1;
    }
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
        x_cq[q] = (grp0 + GPP * q) * 4;
        const int kc = kc0 + x_cq[q];
        x_ok[q] = (grp0 + GPP * q) < XG && kc < g.Ktot;
        const int kcc = x_ok[q] ? kc : 0;
        const int tap = kcc / g.Cin, ci = kcc - tap * g.Cin;
        x_kh[q] = tap / g.KW;
        x_kw[q] = tap - x_kh[q] * g.KW;
        x_tapoff[q] = ((x_kh[q] * g.W + x_kw[q]) * (int)g.ldx + ci) * ES;
    }

    // ---- pixel decode, 32 lanes, one stage ahead (carries instead of divisions inside the loop)
    int d_img = 0, d_oy = 0, d_ox = 0;
    unsigned d_p = p_lo + tid;
    if (tid < WBK) {
        const unsigned pp = d_p < (unsigned)g.Mtot ? d_p : 0u;
        const unsigned t = pp / (unsigned)g.Wo;
        d_ox = (int)(pp - t * (unsigned)g.Wo);
        const unsigned im = t / (unsigned)g.Ho;
        d_oy = (int)(t - im * (unsigned)g.Ho);
        d_img = (int)(im - img_lo);
    }
    auto decode = [&](int slot) {
        if constexpr (XM) return;   // (1x1 / stride 1: a pixel's mask row is at pixel * ldx)
        if (tid < WBK) {
            const int y0 = d_oy * g.stride - g.pad, x0 = d_ox * g.stride - g.pad;
            int4 info;
            info.x = ((d_img * (int)ipix + y0 * g.W + x0) * (int)g.ldx) * ES;
            info.y = y0;
            info.z = x0;
            info.w = d_p < p_hi ? 1 : 0;
            *reinterpret_cast<int4*>(&Pinfo[slot][tid][0]) = info;
            d_p += WBK;
            d_ox += WBK;
            while (d_ox >= g.Wo) {
                d_ox -= g.Wo;
                if (++d_oy == g.Ho) {
                    d_oy = 0;
                    ++d_img;
                }
            }
        }
    };

    // operand quads on their way to LDS: 4 fp32 values, or (SB) 4 bf16 values as two dwords (integer-typed: see k_conv_gather)
    using OReg = typename std::conditional<SB, u32x2, f32x4>::type;
    OReg rd[DQ][4], rx[XQ][4];
    // XM: word k of a thread -> (pixel tid % WBK of the stage, 32-column group tid / WBK + k * (kThreads / WBK)); past the
    // tile / Cin / the split: zeros
    [[maybe_unused]] unsigned rxw[XW] = {}, pxw[XW] = {};
    [[maybe_unused]] const int xm_pl = tid % WBK;
    [[maybe_unused]] const int xm_word = kc0 / 32 + tid / WBK;
    [[maybe_unused]] bool xm_ok[XW];
#pragma unroll
    for (int k = 0; k < XW; ++k)
        xm_ok[k] = tid / WBK + k * (kThreads / WBK) < BNk / 32 && (xm_word + k * (kThreads / WBK)) * 32 < g.Cin;
    if constexpr (XM)   // the whole mask is one buffer (host-checked: Mtot * ldx * 4 < 2^31)
        rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)(g.Mtot * g.ldx * 4), 0x00020000);
    auto load_tiles = [&](unsigned p0, int slot) {
        const int dstage = (int)(p0 - p_lo) * (int)g.lddy * ES;  // scalar
        auto fetch = [&](__amdgpu_buffer_rsrc_t rs, int voff) -> OReg {
            if constexpr (SB) return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0));
            else return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
        };
        if constexpr (XM) {
            const unsigned p = p0 + (unsigned)xm_pl;
#pragma unroll
            for (int k = 0; k < XW; ++k)
                rxw[k] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(
                    rs_x, (xm_ok[k] && p < p_hi) ? (int)((p * (unsigned)g.ldx + (unsigned)(xm_word + k * (kThreads / WBK))) * 4u) : -1, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int4 info = XM ? int4{0, 0, 0, 0} : *reinterpret_cast<const int4*>(&Pinfo[slot][quad * 4 + e][0]);
#pragma unroll
            for (int q = 0; q < DQ; ++q) {
                const int voff = d_off[q] < 0 ? -1 : d_off[q] + e * (int)g.lddy * ES + dstage;
                rd[q][e] = fetch(rs_d, voff);
            }
#pragma unroll
            for (int q = 0; q < (XM ? 0 : XQ); ++q) {
                const int iy = info.y + x_kh[q], ix = info.z + x_kw[q];
                const bool ok = (info.w != 0) & x_ok[q] & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
                const int voff = ok ? info.x + x_tapoff[q] : -1;
                rx[q][e] = fetch(rs_x, voff);
            }
        }
    };
    // 4 pixels x 4 channels -> per channel the 4 pixels as bf16 hi / lo (8 bytes each), kept in registers
    bf16x4 pd[DQ][4][2], px[XQ][4][2];
    auto convert_quad = [&](const OReg (&v)[4], bf16x4 (&out)[4][2]) {
        if constexpr (SB) {   // v[pixel] holds channels (0, 1) in element 0 and (2, 3) in element 1, as bf16 pairs
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned a0 = v[0][c >> 1], a1 = v[1][c >> 1], a2 = v[2][c >> 1], a3 = v[3][c >> 1];
                u32x2 o;
                if (c & 1) o = u32x2{(a0 >> 16) | (a1 & 0xffff0000u), (a2 >> 16) | (a3 & 0xffff0000u)};
                else o = u32x2{(a0 & 0xffffu) | (a1 << 16), (a2 & 0xffffu) | (a3 << 16)};
                out[c][0] = __builtin_bit_cast(bf16x4, o);
            }
        } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                f32x2 rest = {v[e][c], v[e + 1][c]};
                bf16x2 pp = __builtin_convertvector(rest, bf16x2);
                const unsigned bits = __builtin_bit_cast(unsigned, pp);
                out[c][0][e] = pp[0]; out[c][0][e + 1] = pp[1];
                if constexpr (!ONE) {
                    rest[0] -= __builtin_bit_cast(float, bits << 16);
                    rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
                    pp = __builtin_convertvector(rest, bf16x2);
                    out[c][1][e] = pp[0]; out[c][1][e + 1] = pp[1];
                }
            }
        }
    };
    auto convert_spikes = [&](const OReg (&v)[4], bf16x4 (&out)[4][2]) {   // XSP: 4 pixels of a channel as bf16 {0, 1}
        if constexpr (XSP) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                u32x2 o;
#pragma unroll
                for (int e = 0; e < 4; e += 2)
                    o[e >> 1] = (v[e][c] > g.x_th ? 0x3F80u : 0u) | (v[e + 1][c] > g.x_th ? 0x3F800000u : 0u);
                out[c][0] = __builtin_bit_cast(bf16x4, o);
            }
        }
    };
    auto write_tiles = [&]() {
#pragma unroll
        for (int q = 0; q < DQ; ++q)
            if (grp0 + GPP * q < DG) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    *reinterpret_cast<bf16x4*>(&Dh[(d_cq[q] + c) * LDW + quad * 4]) = pd[q][c][0];
                    if constexpr (!ONE) *reinterpret_cast<bf16x4*>(&Dl[(d_cq[q] + c) * LDW + quad * 4]) = pd[q][c][1];
                }
            }
        if constexpr (XM) {
#pragma unroll
            for (int k = 0; k < XW; ++k) Xw[tid + kThreads * k] = pxw[k];
        }
#pragma unroll
        for (int q = 0; q < (XM ? 0 : XQ); ++q)
            if (grp0 + GPP * q < XG) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    *reinterpret_cast<bf16x4*>(&Xh[(x_cq[q] + c) * LDW + quad * 4]) = px[q][c][0];
                    if constexpr (!ONE && !XSP) *reinterpret_cast<bf16x4*>(&Xl[(x_cq[q] + c) * LDW + quad * 4]) = px[q][c][1];
                }
            }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // ---- DX: the wave's dx tile (ci group dx_cg of the column tile, pixel group dx_pg of the stage), its wt rows as bf16
    // hi / lo A fragments (lane (r, h): ci = kc0 + 32 dx_cg + r, co = 16 c + 8 h .. + 7), and the lane's address in the dy
    // images for the transposing read: lane 4 q + p of 16-lane group G supplies row (co) 16 c + 8 (G >> 1) + 4 s + q,
    // columns (pixels) 32 dx_pg + 16 (G & 1) + 4 p .. + 3 and receives its own pixel's 4 co - the B fragment of lane (r, h).
    constexpr int NCH = BMc / 16;   // 16-wide co chunks (rows past Cout hold zeros)
    [[maybe_unused]] bf16x8 wh[DX ? NCH : 1], wl[DX ? NCH : 1];
    [[maybe_unused]] const int dx_cg = wave % (BNk / 32), dx_pg = wave / (BNk / 32);
    [[maybe_unused]] int dx_tr = 0;
    if constexpr (DX) {
        const int ci = kc0 + dx_cg * 32 + r;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int co = 16 * c + 8 * h;
            f32x4 v[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            if (ci < g.Cin) {
                if (co < g.Cout) v[0] = *reinterpret_cast<const f32x4*>(d.wt + (int64_t)ci * g.Cout + co);
                if (co + 4 < g.Cout) v[1] = *reinterpret_cast<const f32x4*>(d.wt + (int64_t)ci * g.Cout + co + 4);
            }
#pragma unroll
            for (int e = 0; e < 8; e += 2) {   // the split of k_conv_gather's loader (and of snn_weight_presplit)
                f32x2 rest = {v[e >> 2][e & 3], v[e >> 2][(e & 3) + 1]};
                bf16x2 pp = __builtin_convertvector(rest, bf16x2);
                const unsigned bits = __builtin_bit_cast(unsigned, pp);
                wh[c][e] = pp[0]; wh[c][e + 1] = pp[1];
                rest[0] -= __builtin_bit_cast(float, bits << 16);
                rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
                pp = __builtin_convertvector(rest, bf16x2);
                wl[c][e] = pp[0]; wl[c][e + 1] = pp[1];
            }
        }
        const int grp = lane_id >> 4, i16 = lane_id & 15;
        dx_tr = (8 * (grp >> 1) + (i16 >> 2)) * LDW + dx_pg * 32 + 16 * (grp & 1) + 4 * (i16 & 3);
    }

    auto mfma_group = [&](int ks) {
        bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int off = ((wm * TM + i) * 32 + r) * LDW + ks * 16 + 8 * h;
            ah[i] = *reinterpret_cast<const bf16x8*>(&Dh[off]);
            if constexpr (!ONE) al[i] = *reinterpret_cast<const bf16x8*>(&Dl[off]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if constexpr (XM) {   // bit r of the words of pixels 16 ks + 8 h .. + 7: bf16 1.0 (0x3F80) or 0
                const u32x4 w0 = *reinterpret_cast<const u32x4*>(&Xw[(wn * TN + j) * WBK + ks * 16 + 8 * h]);
                const u32x4 w1 = *reinterpret_cast<const u32x4*>(&Xw[(wn * TN + j) * WBK + ks * 16 + 8 * h + 4]);
                u32x4 d;
                d[0] = (((w0[0] >> r) & 1u) | (((w0[1] >> r) & 1u) << 16)) * 0x3F80u;
                d[1] = (((w0[2] >> r) & 1u) | (((w0[3] >> r) & 1u) << 16)) * 0x3F80u;
                d[2] = (((w1[0] >> r) & 1u) | (((w1[1] >> r) & 1u) << 16)) * 0x3F80u;
                d[3] = (((w1[2] >> r) & 1u) | (((w1[3] >> r) & 1u) << 16)) * 0x3F80u;
                bh[j] = __builtin_bit_cast(bf16x8, d);
                continue;
            }
            const int off = ((wn * TN + j) * 32 + r) * LDW + ks * 16 + 8 * h;
            bh[j] = *reinterpret_cast<const bf16x8*>(&Xh[off]);
            if constexpr (!ONE && !XSP) bl[j] = *reinterpret_cast<const bf16x8*>(&Xl[off]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (!ONE) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    if constexpr (!XSP) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                }
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
    };
    constexpr int NM = TM * TN * (ONE ? 1 : (XSP ? 2 : 3));
    constexpr int NREAD = XM ? 2 * TM + 2 * TN : (XSP ? 2 * TM + TN : (TM + TN) * (ONE ? 1 : 2));
    constexpr int CQ_OPS = SB ? 12 : 56;   // VALU per converted quad (approx.)
    constexpr int VPG_D = (DQ * CQ_OPS + NM - 1) / NM, VPG_X = XM ? (TN * 20 + NM - 1) / NM : (XQ * (XSP ? 24 : CQ_OPS) + NM - 1) / NM;

    decode(0);
    __syncthreads();
    load_tiles(p_lo, 0);
    decode(1);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < DQ; ++q) convert_quad(rd[q], pd[q]);
#pragma unroll
    for (int k = 0; k < XW; ++k) pxw[k] = rxw[k];
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
        if constexpr (XM) continue;
        else if constexpr (XSP) convert_spikes(rx[q], px[q]);
        else convert_quad(rx[q], px[q]);
    }
    write_tiles();
    load_tiles(p_lo + WBK, 1);
    decode(0);
    __syncthreads();

    int slot = 0;  // Pinfo slot of tile k+2
#pragma unroll 1
    for (unsigned p0 = p_lo; p0 < p_hi; p0 += WBK) {
        // DX: the addend rows of this stage's dx tile are requested before the stage's MFMAs
        [[maybe_unused]] f32x4 ad1[4], ad2[4];
        [[maybe_unused]] const unsigned dx_p = p0 + (unsigned)(dx_pg * 32 + r);
        [[maybe_unused]] const int dx_ci = kc0 + dx_cg * 32 + 4 * h;   // + 8 jj: the 4 consecutive ci of registers 4 jj .. 4 jj + 3
        if constexpr (DX) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const bool ok = dx_p < p_hi && dx_ci + 8 * jj < g.Cin;
                ad1[jj] = ad2[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (d.add1 && ok) ad1[jj] = SnnStore<false>::ld4_last(d.add1, (int64_t)dx_p * d.ld_add1 + dx_ci + 8 * jj);
                if (d.add2 && ok) ad2[jj] = SnnStore<false>::ld4_last(d.add2, (int64_t)dx_p * d.ld_add2 + dx_ci + 8 * jj);
            }
        }
        mfma_group(0);
#pragma unroll
        for (int q = 0; q < DQ; ++q) convert_quad(rd[q], pd[q]);
        __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, VPG_D, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(1);
#pragma unroll
        for (int k = 0; k < XW; ++k) pxw[k] = rxw[k];   // (XM: the words of tile k + 1 as they were loaded; rxw takes tile k + 2 below)
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            if constexpr (XM) continue;
            else if constexpr (XSP) convert_spikes(rx[q], px[q]);
            else convert_quad(rx[q], px[q]);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, VPG_X, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 2; ks < WBK / 16; ++ks) mfma_group(ks);
        if constexpr (DX) {
            f32x16 dacc;
#pragma unroll
            for (int e = 0; e < 16; ++e) dacc[e] = 0.f;
            typedef __attribute__((address_space(3))) s16x4* LdsQuad;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {   // (uniform control flow: the transposing read needs every lane of the wave)
                const int o = dx_tr + 16 * c * LDW;
                const s16x4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsQuad)&Dh[o]);
                const s16x4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsQuad)&Dh[o + 4 * LDW]);
                const s16x4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsQuad)&Dl[o]);
                const s16x4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsQuad)&Dl[o + 4 * LDW]);
                const bf16x8 dh = __builtin_bit_cast(bf16x8, __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7));
                const bf16x8 dl = __builtin_bit_cast(bf16x8, __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7));
                dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[c], dl, dacc, 0, 0, 0);   // dy_lo * w_hi: small terms first
                dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[c], dh, dacc, 0, 0, 0);   // dy_hi * w_lo
                dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[c], dh, dacc, 0, 0, 0);   // dy_hi * w_hi
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (!(dx_p < p_hi && dx_ci + 8 * jj < g.Cin)) continue;
                f32x4 v = {dacc[4 * jj], dacc[4 * jj + 1], dacc[4 * jj + 2], dacc[4 * jj + 3]};
                if (d.add1) v += ad1[jj];
                if (d.add2) v += ad2[jj];
                SnnStore<false>::st4(d.dx, (int64_t)dx_p * d.lddx + dx_ci + 8 * jj, v);
            }
        }
        load_tiles(p0 + 2 * WBK, slot);
        __syncthreads();
        write_tiles();
        decode(slot ^ 1);
        __syncthreads();
        slot ^= 1;
    }

    float* slab = ws + (int64_t)z * g.Cout * (int64_t)g.Ktot;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int kcol = kc0 + (wn * TN + j) * 32 + r;
            if (kcol >= g.Ktot) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (co < g.Cout) slab[(int64_t)co * g.Ktot + kcol] = acc[i][j][e];
            }
        }
}

// Ordered reduction of the split-K slabs ws[splitk][n] -> dw[n].  KG thread groups share the slabs of one element
// (each sums a contiguous run in slab order), then group 0 adds the KG partial sums in group order: fixed order,
// bitwise reproducible, and the early layers (n of a few hundred, splitk of several hundred) are no longer one
// latency-bound serial chain per thread.
template <int KG>
__global__ void k_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splitk,
                               int accumulate) {
    constexpr int EL = kThreads / KG;
    __shared__ float part[KG][EL];
    const int el = threadIdx.x % EL, kg = threadIdx.x / EL;
    const int64_t e = (int64_t)blockIdx.x * EL + el;
    const int per = (splitk + KG - 1) / KG;
    const int k0 = kg * per;
    const int k1 = k0 + per < splitk ? k0 + per : splitk;
    float s = 0.f;
    if (e < n) {
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const float a = ws[(int64_t)k * n + e], b = ws[(int64_t)(k + 1) * n + e];
            const float c = ws[(int64_t)(k + 2) * n + e], d = ws[(int64_t)(k + 3) * n + e];
            s = (((s + a) + b) + c) + d;
        }
        for (; k < k1; ++k) s += ws[(int64_t)k * n + e];
    }
    if (KG > 1) {
        part[kg][el] = s;
        __syncthreads();
        if (kg == 0) {
            s = part[0][el];
#pragma unroll
            for (int g = 1; g < KG; ++g) s += part[g][el];
        }
    }
    if (kg == 0 && e < n) dw[e] = accumulate ? dw[e] + s : s;
}

// The same ordered reduction, 16 bytes per lane and whole 4 KiB runs per block (the kernel above reads 16 ... 64 bytes
// per slab row and block: 0.8 TB/s on the 2 000-slab workspaces of the narrow layers).  dst[g][e] = sum of rows
// [g * per, (g + 1) * per) of src in row order (+ dst when accumulate); a first pass reduces groups of rows IN PLACE
// (into the first row of each group - every thread only overwrites positions it has read itself), a second pass adds
// the group heads.
__global__ __launch_bounds__(kThreads) void k_wgrad_reduce4(const float* __restrict__ src, int64_t n, int rows, int per,
                                                            int64_t row_stride, float* __restrict__ dst,
                                                            int64_t dst_group_stride, int accumulate) {
    const int64_t e = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (e >= n) return;
    const int g = blockIdx.y;
    const int r0 = g * per;
    const int r1 = r0 + per < rows ? r0 + per : rows;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + (int64_t)r * row_stride + e);
        const f32x4 b = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 1) * row_stride + e);
        const f32x4 c = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 2) * row_stride + e);
        const f32x4 d = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 3) * row_stride + e);
        s = (((s + a) + b) + c) + d;
    }
    for (; r < r1; ++r) s = s + *reinterpret_cast<const f32x4*>(src + (int64_t)r * row_stride + e);
    float* out = dst + (int64_t)g * dst_group_stride + e;
    if (accumulate) s = *reinterpret_cast<const f32x4*>(out) + s;
    *reinterpret_cast<f32x4*>(out) = s;
}

// The ordered reduction in ONE launch (round 4; the two-pass form above cost two latency-bound launches behind every one of
// the ~38 weight gradients of a step): a block owns 256 consecutive elements (64 lanes x 16 bytes = 1 KiB runs per slab
// row), its KG waves each sum a contiguous run of slab rows in row order, then wave 0 adds the KG partial sums in wave
// order: fixed order, bitwise reproducible.
template <int KG>
__global__ __launch_bounds__(64 * KG) void k_wgrad_reduce_once(const float* __restrict__ src, int64_t n, int rows,
                                                              float* __restrict__ dst, int accumulate) {
    __shared__ f32x4 part[KG][64];
    const int lane = threadIdx.x & 63, kg = threadIdx.x >> 6;
    const int64_t e = ((int64_t)blockIdx.x * 64 + lane) * 4;
    const int per = (rows + KG - 1) / KG;
    const int r0 = kg * per;
    const int r1 = r0 + per < rows ? r0 + per : rows;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (e < n) {
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(src + (int64_t)r * n + e);
            const f32x4 b = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 1) * n + e);
            const f32x4 c = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 2) * n + e);
            const f32x4 d = *reinterpret_cast<const f32x4*>(src + (int64_t)(r + 3) * n + e);
            s = (((s + a) + b) + c) + d;
        }
        for (; r < r1; ++r) s = s + *reinterpret_cast<const f32x4*>(src + (int64_t)r * n + e);
    }
    if (KG > 1) {
        part[kg][lane] = s;
        __syncthreads();
        if (kg == 0) {
            s = part[0][lane];
#pragma unroll
            for (int g = 1; g < KG; ++g) s = s + part[g][lane];
        }
    }
    if (kg == 0 && e < n) {
        float* out = dst + e;
        if (accumulate) s = *reinterpret_cast<const f32x4*>(out) + s;
        *reinterpret_cast<f32x4*>(out) = s;
    }
}

struct WgradTile { int bm, bn, id, blocks_per_cu; };
// the kernels' template arguments of tile `id`: 32-row MFMA tiles per wave (tm x tn) and waves of a block (wm x wn)
struct WgradShape { int tm, tn, wm, wn; };
constexpr WgradShape kWgradShapes[6] = {{2, 2, 2, 2}, {2, 2, 1, 4}, {1, 2, 1, 4}, {2, 1, 2, 2}, {1, 1, 2, 2}, {1, 1, 1, 4}};
// candidate block tiles (out-channels x (tap,ci) columns); pick the one that wastes the least MFMA work on
// padding, larger tiles first on ties (fewer LDS / L2 bytes per FLOP)
static WgradTile wgrad_tile(int Cout, int Ktot, bool split, int64_t M) {
    // blocks_per_cu: residency of each variant (registers / LDS), used to size the pixel split to ONE full wave
    static const WgradTile cand[] = {{128, 128, 0, 3}, {64, 256, 1, 3}, {32, 256, 2, 4},
                                     {128, 64, 3, 3},  {64, 64, 4, 3},  {32, 128, 5, 3}};
    if (const char* force = snn_tuning_env("SNN_WGRAD_TILE")) {  // tuning aid
        int id = atoi(force);
        if (id >= 0 && id < 6) return cand[id];
    }
    WgradTile best = cand[0];
    double best_eff = -1.0;
    for (const WgradTile& c : cand) {
        double padded = (double)(snn_ceil_div(Cout, c.bm) * c.bm) * (double)(snn_ceil_div(Ktot, c.bn) * c.bn);
        double eff = (double)Cout * Ktot / padded;
        // with the bf16x3 MFMAs (5x cheaper) the per-stage overhead dominates: favour the 128 x 128 tile (measured;
        // 64 -> 64 3x3 is faster on nine 64 x 64 tiles than on three 64 x 256 ones since the loader is coalesced)
        // On very long pixel ranges (the 304x240 T=128 backbone: 18.7 M pixels) the 64 x 256 tile wins again - x is
        // then re-read from HBM once per column tile, 3 instead of 9 times (6.9 vs 8.5 ms).
        if (split && (c.id == 0 || (c.id == 1 && M > 4000000))) eff *= 1.4;
        if (eff > best_eff + 1e-9) {
            best_eff = eff;
            best = c;
        }
    }
    return best;
}

// ---- the plan of a weight gradient: kernel, block tile, pixel splits and the slab reducer, read by wgrad_common,
// wgrad_reduce_slabs and the host-only queries (snn_conv2d_wgrad_plan, snn_conv2d_wgrad_splitk, snn_conv2d_wgrad_kernel)
constexpr unsigned kAlignDy16 = kAlignOut16, kAlignDy8 = kAlignOut8, kAlignDw16 = kAlignAdd16;   // roles of a weight gradient

// workspace slabs snn_conv2d_wgrad wants on a device with num_cu compute units
static int wgrad_splitk(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                        int precision, int num_cu) {
    const int bwd_split = precision == SNN_PREC_FP32 ? 0 : 1;   // SNN_PREC_BF16S plans like the other 16-bit modes
    if (bwd_split) {  // 3x3 layers with whole 32-channel tiles: the halo-resident kernel (wgrad_halo.hip)
        const SnnWgradHaloPlan hp = snn_wgrad_halo_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, num_cu);
        if (hp.ok) return hp.slabs;
    }
    const int64_t M = N * Ho * (int64_t)Wo;
    const int64_t Ktot = (int64_t)KH * KW * Cin;
    if (snn_first_layer_shape(Cin, Cout, KH, KW)) return snn_first_layer_blocks(N * Ho, num_cu);  // one slab per block
    const bool split_mode = bwd_split && Cin % 4 == 0 && Cout % 4 == 0;
    const WgradTile t = wgrad_tile(Cout, (int)Ktot, split_mode, M);
    const int64_t tiles = snn_ceil_div(Cout, t.bm) * snn_ceil_div(Ktot, t.bn);
    // all blocks resident at once (a second, nearly empty wave of equal-length blocks would double the time);
    // residency of the bf16x3 (pipelined) variants by registers / LDS
    // (tools/wgrad_sweep.py over the layer shapes of TinyYolo GEN1, residency 2..4 per variant)
    static const int split_resident[6] = {3, 2, 2, 3, 3, 3};
    int resident = split_mode ? split_resident[t.id] : t.blocks_per_cu;
    if (split_mode && t.id == 4) resident = KH * KW > 1 ? 4 : 2;
    if (split_mode && t.id == 0) {
        // three blocks per CU only while a split keeps >= 24 stages of 32 pixels; shorter splits are all prologue
        const int64_t s3 = (3 * (int64_t)num_cu) / tiles;
        const int64_t s3r = s3 >= 32 ? s3 / 8 * 8 : (s3 < 1 ? 1 : s3);
        if (M / s3r < 24 * WB_K) resident = 2;
    }
    if (const char* force = snn_tuning_env("SNN_WGRAD_RESIDENT")) resident = atoi(force) > 0 ? atoi(force) : resident;  // tuning aid
    int64_t s = ((int64_t)resident * num_cu) / tiles;
    const int64_t max_by_work = snn_ceil_div(M, 8 * WB_K);            // >= 8 LDS stages per block
    const int64_t max_by_mem = (int64_t)(64 << 20) / (Cout * Ktot);   // workspace <= 256 MiB
    if (s > max_by_work) s = max_by_work;
    if (s > max_by_mem) s = max_by_mem;
    if (s >= 32) s = s / 8 * 8;  // whole groups of 8 splits: one split per XCD at a time (XCD-aware mapping)
    if (s > 32768) s = 32768;
    if (s < 1) s = 1;
    return (int)s;
}

// dw (+)= sum over the splitk workspace slabs, fixed order: which kernel walks which rows.  Rows [j * per, (j + 1) * per)
// clipped to splitk belong to group j < groups (none of them empty); kg >= groups thread groups are launched (the ones
// past `groups` add zeros).
enum ReduceKind { kReduceScalar = 0, kReduceOnce = 1, kReduce4TwoPass = 2, kReduce4OnePass = 3 };
struct ReducePlan {
    int kind;
    int kg;          // thread groups sharing the rows of an element (k_wgrad_reduce<KG>, k_wgrad_reduce_once<KG>); reduce4: 1
    int groups, per; // non-empty row groups and rows per group (the last one may be shorter)
    int64_t blocks;  // blocks of the (first) launch along x
};
static ReducePlan wgrad_reduce_plan(int64_t n, int splitk, bool aligned, int num_cu) {
    ReducePlan r = {};
    const bool vec = n % 4 == 0 && aligned;   // 16 bytes per lane: workspace and dw 16-byte aligned
    if (vec && splitk > 1) {
        // one launch when the rows a wave has to walk stay short: blocks of 256 elements, KG waves sharing the slab rows
        const int64_t nb1 = snn_ceil_div(n, 256);
        int kg = 1;
        while (kg < 16 && nb1 * kg < 8 * (int64_t)num_cu && splitk / (2 * kg) >= 4) kg *= 2;
        if (snn_ceil_div(splitk, kg) <= 48) {
            r.kind = kReduceOnce;
            r.kg = kg;
            r.per = (int)snn_ceil_div(splitk, kg);
            r.groups = (int)snn_ceil_div(splitk, r.per);
            r.blocks = nb1;
            return r;
        }
    }
    if (vec && splitk > 8) {
        const int64_t nb = snn_ceil_div(n / 4, kThreads);
        int64_t groups = snn_ceil_div(4 * num_cu, nb);   // ~4 blocks per CU in the first pass
        if (groups > splitk / 4) groups = splitk / 4;          // at least 4 rows per group
        if (groups < 1) groups = 1;
        const int per = (int)snn_ceil_div(splitk, groups);
        groups = snn_ceil_div(splitk, per);
        r.kind = groups > 1 ? kReduce4TwoPass : kReduce4OnePass;
        r.kg = 1;
        r.groups = (int)groups;
        r.per = groups > 1 ? per : splitk;
        r.blocks = nb;
        return r;
    }
    r.kind = kReduceScalar;
    r.kg = splitk <= 8 ? 1 : (splitk <= 64 ? 4 : (splitk <= 256 ? 16 : 64));
    r.per = (int)snn_ceil_div(splitk, r.kg);
    r.groups = (int)snn_ceil_div(splitk, r.per);
    r.blocks = snn_ceil_div(n, kThreads / r.kg);
    return r;
}

}  // namespace

static int wgrad_reduce_slabs(float* workspace, float* dw, int64_t n, int splitk, int accumulate, hipStream_t st) {
    const ReducePlan r = wgrad_reduce_plan(n, splitk, aligned(16, {workspace, dw}), snn_num_cu());
    // (the plan gives no other kg than the instances listed: it doubles from 1 up to 16, or is one of four literals)
    if (r.kind == kReduceOnce) {
        const bool launched = dispatch(
            [&](auto KG) {
                hipLaunchKernelGGL((k_wgrad_reduce_once<KG()>), dim3((unsigned)r.blocks), dim3(64 * KG()), 0, st, workspace, n,
                                   splitk, dw, accumulate);
                return true;
            },
            OneOf<1, 2, 4, 8, 16>{r.kg});
        SNN_REQUIRE(launched, "snn_conv2d_wgrad_reduce: no kernel for %d thread groups", r.kg);
        SNN_CHECK_LAUNCH("snn_conv2d_wgrad_reduce");
        return 0;
    }
    if (r.kind == kReduce4TwoPass) {
        hipLaunchKernelGGL(k_wgrad_reduce4, dim3((unsigned)r.blocks, (unsigned)r.groups), dim3(kThreads), 0, st, workspace,
                           n, splitk, r.per, n, workspace, (int64_t)r.per * n, 0);
        hipLaunchKernelGGL(k_wgrad_reduce4, dim3((unsigned)r.blocks, 1), dim3(kThreads), 0, st, workspace, n,
                           r.groups, r.groups, (int64_t)r.per * n, dw, 0, accumulate);
        SNN_CHECK_LAUNCH("snn_conv2d_wgrad_reduce");
        return 0;
    }
    if (r.kind == kReduce4OnePass) {
        hipLaunchKernelGGL(k_wgrad_reduce4, dim3((unsigned)r.blocks, 1), dim3(kThreads), 0, st, workspace, n, splitk,
                           splitk, n, dw, 0, accumulate);
        SNN_CHECK_LAUNCH("snn_conv2d_wgrad_reduce");
        return 0;
    }
    const bool launched = dispatch(
        [&](auto KG) {
            hipLaunchKernelGGL((k_wgrad_reduce<KG()>), dim3((unsigned)r.blocks), dim3(kThreads), 0, st, workspace, dw, n, splitk,
                               accumulate);
            return true;
        },
        OneOf<1, 4, 16, 64>{r.kg});
    SNN_REQUIRE(launched, "snn_conv2d_wgrad_reduce: no kernel for %d thread groups", r.kg);
    SNN_CHECK_LAUNCH("snn_conv2d_wgrad_reduce");
    return 0;
}

namespace {
// the weight-gradient plan of k_conv_first, ok = 0 when the shape or the buffers are not covered
static FirstPlan first_layer_wgrad_plan(unsigned align, int64_t ldx, int64_t lddy, int64_t N, int H, int W, int Cin, int Ho,
                                        int Wo, int Cout, int KH, int KW, int stride, int pad, bool dy_bf16, int num_cu) {
    if (Cin != 2 || KH != 3 || KW != 3) return FirstPlan{};
    FirstPlan p = snn_first_layer_plan(N, H, W, Ho, Wo, Cout, stride, pad, 0, true, num_cu);
    if (!(ldx % 2 == 0 && (align & kAlignIn8) && lddy % 4 == 0 && (align & (dy_bf16 ? kAlignDy8 : kAlignDy16)) &&
          (int64_t)W * ldx < 0x7fffffffLL))
        p.ok = 0;
    return p;
}
static unsigned wgrad_align_bits(const void* x, const void* dy) {
    return (aligned(16, {x}) ? kAlignIn16 : 0u) | (aligned(8, {x}) ? kAlignIn8 : 0u) | (aligned(16, {dy}) ? kAlignDy16 : 0u) |
           (aligned(8, {dy}) ? kAlignDy8 : 0u);
}
static FirstPlan first_layer_wgrad_plan(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t N, int H, int W,
                                        int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad) {
    return first_layer_wgrad_plan(wgrad_align_bits(x, dy), ldx, lddy, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, false, 0);
}

// The plan of snn_conv2d_wgrad / snn_conv2d_spikes_wgrad (xsp) for valid arguments.  splitk > 0: the caller's slab count
// (the halo-resident kernel insists on its own); 0: the count snn_conv2d_wgrad_splitk gives for num_cu compute units.
// halo = false: the halo-resident kernel could not address the buffers, plan the implicit GEMM with the same slabs.
enum WgradKernel { kWgradPipe = 0, kWgradVec = 1, kWgradScalar = 2, kWgradHalo = 3, kWgradFirst = 4 };
enum WgradRefusal { kWgradOk = 0, kWgradHaloSplitk, kWgradNotPipeSB, kWgradNotPipeXSP, kWgradGridTooLarge };
struct WgradPlan {
    int ok, why;
    int kernel;                   // WgradKernel
    WgradTile t;                  // implicit GEMM: block tile (out-channels x (tap, ci) columns)
    int tiles_m, tiles_n, wbk;    // ... tiles over Cout and over Ktot, pixels per LDS stage (32 / 64)
    int splitk;
    int64_t pix_per_split;        // ... a whole number of stages; split z owns pixels [z, z + 1) * pix_per_split below M
    int64_t last_pix;             // ... pixels of the last split that owns any
    int empty_splits;             // ... splits past it: they write a zero slab
    bool one;                     // one bf16 product (bf16 x 1, bf16 storage)
    FirstPlan fp;
    SnnWgradHaloPlan hp;
    ReducePlan r;
};
static WgradPlan wgrad_plan(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                            int64_t ldx, int64_t lddy, unsigned align, int precision, bool xsp, int num_cu, int splitk,
                            bool halo = true, bool xm = false) {
    // xm (with xsp, 1x1 / stride 1): x is a spike bit mask of ldx uint32 words per pixel; kAlignIn16 stands for its 4-byte
    // alignment
    WgradPlan p = {};
    if (num_cu <= 0) num_cu = snn_num_cu();
    const int bwd_split = precision;
    const bool sbf = precision == SNN_PREC_BF16S;   // x (but for the fp32 event frames) and dy are bf16
    const int64_t M = N * Ho * (int64_t)Wo;
    const int Ktot = KH * KW * Cin;
    const int64_t n = (int64_t)Cout * Ktot;
    p.splitk = splitk > 0 ? splitk : wgrad_splitk(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, precision, num_cu);
    p.r = wgrad_reduce_plan(n, p.splitk, (align & kAlignDw16) != 0, num_cu);
    p.fp = xsp ? FirstPlan{}
               : first_layer_wgrad_plan(align, ldx, lddy, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, sbf, num_cu);
    if (p.fp.ok) {
        p.kernel = kWgradFirst;
        p.ok = 1;
        return p;
    }
    if (bwd_split && halo) {
        p.hp = snn_wgrad_halo_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, num_cu);
        if (p.hp.ok) {
            p.kernel = kWgradHalo;
            p.ok = p.splitk == p.hp.slabs;
            p.why = p.ok ? kWgradOk : kWgradHaloSplitk;
            return p;
        }
    }
    const bool vec = (Cin % 4 == 0) && (Cout % 4 == 0) && (xm || ldx % 4 == 0) && (lddy % 4 == 0) &&
                     (sbf ? (align & kAlignIn8) && (align & kAlignDy8) : (align & kAlignIn16) && (align & kAlignDy16));
    p.t = wgrad_tile(Cout, Ktot, bwd_split && Cin % 4 == 0 && Cout % 4 == 0, M);
    // small tiles (64 x 64, 32 x 128) run 64-pixel stages in the pipelined kernel (latency cover), the others 32
    static const int wbk_small = snn_tuning_env("SNN_WGRAD_WBK") ? atoi(snn_tuning_env("SNN_WGRAD_WBK")) : 64;  // tuning aid
    p.wbk = (p.t.id >= 4 && wbk_small == 64) ? 64 : 32;
    p.pix_per_split = snn_ceil_div(snn_ceil_div(M, p.splitk), p.wbk) * p.wbk;
    // pipelined kernel: 32-bit byte offsets relative to the first image of a pixel split
    const int64_t span_pix = p.pix_per_split * (int64_t)stride * stride + 3 * (int64_t)H * W;
    static const bool no_pipe = snn_tuning_env("SNN_WGRAD_NO_PIPE") != nullptr;  // tuning / bisecting aid
    const bool pipe = vec && bwd_split && !no_pipe && M < 0x7fffffffLL && span_pix * ldx * 4 < 0x7fffffffLL &&
                      p.pix_per_split * lddy * 4 < 0x7fffffffLL && (int64_t)H * W * ldx * 4 < 0x7fffffffLL &&
                      (!xm || (Cin % 32 == 0 && ldx * 32 >= Cin && M * ldx * 4 < 0x7fffffffLL));
    p.one = precision == SNN_PREC_BF16X1 || sbf;
    p.kernel = pipe ? kWgradPipe : (vec ? kWgradVec : kWgradScalar);
    if (sbf && !pipe) {
        p.why = kWgradNotPipeSB;
        return p;
    }
    if (xsp && !(pipe && !p.one)) {
        p.why = kWgradNotPipeXSP;
        return p;
    }
    p.tiles_m = (int)snn_ceil_div(Cout, p.t.bm);
    p.tiles_n = (int)snn_ceil_div(Ktot, p.t.bn);
    if ((int64_t)p.tiles_m * p.tiles_n * p.splitk > 0x7fffffff) {
        p.why = kWgradGridTooLarge;
        return p;
    }
    const int64_t owners = snn_ceil_div(M, p.pix_per_split);   // splits that own a pixel
    p.last_pix = M - (owners - 1) * p.pix_per_split;
    p.empty_splits = (int)(p.splitk - owners);
    p.ok = 1;
    return p;
}
}  // namespace

// xsp: x holds saved LIF potentials, the operand is z = (x > x_th) (snn_conv1x1_spikes_wgrad; pipelined bf16 x 3 kernel only)
static int wgrad_common(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, int64_t N,
                        int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                        int accumulate, float* workspace, int splitk, int precision, void* stream, bool xsp, float x_th,
                        bool xm = false) {
    SNN_REQUIRE(x && dy && dw && workspace, "snn_conv2d_wgrad: null pointer");
    SNN_REQUIRE(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X3 || precision == SNN_PREC_BF16X1 ||
                    precision == SNN_PREC_BF16S,
                "snn_conv2d_wgrad: precision must be SNN_PREC_FP32, _BF16X3, _BF16X1 or _BF16S (got %d)", precision);
    const bool sbf = precision == SNN_PREC_BF16S;   // x (but for the fp32 event frames) and dy are bf16
    if (check_conv_shape("snn_conv2d_wgrad", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    SNN_REQUIRE((xm || ldx >= Cin) && lddy >= Cout, "snn_conv2d_wgrad: pixel stride smaller than channel count");
    SNN_REQUIRE(splitk >= 1 && splitk <= 32768, "snn_conv2d_wgrad: bad splitk %d", splitk);
    SNN_REQUIRE(N * (int64_t)H * W < 0x7fffffffLL, "snn_conv2d_wgrad: more than 2^31 input pixels");
    WgradGeom g;
    g.Mtot = N * Ho * (int64_t)Wo;
    g.H = H; g.W = W; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.Cout = Cout;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.ldx = ldx; g.lddy = lddy;
    g.Ktot = KH * KW * Cin;
    g.x_th = x_th;
    // (the reducer plan in p.r is the one wgrad_reduce_slabs derives again from the same two pointers)
    unsigned align = wgrad_align_bits(x, dy) | (aligned(16, {dw, workspace}) ? kAlignDw16 : 0u);
    if (xm) align = (align & ~(kAlignIn16 | kAlignIn8)) | (aligned(4, {x}) ? kAlignIn16 : 0u);
    WgradPlan p = wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldx, lddy, align, precision, xsp, 0, splitk, !xm, xm);
    if (p.kernel == kWgradFirst) {
        const FirstPlan& fp = p.fp;
        FirstGeom fg = {ldx, lddy, (int)(N * Ho), H, W, Ho, Wo, Cout, stride, pad, fp.group_rows, splitk, nullptr,
                        nullptr, 0, nullptr, 0, 1, fp.rs};
        if (const int rc = snn_launch_first(true, false, sbf, splitk, fp.lds, x, nullptr, dy, workspace, fg, stream, "snn_conv2d_wgrad"))
            return rc;
        return wgrad_reduce_slabs(workspace, dw, (int64_t)Cout * g.Ktot, splitk, accumulate, (hipStream_t)stream);
    }
    if (p.kernel == kWgradHalo) {
        const SnnWgradHaloPlan& hp = p.hp;
        SNN_REQUIRE(p.why != kWgradHaloSplitk, "snn_conv2d_wgrad: splitk %d, expected %d (snn_conv2d_wgrad_splitk)", splitk,
                    hp.slabs);
        const int rc = snn_wgrad_halo_launch(hp, x, ldx, dy, lddy, workspace, N, H, W, Cin, Ho, Wo, Cout, stride,
                                             xsp ? 2 : ((precision == SNN_PREC_BF16X1 || sbf) ? 1 : 3), sbf,
                                             (hipStream_t)stream, x_th);
        if (rc == 0)
            return wgrad_reduce_slabs(workspace, dw, (int64_t)Cout * g.Ktot, hp.slabs, accumulate, (hipStream_t)stream);
        if (rc > 0) return rc;
        // rc < 0: buffers this kernel cannot address (unaligned / > 2 GiB per image): the implicit-GEMM kernel
        p = wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldx, lddy, align, precision, xsp, 0, splitk, false);
    }
    SNN_REQUIRE(p.why != kWgradNotPipeSB, "snn_conv2d_wgrad: bf16 storage covers the event-frame layer and the pipelined kernels only "
                "(channels and strides multiples of 4, 8-byte aligned tensors, < 2 GiB per pixel split)");
    SNN_REQUIRE(p.why != kWgradNotPipeXSP, "snn_conv1x1_spikes_wgrad: covers the pipelined bf16 x 3 kernel only (channels and "
                "strides multiples of 4, 16-byte aligned tensors, < 2 GiB per pixel split)");
    SNN_REQUIRE(p.why != kWgradGridTooLarge, "snn_conv2d_wgrad: grid too large");
    g.pix_per_split = p.pix_per_split;
    g.nimg = (int)N;
    g.tiles_m = p.tiles_m;
    g.tiles_n = p.tiles_n;
    g.splitk = splitk;
    dim3 grid((unsigned)((int64_t)g.tiles_m * g.tiles_n * splitk));
    hipStream_t st = (hipStream_t)stream;
    dispatch(
        [&](auto ID, auto KERNEL, auto WBK, auto ONE, auto SB, auto XSP, auto XM) {
            constexpr WgradShape t = kWgradShapes[ID()];
            if constexpr (KERNEL() != kWgradPipe) {
                hipLaunchKernelGGL((k_conv_wgrad<t.tm, t.tn, t.wm, t.wn, KERNEL() == kWgradVec>), grid, dim3(kThreads), 0, st, x, dy,
                                   workspace, g);
            } else if constexpr ((!SB() || ONE()) && (!XSP() || (!ONE() && !SB())) && (!XM() || XSP())) {   // bf16 storage: one product; spikes: three
                hipLaunchKernelGGL((k_conv_wgrad_pipe<t.tm, t.tn, t.wm, t.wn, WBK(), ONE(), SB(), XSP(), XM()>), grid, dim3(kThreads), 0,
                                   st, x, dy, workspace, g, WgradDx{});
            }
            return true;
        },
        OneOf<0, 1, 2, 3, 4, 5>{p.t.id}, OneOf<0, 1, 2>{p.kernel}, OneOf<32, 64>{p.wbk}, Flag{p.one}, Flag{sbf}, Flag{xsp}, Flag{xm});
    SNN_CHECK_LAUNCH("snn_conv2d_wgrad");
    return wgrad_reduce_slabs(workspace, dw, (int64_t)Cout * g.Ktot, splitk, accumulate, st);
}

extern "C" int snn_conv2d_wgrad_splitk(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                                       int stride, int pad, int precision) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0) return 1;
    return wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Cin, Cout, kAlignAll, precision, false, 0, 0).splitk;
}

// which kernel snn_conv2d_wgrad launches for a shape: 0 the implicit GEMM (k_conv_wgrad_pipe / k_conv_wgrad), 1 the
// halo-resident kernel (k_conv_wgrad_halo), 2 the event-frame row kernel (k_conv_first) - for measurement labels; host-only
extern "C" int snn_conv2d_wgrad_kernel(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                       int pad, int precision) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0) return 0;
    if (snn_first_layer_shape(Cin, Cout, KH, KW)) return 2;
    const int k = wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, Cin, Cout, kAlignAll, precision, false, 0, 0).kernel;
    return k == kWgradHalo ? 1 : (k == kWgradFirst ? 2 : 0);
}

extern "C" int snn_conv2d_wgrad_bn_supported(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                                             int stride, int pad) {
    // the event-frame layer's row kernel (pointer alignment is checked by the call itself)
    if (Cin != 2 || KH != 3 || KW != 3) return 0;
    return snn_first_layer_plan(N, H, W, Ho, Wo, Cout, stride, pad, 0, true, 0).ok;
}

extern "C" int snn_conv2d_wgrad_bn(const float* x, int64_t ldx, const float* gx, int64_t ldgx, const float* y, int64_t ldy,
                                   const float* coef, int T, int frames_per_step, float* dw, int64_t N, int H, int W,
                                   int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int accumulate,
                                   float* workspace, int splitk, void* stream) {
    SNN_REQUIRE(x && gx && y && coef && dw && workspace, "snn_conv2d_wgrad_bn: null pointer");
    if (check_conv_shape("snn_conv2d_wgrad_bn", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    SNN_REQUIRE(frames_per_step > 0 && T > 0 && (int64_t)T * frames_per_step == N,
                "snn_conv2d_wgrad_bn: %lld frames are not %d timesteps of %d", (long long)N, T, frames_per_step);
    SNN_REQUIRE(ldx >= Cin && ldgx >= Cout && ldy >= Cout, "snn_conv2d_wgrad_bn: pixel stride smaller than channel count");
    SNN_REQUIRE(splitk >= 1 && splitk <= 32768, "snn_conv2d_wgrad_bn: bad splitk %d", splitk);
    const FirstPlan fp = first_layer_wgrad_plan(x, ldx, gx, ldgx, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad);
    SNN_REQUIRE(fp.ok && ldy % 4 == 0 && aligned(16, {y, coef}) && (int64_t)Wo * ldy < 0x7fffffffLL &&
                    (int64_t)Wo * ldgx < 0x7fffffffLL,
                "snn_conv2d_wgrad_bn: shape / alignment not covered (ask snn_conv2d_wgrad_bn_supported)");
    FirstGeom fg = {ldx, ldgx, (int)(N * Ho), H, W, Ho, Wo, Cout, stride, pad, fp.group_rows, splitk, nullptr,
                    y, ldy, coef, T * Cout, frames_per_step, fp.rs};
    if (const int rc = snn_launch_first(true, true, false, splitk, fp.lds, x, nullptr, gx, workspace, fg, stream, "snn_conv2d_wgrad_bn"))
        return rc;
    return wgrad_reduce_slabs(workspace, dw, (int64_t)Cout * KH * KW * Cin, splitk, accumulate, (hipStream_t)stream);
}

extern "C" int snn_conv2d_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, int64_t N,
                                int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                                int accumulate, float* workspace, int splitk, int precision, void* stream) {
    return wgrad_common(x, ldx, dy, lddy, dw, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, accumulate, workspace, splitk,
                        precision, stream, false, 0.0f);
}

// Host-only: the plan of snn_conv2d_wgrad (spikes = 1: snn_conv2d_spikes_wgrad) on a device with num_cu compute units; see
// include/snn_hip.h.  It reads the plan function the launch and the slab reducer read.
extern "C" int snn_conv2d_wgrad_plan(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                     int pad, int64_t ldx, int64_t lddy, int align_bits, int precision, int spikes, int num_cu,
                                     int* out) {
    if (!out) return 1;
    for (int i = 0; i < 18; ++i) out[i] = 0;
    if (check_conv_shape("snn_conv2d_wgrad_plan", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    if (!(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X3 || precision == SNN_PREC_BF16X1 ||
          precision == SNN_PREC_BF16S) || ldx < Cin || lddy < Cout || !(N * (int64_t)H * W < 0x7fffffffLL))
        return 1;
    if (spikes && (precision != SNN_PREC_BF16X3 || !spikes_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldx)))
        return 1;
    const WgradPlan p = wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldx, lddy, (unsigned)align_bits, precision,
                                   spikes != 0, num_cu, 0);
    if (!p.ok) return 1;
    const bool gemm = p.kernel <= kWgradScalar;
    const int v[18] = {1, p.kernel, gemm ? p.t.id : 0, gemm ? p.t.bm : 0, gemm ? p.t.bn : 0, p.tiles_m, p.tiles_n, gemm ? p.wbk : 0,
                       p.splitk, (int)p.pix_per_split, (int)p.last_pix, p.empty_splits, p.r.kind, p.r.kg, p.r.groups, p.r.per,
                       (int)p.r.blocks, gemm ? (int)((int64_t)p.tiles_m * p.tiles_n * p.splitk) : 0};
    for (int i = 0; i < 18; ++i) out[i] = v[i];
    return 0;
}

// ---- the weight gradient over spikes that were never stored (see k_conv_wgrad_pipe XSP, include/snn_hip.h)
extern "C" int snn_conv2d_spikes_wgrad(const float* vdec, int64_t ld, float v_th, const float* dy, int64_t lddy, float* dw,
                                       int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                       int pad, int accumulate, float* workspace, int splitk, void* stream) {
    SNN_REQUIRE(v_th >= 0.0f, "snn_conv2d_spikes_wgrad: a negative threshold would turn padding into spikes");
    SNN_REQUIRE(spikes_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld),
                "snn_conv2d_spikes_wgrad: shape not covered (ask snn_conv2d_spikes_supported)");
    return wgrad_common(vdec, ld, dy, lddy, dw, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, accumulate, workspace, splitk,
                        SNN_PREC_BF16X3, stream, true, v_th);
}

extern "C" int snn_conv1x1_spikes_wgrad(const float* vdec, int64_t ld, float v_th, const float* dy, int64_t lddy, float* dw,
                                        int64_t N, int H, int W, int Cin, int Cout, int accumulate, float* workspace,
                                        int splitk, void* stream) {
    return snn_conv2d_spikes_wgrad(vdec, ld, v_th, dy, lddy, dw, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, accumulate, workspace,
                                   splitk, stream);
}

// ---- the 1x1 weight gradient over the spike bit mask of a scan with SNN_SCAN_SPIKE_MASK (see k_conv_wgrad_pipe XM)
bool snn_wgrad_mask_ok(int64_t N, int H, int W, int Cin, int Cout, const uint32_t* mask, int64_t ld_mask, const float* dy,
                       int64_t lddy, const float* dw) {
    if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && mask && dy && dw && Cin % 32 == 0 && Cout % 4 == 0 &&
          ld_mask >= Cin / 32 && lddy >= Cout && lddy % 4 == 0 && aligned(4, {mask, dw}) && aligned(16, {dy}) &&
          (int64_t)Cin * Cout < (1LL << 26)))
        return false;
    // whatever slab count the caller brings, a pixel split is at most the 64-rounded pixel count
    const int64_t M = N * H * (int64_t)W;
    if (!(M < 0x7fffffffLL - 64 && (M + 64 + 3 * (int64_t)H * W) * ld_mask * 4 < 0x7fffffffLL && (M + 64) * lddy * 4 < 0x7fffffffLL))
        return false;
    const unsigned align = kAlignIn16 | kAlignDy16 | kAlignDy8 | (aligned(16, {dw}) ? kAlignDw16 : 0u);
    const WgradPlan p = wgrad_plan(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, ld_mask, lddy, align, SNN_PREC_BF16X3, true, 0, 0, false, true);
    return p.ok && p.kernel == kWgradPipe;
}

extern "C" int snn_conv1x1_mask_wgrad(const uint32_t* mask, int64_t ld_mask, const float* dy, int64_t lddy, float* dw, int64_t N,
                                      int H, int W, int Cin, int Cout, int accumulate, float* workspace, int splitk,
                                      void* stream) {
    SNN_REQUIRE(mask && dy && dw && workspace, "snn_conv1x1_mask_wgrad: null pointer");
    SNN_REQUIRE(snn_wgrad_mask_ok(N, H, W, Cin, Cout, mask, ld_mask, dy, lddy, dw),
                "snn_conv1x1_mask_wgrad: call not covered (ask snn_conv1x1_mask_supported)");
    return wgrad_common(reinterpret_cast<const float*>(mask), ld_mask, dy, lddy, dw, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0,
                        accumulate, workspace, splitk, SNN_PREC_BF16X3, stream, true, 0.0f, true);
}

// ---- both gradients of a 1x1 / stride 1 convolution from ONE pass over dy (see k_conv_wgrad_pipe DX, include/snn_hip.h)
namespace {
struct Bwd1x1Call {
    const void* x;   // fp32 activations, or (xm) the spike bit mask
    int64_t ldx;
    bool xm;
    const float* dy;
    int64_t lddy;
    const float* wt;
    const float* dx;
    int64_t lddx;
    const float *add1, *add2;
    int64_t ld_add1, ld_add2;
    const float* dw;   // may be null (query: unchecked; launch: the slabs stay in the workspace)
};
// nullptr: snn_conv1x1_bwd / snn_conv1x1_mask_bwd take the call (plan in *out); else why not.  The ONE place both the query
// and the launches ask.  splitk 0: the count of snn_conv2d_wgrad_splitk.
static const char* bwd1x1_refusal(int64_t N, int H, int W, int Cin, int Cout, const Bwd1x1Call& c, int splitk, int precision,
                                  WgradPlan* out) {
    if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0)) return "bad shape";
    if (!(c.x && c.dy && c.wt && c.dx)) return "null pointer";
    if (precision != SNN_PREC_BF16X3) return "bf16 x 3 arithmetic on fp32 tensors only";
    if (Cout > 128) return "more than 128 output channels (a block must own all of them)";
    if (Cout % 4 || Cin % 4) return "channel counts must be multiples of 4";
    if (splitk < 0 || splitk > 32768) return "bad splitk";
    if (c.xm ? !(Cin % 32 == 0 && c.ldx >= Cin / 32) : !(c.ldx >= Cin && c.ldx % 4 == 0))
        return "x: pixel stride smaller than the channel count or no multiple of 4 (mask: Cin % 32, ld >= Cin / 32)";
    if (!(c.lddy >= Cout && c.lddy % 4 == 0 && c.lddx >= Cin && c.lddx % 4 == 0))
        return "dy / dx: pixel stride smaller than the channel count or no multiple of 4";
    if (!(aligned(c.xm ? 4 : 16, {c.x}) && aligned(16, {c.dy, c.wt, c.dx}))) return "x, dy, wt and dx must be 16-byte aligned (mask: 4)";
    if (c.add1 && !(c.ld_add1 >= Cin && c.ld_add1 % 4 == 0 && aligned(16, {c.add1}))) return "addend: stride or alignment";
    if (c.add2 && !(c.ld_add2 >= Cin && c.ld_add2 % 4 == 0 && aligned(16, {c.add2}))) return "addend2: stride or alignment";
    if (c.dw && !aligned(4, {c.dw})) return "dw must be 4-byte aligned";
    // (the 2 GiB spans of k_conv_wgrad_pipe - dy and x of one pixel split, the whole mask - are wgrad_plan's to check, with
    // this call's slab count; dx and the addends are addressed with 64 bits)
    if (!(N * H * (int64_t)W < 0x7fffffffLL - 64)) return "more than 2^31 pixels";
    const unsigned align = kAlignIn16 | kAlignDy16 | kAlignDy8 | ((c.dw && aligned(16, {c.dw})) ? kAlignDw16 : 0u);
    const WgradPlan p = wgrad_plan(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, c.ldx, c.lddy, align, precision, c.xm, 0, splitk, false, c.xm);
    if (!(p.ok && p.kernel == kWgradPipe && !p.one)) return "the weight gradient does not take the pipelined bf16 x 3 kernel";
    if (p.tiles_m != 1) return "the weight-gradient tile does not own all output channels";
    if (!(p.t.id == 0 || p.t.id == 4)) return "no fused instance for this weight-gradient tile";
    if (out) *out = p;
    return nullptr;
}

// Layer classes whose fused launch measured slower than the two launches it replaces are not offered by the query (the
// launch still takes them: the kernels are tested on every tile they have an instance for).
static bool bwd1x1_pays(const WgradPlan& p, bool xm) {
    // the 128 x 128 tile on fp32 x (the C2f exit 320 -> 128 at 60 x 76): its instance runs one wave per SIMD against a
    // split count planned for three blocks per CU - 888 us fused against 405 + 305 us in two launches
    return !(p.t.id == 0 && !xm);
}

static int bwd1x1_common(const char* name, const Bwd1x1Call& c, float* dx, float* dw, int64_t N, int H, int W, int Cin, int Cout,
                         int accumulate, float* workspace, int splitk, int precision, void* stream) {
    SNN_REQUIRE(workspace, "%s: null workspace", name);
    SNN_REQUIRE(splitk >= 1, "%s: bad splitk %d", name, splitk);
    WgradPlan p;
    const char* why = bwd1x1_refusal(N, H, W, Cin, Cout, c, splitk, precision, &p);
    SNN_REQUIRE(!why, "%s: call not covered: %s (ask snn_conv1x1_bwd_supported)", name, why);
    WgradGeom g;
    g.Mtot = N * H * (int64_t)W;
    g.H = H; g.W = W; g.Cin = Cin; g.Ho = H; g.Wo = W; g.Cout = Cout;
    g.KH = 1; g.KW = 1; g.stride = 1; g.pad = 0;
    g.ldx = c.ldx; g.lddy = c.lddy;
    g.Ktot = Cin;
    g.x_th = 0.0f;
    g.pix_per_split = p.pix_per_split;
    g.nimg = (int)N;
    g.tiles_m = p.tiles_m;
    g.tiles_n = p.tiles_n;
    g.splitk = splitk;
    const WgradDx d = {c.wt, dx, c.add1, c.add2, c.lddx, c.ld_add1, c.ld_add2};
    const dim3 grid((unsigned)((int64_t)g.tiles_m * g.tiles_n * splitk));
    hipStream_t st = (hipStream_t)stream;
    const float* xf = static_cast<const float*>(c.x);
    dispatch(
        [&](auto ID, auto XM) {
            constexpr WgradShape t = kWgradShapes[ID()];
            constexpr int wbk = ID() >= 4 ? 64 : 32;
            hipLaunchKernelGGL((k_conv_wgrad_pipe<t.tm, t.tn, t.wm, t.wn, wbk, false, false, XM(), XM(), true>), grid, dim3(kThreads), 0, st,
                               xf, c.dy, workspace, g, d);
            return true;
        },
        OneOf<0, 4>{p.t.id}, Flag{c.xm});
    SNN_CHECK_LAUNCH(name);
    if (!dw) return 0;   // the slabs stay in the workspace: snn_conv2d_wgrad_reduce sums them (on any stream)
    return wgrad_reduce_slabs(workspace, dw, (int64_t)Cout * Cin, splitk, accumulate, st);
}
}  // namespace

extern "C" int snn_conv1x1_bwd_supported(int64_t N, int H, int W, int Cin, int Cout, const void* x, int64_t ldx, int is_mask,
                                         const float* dy, int64_t lddy, const float* wt, const float* dx, int64_t lddx,
                                         const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2,
                                         const float* dw, int splitk, int precision) {
    const Bwd1x1Call c = {x, ldx, is_mask != 0, dy, lddy, wt, dx, lddx, addend, addend2, ld_addend, ld_addend2, dw};
    WgradPlan p;
    if (bwd1x1_refusal(N, H, W, Cin, Cout, c, splitk, precision, &p)) return 0;
    // the launch would run; whether it PAYS is a matter of the layer class ("1x1 backward in one pass")
    return bwd1x1_pays(p, c.xm) ? 1 : 0;
}

extern "C" int snn_conv1x1_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* wt, float* dx, int64_t lddx,
                               const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2, float* dw,
                               int64_t N, int H, int W, int Cin, int Cout, int accumulate, float* workspace, int splitk,
                               int precision, void* stream) {
    const Bwd1x1Call c = {x, ldx, false, dy, lddy, wt, dx, lddx, addend, addend2, ld_addend, ld_addend2, dw};
    return bwd1x1_common("snn_conv1x1_bwd", c, dx, dw, N, H, W, Cin, Cout, accumulate, workspace, splitk, precision, stream);
}

extern "C" int snn_conv1x1_mask_bwd(const uint32_t* mask, int64_t ld_mask, const float* dy, int64_t lddy, const float* wt, float* dx,
                                    int64_t lddx, const float* addend, int64_t ld_addend, const float* addend2,
                                    int64_t ld_addend2, float* dw, int64_t N, int H, int W, int Cin, int Cout, int accumulate,
                                    float* workspace, int splitk, int precision, void* stream) {
    const Bwd1x1Call c = {mask, ld_mask, true, dy, lddy, wt, dx, lddx, addend, addend2, ld_addend, ld_addend2, dw};
    return bwd1x1_common("snn_conv1x1_mask_bwd", c, dx, dw, N, H, W, Cin, Cout, accumulate, workspace, splitk, precision, stream);
}

// dw (+)= the workspace slabs of any weight-gradient launch, in slab order: the reducer every snn_conv2d_wgrad call ends
// with, for a caller that ran the slab kernel with dw = NULL (snn_conv1x1_bwd on the main stream, the reduction elsewhere)
extern "C" int snn_conv2d_wgrad_reduce(float* workspace, float* dw, int64_t n, int splitk, int accumulate, void* stream) {
    SNN_REQUIRE(workspace && dw && n > 0 && splitk >= 1 && splitk <= 32768, "snn_conv2d_wgrad_reduce: bad arguments");
    return wgrad_reduce_slabs(workspace, dw, n, splitk, accumulate, (hipStream_t)stream);
}
