// Pooling with padding and the fused spatial-pyramid forward (gfx950): AvgPool2d / MaxPool2d / SumPool2d(k, stride, pad)
// over channels-last frames [N = T*B][H][W][ld >= C] in fp32, floor mode, 2 <= k <= 7, 1 <= stride <= k, 0 <= pad <= k / 2.
// Memory-bound stencils like the depthwise convolution beside them: a lane owns 4 consecutive channels and uses one 16-byte
// access per pixel when the slice is 16-byte aligned and the pixel stride a multiple of 4; every other layout and the C % 4
// tail go through guarded scalar accesses with the same arithmetic order (ldv / stv).  No atomics, every output element is
// written exactly once, frames never see each other's pixels.
//
// MAX: padding is -inf (an out-of-image tap is skipped, which is the same thing under the rule), the comparison is
// `v > acc || v != v` in window row-major order - ATen's: the first maximum wins a tie, a NaN wins and is only replaced
// by a later NaN.  AVG / SUM: the in-image taps are added one by one in window row-major order, the divisor is k * k
// (count_include_pad), then the expressions of k_pool_fwd / k_pool_bwd (elementwise.hip): at pad = 0 the results have the
// bits of snn_pool_fwd / snn_pool_bwd.
#include "snn_common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;

// 4 consecutive channels from channel c of one pixel (p points at channel c); channels >= C read as zero and are never stored
template <bool VEC> __device__ __forceinline__ f32x4 ldv(const float* __restrict__ p, int c, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC && c + 4 <= C) {
        v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C) v[j] = p[j];
    }
    return v;
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
__device__ __forceinline__ f32x4 splat(float a) { return f32x4{a, a, a, a}; }
// one tap of a max window (ATen's rule, as k_pool_fwd)
__device__ __forceinline__ f32x4 max4(f32x4 acc, f32x4 v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (v[j] > acc[j] || v[j] != v[j]) ? v[j] : acc[j];
    return acc;
}
template <bool MAXK> __device__ __forceinline__ f32x4 tap(f32x4 acc, f32x4 v) {
    if constexpr (MAXK) return max4(acc, v);
    else return acc + v;
}

// ---------------------------------------------------------------------------------------------------- forward
// K > 0: a compile-time instance (K, S, P); K = 0: window, stride and padding from the arguments, the same order of
// operations.  A stride-1 instance produces RUN = 4 output pixels along W per lane: each input row's RUN - 1 + K columns
// are loaded once and reused from registers; the K row re-reads come from L1 / L2.  Work items: (row = n*Ho + ho, run,
// channel group), channel group fastest - the lanes of a wave read consecutive 16-byte pieces of a pixel.
template <int K, int S, int P, bool MAXK, bool VEC>
__global__ __launch_bounds__(kThreads) void k_pool2d_fwd(int kind, const float* __restrict__ x, int64_t ldx,
                                                          float* __restrict__ y, int64_t ldy, int H, int W, int Ho, int Wo,
                                                          int C, int CG, int WR, int rk, int rs, int rp, int64_t total) {
    constexpr int RUN = (K > 0 && S == 1) ? 4 : 1;
    const int k = K ? K : rk, s = K ? S : rs, p = K ? P : rp;
    const float init = MAXK ? -INFINITY : 0.0f;
    const int per_row = WR * CG;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / per_row;
        const int it = (int)(idx - row * per_row);
        const int wr = it / CG;
        const int c = (it - wr * CG) * 4;
        const int64_t n = row / Ho;
        const int ho = (int)(row - n * Ho);
        const int wo0 = wr * RUN;
        const int wi0 = wo0 * s - p;
        f32x4 acc[RUN];
#pragma unroll
        for (int r = 0; r < RUN; ++r) acc[r] = splat(init);
        if constexpr (RUN > 1) {
            constexpr int COLS = RUN - 1 + K;
#pragma unroll
            for (int kh = 0; kh < K; ++kh) {
                const int hi = ho - P + kh;
                if (hi < 0 || hi >= H) continue;
                const float* xr = x + ((n * H + hi) * W) * ldx + c;
                f32x4 col[COLS];
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int wi = wi0 + j;
                    col[j] = (wi >= 0 && wi < W) ? ldv<VEC>(xr + (int64_t)wi * ldx, c, C) : splat(init);
                }
#pragma unroll
                for (int r = 0; r < RUN; ++r)
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) {
                        const int wi = wi0 + r + kw;
                        if (wi >= 0 && wi < W) acc[r] = tap<MAXK>(acc[r], col[r + kw]);
                    }
            }
        } else {
            for (int kh = 0; kh < k; ++kh) {
                const int hi = ho * s - p + kh;
                if (hi < 0 || hi >= H) continue;
                const float* xr = x + ((n * H + hi) * W) * ldx + c;
                for (int kw = 0; kw < k; ++kw) {
                    const int wi = wi0 + kw;
                    if (wi >= 0 && wi < W) acc[0] = tap<MAXK>(acc[0], ldv<VEC>(xr + (int64_t)wi * ldx, c, C));
                }
            }
        }
        float* yr = y + ((n * Ho + ho) * Wo) * ldy + c;
#pragma unroll
        for (int r = 0; r < RUN; ++r) {
            if (wo0 + r >= Wo) continue;
            f32x4 v = acc[r];
            if (kind == SNN_POOL_AVG) v = v / (float)(k * k);
            // SumPool2d = avg_pool2d * k * k: divide then multiply twice, as k_pool_fwd does
            if (kind == SNN_POOL_SUM) v = ((v / (float)(k * k)) * (float)k) * (float)k;
            stv<VEC>(yr + (int64_t)(wo0 + r) * ldy, c, C, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- backward
// A gather: one block owns kBT x kBT input pixels of one frame and kBCG channel groups, one lane one pixel's 4 channels.
// gx = addend (or 0) + the terms of the covering windows in ascending (ho, wo), added one by one.  MAX: the x pixels under
// the windows that reach the tile are staged in LDS once ((kBT + 2 (k - 1))^2 at the most), every such window's arg-max
// is found ONCE from there (k^2 LDS reads, not k^2 loads per covering window and element) and kept as one byte per channel;
// the gather then compares its own tap number with the stored one.  An all -inf window points at its first in-image tap.
// x rows / columns under the windows that reach a tile: kBT + 2 (k - 1) at the most; such windows per dimension: kBT + k - 1
constexpr int kBT = 8, kBCG = 4, kBKmax = 7;

__device__ __forceinline__ int first_window(int h, int k, int s, int p) {   // smallest ho with ho*s - p + k - 1 >= h
    const int t = h + p - k + 1;
    return t <= 0 ? 0 : (t + s - 1) / s;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_pool2d_bwd(int kind, const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ gy, int64_t ldgy,
                                                          const float* __restrict__ add, int64_t ldadd,
                                                          float* __restrict__ gx, int64_t ldgx, int H, int W, int Ho, int Wo,
                                                          int C, int k, int s, int p, int tiles_h, int tiles_w) {
    // dynamic LDS, sized by the launcher for this k (MAX only): the x tile [XR][XR][kBCG] x 16 bytes, then the windows'
    // arg-max bytes [WN][WN][kBCG] x 4 - 18.7 KB at k = 5 (eight blocks per CU), 28.7 KB at k = 7
    extern __shared__ f32x4 pool_lds[];
    const int XR = kBT + 2 * (k - 1), WN = kBT + k - 1;
    f32x4* sx = pool_lds;
    unsigned* sarg = reinterpret_cast<unsigned*>(pool_lds + XR * XR * kBCG);
    const int tid = threadIdx.x;
    const int cg = tid & (kBCG - 1), pix = tid >> 2;
    const int c = (int)(blockIdx.y * kBCG + cg) * 4;
    unsigned b = blockIdx.x;
    const int tw = (int)(b % (unsigned)tiles_w);
    b /= (unsigned)tiles_w;
    const int th = (int)(b % (unsigned)tiles_h);
    const int64_t n = b / (unsigned)tiles_h;
    const int h0 = th * kBT, w0 = tw * kBT;
    // the windows that reach the tile's pixels
    const int ho_lo = first_window(h0, k, s, p), wo_lo = first_window(w0, k, s, p);
    const int ho_hi = std::min(Ho - 1, (std::min(h0 + kBT, H) - 1 + p) / s);
    const int wo_hi = std::min(Wo - 1, (std::min(w0 + kBT, W) - 1 + p) / s);
    const int nwh = std::max(0, ho_hi - ho_lo + 1), nww = std::max(0, wo_hi - wo_lo + 1);
    if (kind == SNN_POOL_MAX) {   // (block-uniform: the barriers below are reached by every lane)
        const int xr0 = ho_lo * s - p, xc0 = wo_lo * s - p;
        const int xrows = nwh ? (nwh - 1) * s + k : 0, xcols = nww ? (nww - 1) * s + k : 0;
        for (int i = pix; i < xrows * xcols; i += kThreads / kBCG) {
            const int rr = i / xcols, cc = i - rr * xcols;
            const int hi = xr0 + rr, wi = xc0 + cc;
            if (hi >= 0 && hi < H && wi >= 0 && wi < W && c < C)
                sx[(rr * XR + cc) * kBCG + cg] = ldv<VEC>(x + ((n * H + hi) * W + wi) * ldx + c, c, C);
        }
        __syncthreads();
        for (int i = pix; i < nwh * nww; i += kThreads / kBCG) {
            const int a = i / nww, bb = i - a * nww;
            f32x4 best = splat(-INFINITY);
            int arg[4] = {-1, -1, -1, -1};
            if (c < C)
                for (int kh = 0; kh < k; ++kh) {
                    const int hi = xr0 + a * s + kh;
                    if (hi < 0 || hi >= H) continue;
                    for (int kw = 0; kw < k; ++kw) {
                        const int wi = xc0 + bb * s + kw;
                        if (wi < 0 || wi >= W) continue;
                        const f32x4 v = sx[((a * s + kh) * XR + bb * s + kw) * kBCG + cg];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (arg[j] < 0 || v[j] > best[j] || v[j] != v[j]) {
                                best[j] = v[j];
                                arg[j] = kh * k + kw;
                            }
                    }
                }
            sarg[(a * WN + bb) * kBCG + cg] = (unsigned)(arg[0] & 255) | (unsigned)(arg[1] & 255) << 8 |
                                                (unsigned)(arg[2] & 255) << 16 | (unsigned)(arg[3] & 255) << 24;
        }
        __syncthreads();
    }
    const int h = h0 + (pix >> 3), w = w0 + (pix & (kBT - 1));
    if (h >= H || w >= W || c >= C) return;
    const int64_t e = (n * H + h) * W + w;
    f32x4 acc = add ? ldv<VEC>(add + e * ldadd + c, c, C) : splat(0.0f);
    const int hlo = first_window(h, k, s, p), wlo = first_window(w, k, s, p);
    const int hhi = std::min(Ho - 1, (h + p) / s), whi = std::min(Wo - 1, (w + p) / s);
    const float kk = (float)(k * k), kf = (float)k;
    for (int ho = hlo; ho <= hhi; ++ho)
        for (int wo = wlo; wo <= whi; ++wo) {
            const f32x4 g = ldv<VEC>(gy + ((n * Ho + ho) * Wo + wo) * ldgy + c, c, C);
            if (kind == SNN_POOL_MAX) {
                const unsigned mine = (unsigned)((h - (ho * s - p)) * k + (w - (wo * s - p)));
                const unsigned ua = sarg[((ho - ho_lo) * WN + (wo - wo_lo)) * kBCG + cg];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (((ua >> (8 * j)) & 255u) == mine) acc[j] += g[j];
            } else if (kind == SNN_POOL_AVG) {
                acc = acc + g / kk;
            } else {
                acc = acc + ((g * kf) * kf) / kk;
            }
        }
    stv<VEC>(gx + e * ldgx + c, c, C, acc);
}

// ---------------------------------------------------------------------------------------------------- SPP forward
// y = [x | m_1 | ... | m_L] on channels, m_j = MaxPool(K, 1, K / 2)(m_{j-1}), m_0 = x: the chain itself, level by level, so
// the bits are those of L calls of snn_pool2d_fwd.  A K x K max under the rule above is separable without changing which
// element wins: the row pass keeps the first maximum (last NaN) of a row, the column pass the first row (last NaN row).
//
// A block owns RW = 2^rw_log2 columns x 256 / RW channel groups of one frame and walks DOWN the rows r of its row chunk
// (with R = L * (K / 2) rows of run-in above and below).  Per step a lane loads ONE x pixel (its column, 4 channels; the
// next row's load is already in flight), and for each level: the lanes exchange the level's newest row through LDS, a
// lane takes the row maximum over its K neighbours, pushes it into a K-deep register window and emits the column maximum
// of the window - the next level's newest row, K / 2 rows higher up.  LDS holds one row per level and step parity (24 KiB
// static: six blocks per CU by LDS); x is read from HBM once per row chunk, the run-in rows again by the chunk's neighbour.
// Absent pixels (outside the image, channels >= C) are -inf at EVERY level - padding of the chained pools - while pixels
// of the image outside the block's region are merely not read: what they would change lies within R of the region's
// edge, and only pixels at least R inside it (or at an image edge) are stored.
template <int K, int L, bool VEC>
__global__ __launch_bounds__(kThreads) void k_spp_fwd(const float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                       int64_t ldy, int H, int W, int C, int rw_log2, int col_tiles,
                                                       int tile_w, int row_chunks, int tile_h) {
    constexpr int HK = K / 2, R = L * HK;
    __shared__ f32x4 sl[2][L][kThreads];
    const int tid = threadIdx.x;
    const int cgb_log2 = 8 - rw_log2, RW = 1 << rw_log2;
    const int cg = tid & ((1 << cgb_log2) - 1), col = tid >> cgb_log2;
    const int c = (int)((blockIdx.y << cgb_log2) + cg) * 4;
    unsigned b = blockIdx.x;
    const int ct = (int)(b % (unsigned)col_tiles);
    b /= (unsigned)col_tiles;
    const int rc = (int)(b % (unsigned)row_chunks);
    const int64_t n = b / (unsigned)row_chunks;
    const int wbase = col_tiles == 1 ? 0 : ct * tile_w - R;
    const int w = wbase + col;
    const int wo_lo = ct * tile_w, wo_hi = std::min(W, wo_lo + tile_w);   // columns this block stores
    const bool present = w >= 0 && w < W && c < C;
    const bool stores = present && w >= wo_lo && w < wo_hi;
    const int h0 = rc * tile_h, h1 = std::min(H, h0 + tile_h);            // rows this block stores
    const int ra = std::max(0, h0 - R), rb = std::min(H, h1 + R);         // rows it reads
    const float* xp = x + ((n * H) * W + (present ? w : 0)) * ldx + c;
    float* yp = y + ((n * H) * W + (present ? w : 0)) * ldy + c;
    const int64_t xrow = (int64_t)W * ldx, yrow = (int64_t)W * ldy;
    const f32x4 ninf = splat(-INFINITY);
    f32x4 win[L][K];
#pragma unroll
    for (int j = 0; j < L; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) win[j][i] = ninf;
    f32x4 nxt = present ? ldv<VEC>(xp + ra * xrow, c, C) : ninf;
    for (int r = ra; r < h1 + R; ++r) {   // (block-uniform bounds: barriers inside)
        const int par = (r - ra) & 1;
        f32x4 cur = nxt;
        nxt = (present && r + 1 < rb) ? ldv<VEC>(xp + (r + 1) * xrow, c, C) : ninf;
        if (stores && r >= h0 && r < h1) stv<VEC>(yp + r * yrow, c, C, cur);
#pragma unroll
        for (int j = 0; j < L; ++j) {   // level j + 1 from level j, whose newest row is `cur` (row r - j * HK)
            sl[par][j][tid] = cur;
            __syncthreads();
            f32x4 rm = ninf;
#pragma unroll
            for (int d = -HK; d <= HK; ++d) {
                const int cc = col + d;
                if (cc >= 0 && cc < RW) rm = max4(rm, sl[par][j][(cc << cgb_log2) + cg]);
            }
#pragma unroll
            for (int i = 0; i + 1 < K; ++i) win[j][i] = win[j][i + 1];
            win[j][K - 1] = rm;
            f32x4 out = ninf;
#pragma unroll
            for (int i = 0; i < K; ++i) out = max4(out, win[j][i]);
            const int rj = r - (j + 1) * HK;   // the row of level j + 1 this is
            if (stores && rj >= h0 && rj < h1) stv<VEC>(yp + rj * yrow + (int64_t)(j + 1) * C, c, C, out);
            cur = (present && rj >= 0 && rj < H) ? out : ninf;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static int out_size(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

static bool pool2d_supported(int64_t N, int H, int W, int C, int k, int stride, int pad) {
    if (k < 2 || k > kBKmax || stride < 1 || stride > k || pad < 0 || pad > k / 2) return false;
    if (N < 1 || H < 1 || W < 1 || C < 1) return false;
    if (H + 2 * pad < k || W + 2 * pad < k) return false;
    // pixel indices are 32-bit in the kernels (element offsets are 64-bit)
    return N <= (int64_t)0x7fffffff / ((int64_t)H * W);
}
static bool spp_supported(int64_t N, int H, int W, int C, int k, int levels) {
    if (!(k == 3 || k == 5) || levels < 1 || levels > 3) return false;
    if (N < 1 || H < 1 || W < 1 || C < 1) return false;
    return N <= (int64_t)0x7fffffff / ((int64_t)H * W);
}

#define POOL2D_COVERED "2 <= k <= 7, 1 <= stride <= k, 0 <= pad <= k / 2, H + 2 pad >= k, W + 2 pad >= k, N * H * W < 2^31"

}  // namespace

extern "C" int snn_pool2d_supported(int64_t N, int H, int W, int C, int k, int stride, int pad) {
    return pool2d_supported(N, H, W, C, k, stride, pad) ? 1 : 0;
}

extern "C" int snn_pool2d_fwd(int kind, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t N, int H, int W, int C,
                              int k, int stride, int pad, void* stream) {
    SNN_REQUIRE(x && y, "snn_pool2d_fwd: null pointer");
    SNN_REQUIRE(kind >= SNN_POOL_AVG && kind <= SNN_POOL_SUM, "snn_pool2d_fwd: bad pool kind %d", kind);
    SNN_REQUIRE(pool2d_supported(N, H, W, C, k, stride, pad),
                "snn_pool2d_fwd: not covered (N %lld, %dx%d, C %d, k %d, stride %d, pad %d): " POOL2D_COVERED, (long long)N,
                H, W, C, k, stride, pad);
    SNN_REQUIRE(ldx >= C && ldy >= C, "snn_pool2d_fwd: pixel strides %lld / %lld below the %d channels", (long long)ldx,
                (long long)ldy, C);
    const int Ho = out_size(H, k, stride, pad), Wo = out_size(W, k, stride, pad);
    const int run = ((k == 5 && pad == 2) || (k == 3 && pad == 1)) && stride == 1 ? 4 : 1;
    const int CG = (C + 3) / 4, WR = (Wo + run - 1) / run;
    SNN_REQUIRE((int64_t)WR * CG <= 0x7fffffff, "snn_pool2d_fwd: a row of %d pixels x %d channels is too long", Wo, C);
    const int64_t total = N * Ho * WR * CG;
    const bool vec = aligned(16, {x, y}) && multiples(4, {ldx, ldy});
    // (k, stride, pad) packed into one value: the compiled instances, 0 = the runtime path
    const int ksp = k * 100 + stride * 10 + pad;
    const int inst = (ksp == 220 || ksp == 321 || ksp == 512 || ksp == 311) ? ksp : 0;
    hipStream_t st = (hipStream_t)stream;
    const bool launched = dispatch(
        [&](auto I, auto MX, auto VEC) {
            constexpr int KC = I() / 100, SC = I() / 10 % 10, PC = I() % 10;
            hipLaunchKernelGGL((k_pool2d_fwd<KC, SC, PC, MX(), VEC()>), dim3(snn_grid_for(total, kThreads)), dim3(kThreads), 0,
                               st, kind, x, ldx, y, ldy, H, W, Ho, Wo, C, CG, WR, k, stride, pad, total);
            return true;
        },
        OneOf<0, 220, 321, 512, 311>{inst}, Flag{kind == SNN_POOL_MAX}, Flag{vec});
    SNN_REQUIRE(launched, "snn_pool2d_fwd: no kernel instance (k %d, stride %d, pad %d)", k, stride, pad);
    SNN_CHECK_LAUNCH("snn_pool2d_fwd");
    return 0;
}

extern "C" int snn_pool2d_bwd(int kind, const float* x, int64_t ldx, const float* gy, int64_t ldgy, const float* addend,
                              int64_t ldadd, float* gx, int64_t ldgx, int64_t N, int H, int W, int C, int k, int stride,
                              int pad, void* stream) {
    SNN_REQUIRE(gy && gx, "snn_pool2d_bwd: null pointer");
    SNN_REQUIRE(kind >= SNN_POOL_AVG && kind <= SNN_POOL_SUM, "snn_pool2d_bwd: bad pool kind %d", kind);
    SNN_REQUIRE(kind != SNN_POOL_MAX || x, "snn_pool2d_bwd: max pooling needs the forward input (null pointer)");
    SNN_REQUIRE(pool2d_supported(N, H, W, C, k, stride, pad),
                "snn_pool2d_bwd: not covered (N %lld, %dx%d, C %d, k %d, stride %d, pad %d): " POOL2D_COVERED, (long long)N,
                H, W, C, k, stride, pad);
    SNN_REQUIRE(ldgy >= C && ldgx >= C && (kind != SNN_POOL_MAX || ldx >= C) && (!addend || ldadd >= C),
                "snn_pool2d_bwd: pixel strides %lld / %lld / %lld / %lld below the %d channels", (long long)ldx,
                (long long)ldgy, (long long)ldadd, (long long)ldgx, C);
    SNN_REQUIRE(addend != gx, "snn_pool2d_bwd: addend must not alias gx");
    const int Ho = out_size(H, k, stride, pad), Wo = out_size(W, k, stride, pad);
    const int tiles_h = (H + kBT - 1) / kBT, tiles_w = (W + kBT - 1) / kBT;
    const int64_t gyb = ((int64_t)(C + 3) / 4 + kBCG - 1) / kBCG;
    SNN_REQUIRE(gyb <= 65535, "snn_pool2d_bwd: %d channels are too many", C);
    const float* xm = kind == SNN_POOL_MAX ? x : nullptr;
    const bool vec = aligned(16, {xm, gy, addend, gx}) && multiples(4, {xm ? ldx : 0, ldgy, addend ? ldadd : 0, ldgx});
    const unsigned blocks = (unsigned)(N * tiles_h * tiles_w);   // < 2^31: N * H * W is
    const int xr = kBT + 2 * (k - 1), wn = kBT + k - 1;
    const size_t lds = xm ? (size_t)kBCG * (xr * xr * sizeof(f32x4) + wn * wn * sizeof(unsigned)) : 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_pool2d_bwd<true>, dim3(blocks, (unsigned)gyb), dim3(kThreads), lds, st, kind, xm, ldx, gy, ldgy,
                           addend, ldadd, gx, ldgx, H, W, Ho, Wo, C, k, stride, pad, tiles_h, tiles_w);
    else
        hipLaunchKernelGGL(k_pool2d_bwd<false>, dim3(blocks, (unsigned)gyb), dim3(kThreads), lds, st, kind, xm, ldx, gy, ldgy,
                           addend, ldadd, gx, ldgx, H, W, Ho, Wo, C, k, stride, pad, tiles_h, tiles_w);
    SNN_CHECK_LAUNCH("snn_pool2d_bwd");
    return 0;
}

extern "C" int snn_spp_supported(int64_t N, int H, int W, int C, int k, int levels) {
    return spp_supported(N, H, W, C, k, levels) ? 1 : 0;
}

extern "C" int snn_spp_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t N, int H, int W, int C, int k,
                           int levels, void* stream) {
    SNN_REQUIRE(x && y, "snn_spp_fwd: null pointer");
    SNN_REQUIRE(spp_supported(N, H, W, C, k, levels),
                "snn_spp_fwd: not covered (N %lld, %dx%d, C %d, k %d, levels %d): k in {3, 5}, levels in {1, 2, 3}, "
                "N * H * W < 2^31", (long long)N, H, W, C, k, levels);
    SNN_REQUIRE(ldx >= C && ldy >= (int64_t)(levels + 1) * C,
                "snn_spp_fwd: pixel strides %lld / %lld below the %d / %lld channels", (long long)ldx, (long long)ldy, C,
                (long long)(levels + 1) * C);
    // plan: a function of the shape only.  Columns: the whole width when it fits 64 lanes, else tiles with a run-in of R
    const int R = levels * (k / 2);
    const int rw_log2 = W <= 16 ? 4 : W <= 32 ? 5 : 6;
    const int tile_w = W <= 64 ? W : 64 - 2 * R;
    const int col_tiles = (W + tile_w - 1) / tile_w;
    const int cgb = kThreads >> rw_log2;
    const int64_t gyb = ((int64_t)(C + 3) / 4 + cgb - 1) / cgb;
    SNN_REQUIRE(gyb <= 65535, "snn_spp_fwd: %d channels are too many", C);
    // rows: chunks of at least 16 rows, as many as it takes to reach about eight blocks per CU
    const int64_t base = N * col_tiles * gyb;
    int row_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(snn_ceil_div(2048, base), H / 16));
    const int tile_h = (H + row_chunks - 1) / row_chunks;
    row_chunks = (H + tile_h - 1) / tile_h;
    // C % 4 != 0 puts slices 1.. at channel offsets that are no multiple of 4: the scalar path
    const bool vec = aligned(16, {x, y}) && multiples(4, {ldx, ldy, (int64_t)C});
    const unsigned blocks = (unsigned)(N * row_chunks * col_tiles);
    hipStream_t st = (hipStream_t)stream;
    const bool launched = dispatch(
        [&](auto KC, auto LC, auto VEC) {
            hipLaunchKernelGGL((k_spp_fwd<KC(), LC(), VEC()>), dim3(blocks, (unsigned)gyb), dim3(kThreads), 0, st, x, ldx, y,
                               ldy, H, W, C, rw_log2, col_tiles, tile_w, row_chunks, tile_h);
            return true;
        },
        OneOf<3, 5>{k}, OneOf<1, 2, 3>{levels}, Flag{vec});
    SNN_REQUIRE(launched, "snn_spp_fwd: no kernel instance (k %d, levels %d)", k, levels);
    SNN_CHECK_LAUNCH("snn_spp_fwd");
    return 0;
}
