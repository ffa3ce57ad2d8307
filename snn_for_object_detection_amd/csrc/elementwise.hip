// Layout adapters, merges (Residual sum / Dense concat slices), pointwise activations, pooling,
// nearest upsampling, fused Adamax and event voxelisation for gfx950.  All HBM-bound: 16-byte
// lane-contiguous accesses where the shape allows, grid-stride loops capped at 8 blocks / CU.
#include <stdarg.h>
#include "snn_common.h"

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void snn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* snn_last_error(void) { return g_err; }
extern "C" int snn_abi_version(void) { return SNN_ABI_VERSION; }

namespace {

constexpr int kThreads = 256;

static unsigned grid_for(int64_t n) {
    int64_t b = snn_ceil_div(n, kThreads);
    if (b > snn_max_blocks()) b = snn_max_blocks();
    if (b < 1) b = 1;
    return (unsigned)b;
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ------------------------------------------------------------------------------------------ layout
// [N][C][HW] -> [N][HW][C] through a 32x33 LDS tile: both sides coalesced.
__global__ void k_transpose_cp(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
    // per image: src is [rows][cols], dst is [cols][rows]
    __shared__ float tile[32][33];
    const int64_t img = blockIdx.z;
    const float* s = src + img * (int64_t)rows * cols;
    float* d = dst + img * (int64_t)rows * cols;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int r = r0 + j, c = c0 + threadIdx.x;
        if (r < rows && c < cols) tile[j][threadIdx.x] = s[(int64_t)r * cols + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int c = c0 + j, r = r0 + threadIdx.x;
        if (r < rows && c < cols) d[(int64_t)c * rows + r] = tile[threadIdx.x][j];
    }
}

// small-channel NCHW -> NHWC (C <= 4, e.g. the 2-polarity event frames): one thread per pixel
template <int C>
__global__ void k_nchw_to_nhwc_small(const float* __restrict__ src, float* __restrict__ dst, int64_t N, int64_t HW) {
    const int64_t total = N * HW;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t n = e / HW, px = e % HW;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = src[(n * C + c) * HW + px];
#pragma unroll
        for (int c = 0; c < C; ++c) dst[e * C + c] = v[c];
    }
}

__global__ void k_weight_transpose(const float* __restrict__ w, float* __restrict__ wt, int Cout, int taps, int Cin) {
    const int64_t total = (int64_t)Cout * taps * Cin;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        // e indexes wt[ci][tap][co]
        int co = (int)(e % Cout);
        int64_t r = e / Cout;
        int tap = (int)(r % taps);
        int ci = (int)(r / taps);
        wt[e] = w[((int64_t)co * taps + tap) * Cin + ci];
    }
}

// All conv weights of a flat parameter buffer in one launch: table[l] = {offset, Cout, taps, Cin}; block (x, l)
// walks layer l with stride gridDim.x.  (47 per-layer launches of 6.5 us each sat in the backward critical path.)
__global__ void k_weight_transpose_batched(const float* __restrict__ flat_w, float* __restrict__ flat_wt,
                                           const int64_t* __restrict__ table) {
    // Per tap a Cout x Cin matrix is transposed in 32 x 32 tiles through LDS: rows of 32 consecutive ci are read (128
    // contiguous bytes), rows of 32 consecutive co are written.  (The first form gathered one element per lane with a
    // stride of taps * Cin floats - every lane its own cache line: 43 us between the optimiser and the first forward kernel
    // of every step.)  32-bit index arithmetic: a layer's weights are far below 2^31 elements (the caller that builds the
    // device-side table checks it).
    __shared__ float tile[32][33];
    const int64_t* d = table + (int64_t)blockIdx.y * 4;
    const int64_t off = d[0];
    const unsigned Cout = (unsigned)d[1], taps = (unsigned)d[2], Cin = (unsigned)d[3];
    const float* w = flat_w + off;
    float* wt = flat_wt + off;
    const unsigned tco = (Cout + 31) / 32, tci = (Cin + 31) / 32;
    const unsigned ntiles = taps * tco * tci;
    const unsigned tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads
    for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned tap = t / (tco * tci), rem = t - tap * (tco * tci);
        const unsigned co0 = (rem / tci) * 32, ci0 = (rem % tci) * 32;
#pragma unroll
        for (unsigned k = 0; k < 32; k += 8) {
            const unsigned co = co0 + ty + k, ci = ci0 + tx;
            if (co < Cout && ci < Cin) tile[ty + k][tx] = w[(co * taps + tap) * Cin + ci];
        }
        __syncthreads();
#pragma unroll
        for (unsigned k = 0; k < 32; k += 8) {
            const unsigned ci = ci0 + ty + k, co = co0 + tx;
            if (ci < Cin && co < Cout) wt[(ci * taps + tap) * Cout + co] = tile[tx][ty + k];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ merges
template <int VEC, bool ADD>
__global__ void k_channels(const float* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd, int64_t M,
                           int C) {
    const int cv = C / VEC;
    const int64_t total = M * cv;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t m = e / cv;
        const int c = (int)(e % cv) * VEC;
        if (VEC == 4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + m * lds + c);
            f32x4* d = reinterpret_cast<f32x4*>(dst + m * ldd + c);
            if (ADD) v += *d;
            *d = v;
        } else {
            float v = src[m * lds + c];
            if (ADD) v += dst[m * ldd + c];
            dst[m * ldd + c] = v;
        }
    }
}

template <int VEC>
__global__ void k_add(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                      float* __restrict__ dst, int64_t ldd, int64_t M, int C) {
    const int cv = C / VEC;
    const int64_t total = M * cv;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t m = e / cv;
        const int c = (int)(e % cv) * VEC;
        if (VEC == 4) {
            f32x4 x = *reinterpret_cast<const f32x4*>(a + m * lda + c);
            f32x4 y = *reinterpret_cast<const f32x4*>(b + m * ldb + c);
            *reinterpret_cast<f32x4*>(dst + m * ldd + c) = x + y;
        } else {
            dst[m * ldd + c] = a[m * lda + c] + b[m * ldb + c];
        }
    }
}

// the merges of the bf16-storage mode (SnnStore<true>, snn_common.h): bf16 tensors, the sum formed in fp32 and rounded once.
// MODE 0: dst = a (copy), 1: dst = a + b.  VEC 4 (8-byte accesses) or 1.
template <int VEC, int MODE>
__global__ void k_merge_bf16(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                             float* __restrict__ dst, int64_t ldd, int64_t M, int C) {
    typedef SnnStore<true> St;
    const int cv = C / VEC;
    const int64_t total = M * cv;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t m = e / cv;
        const int c = (int)(e % cv) * VEC;
        if (VEC == 4) {
            f32x4 v = St::ld4(a, m * lda + c);
            if (MODE == 1) v += St::ld4(b, m * ldb + c);
            St::st4(dst, m * ldd + c, v);
        } else {
            float v = St::ld1(a, m * lda + c);
            if (MODE == 1) v += St::ld1(b, m * ldb + c);
            St::st1(dst, m * ldd + c, v);
        }
    }
}

// fp32 <-> bf16 (round to nearest even), dense: the boundary of the bf16-storage domain (the head's last-step read-out)
template <bool TO_BF16>
__global__ void k_convert_bf16(const void* __restrict__ src, void* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (TO_BF16) SnnStore<true>::st1(dst, i, static_cast<const float*>(src)[i]);
        else static_cast<float*>(dst)[i] = SnnStore<true>::ld1(src, i);
    }
}

// ------------------------------------------------------------------------------------------ activations
__device__ __forceinline__ float act_f(int act, float x) {
    switch (act) {
        case SNN_ACT_RELU: return x > 0.0f ? x : 0.0f;
        case SNN_ACT_SILU: return x / (1.0f + expf(-x));
        default: return tanhf(x);
    }
}
__device__ __forceinline__ float act_g(int act, float x, float y) {
    switch (act) {
        case SNN_ACT_RELU: return x > 0.0f ? 1.0f : 0.0f;
        case SNN_ACT_SILU: {
            float s = 1.0f / (1.0f + expf(-x));
            return s * (1.0f + x * (1.0f - s));
        }
        default: return 1.0f - y * y;
    }
}
__global__ void k_act_fwd(int act, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads)
        y[e] = act_f(act, x[e]);
}
__global__ void k_act_bwd(int act, const float* __restrict__ x, const float* __restrict__ y,
                          const float* __restrict__ gy, float* __restrict__ gx, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads)
        gx[e] = gy[e] * act_g(act, x[e], y[e]);
}

// ------------------------------------------------------------------------------------------ ConvLSTM cell
// gates[m][4C] = (input, forget, output, candidate) pre-activations, conv_lstm.py:66-76 (sigmoidf_: snn_common.h)

__global__ void k_lstm_fwd(const float* __restrict__ gates, const float* __restrict__ c_prev, float* __restrict__ h,
                           float* __restrict__ c, int64_t M, int C) {
    const int64_t total = M * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t m = e / C;
        const int ch = (int)(e % C);
        const float* g = gates + m * 4 * C;
        const float I = sigmoidf_(g[ch]), F = sigmoidf_(g[C + ch]), O = sigmoidf_(g[2 * C + ch]);
        const float G = tanhf(g[3 * C + ch]);
        const float cp = c_prev ? c_prev[e] : 0.0f;
        const float cn = F * cp + I * G;
        c[e] = cn;
        h[e] = O * tanhf(cn);
    }
}

__global__ void k_lstm_bwd(const float* __restrict__ gates, const float* __restrict__ c_prev,
                           const float* __restrict__ c, const float* __restrict__ gh, const float* __restrict__ gc,
                           float* __restrict__ g_gates, float* __restrict__ g_c_prev, int64_t M, int C) {
    const int64_t total = M * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t m = e / C;
        const int ch = (int)(e % C);
        const float* g = gates + m * 4 * C;
        const float I = sigmoidf_(g[ch]), F = sigmoidf_(g[C + ch]), O = sigmoidf_(g[2 * C + ch]);
        const float G = tanhf(g[3 * C + ch]);
        const float tc = tanhf(c[e]);
        const float dh = gh ? gh[e] : 0.0f;
        const float dc = (gc ? gc[e] : 0.0f) + dh * O * (1.0f - tc * tc);
        const float cp = c_prev ? c_prev[e] : 0.0f;
        float* d = g_gates + m * 4 * C;
        d[ch] = (dc * G) * (I * (1.0f - I));
        d[C + ch] = (dc * cp) * (F * (1.0f - F));
        d[2 * C + ch] = (dh * tc) * (O * (1.0f - O));
        d[3 * C + ch] = (dc * I) * (1.0f - G * G);
        if (g_c_prev) g_c_prev[e] = dc * F;
    }
}

// ------------------------------------------------------------------------------------------ pooling
__global__ void k_pool_fwd(int kind, const float* __restrict__ x, float* __restrict__ y, int64_t N, int H, int W, int C,
                           int Ho, int Wo, int k, int stride) {
    const int64_t total = N * Ho * Wo * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        int c = (int)(e % C);
        int64_t r = e / C;
        int wo = (int)(r % Wo);
        r /= Wo;
        int ho = (int)(r % Ho);
        int64_t n = r / Ho;
        float acc = (kind == SNN_POOL_MAX) ? -INFINITY : 0.0f;
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) {
                float v = x[((n * H + ho * stride + i) * W + wo * stride + j) * C + c];
                if (kind == SNN_POOL_MAX) acc = (v > acc || v != v) ? v : acc;
                else acc += v;
            }
        if (kind == SNN_POOL_AVG) acc = acc / (float)(k * k);
        // SumPool2d = avg_pool2d * k * k (common.py:44-48): divide then multiply twice, as the reference does
        if (kind == SNN_POOL_SUM) acc = ((acc / (float)(k * k)) * (float)k) * (float)k;
        y[e] = acc;
    }
}

// one thread per INPUT element: gathers from every window that covers it (windows overlap when stride < k)
__global__ void k_pool_bwd(int kind, const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx,
                           int64_t N, int H, int W, int C, int Ho, int Wo, int k, int stride) {
    const int64_t total = N * H * W * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        int c = (int)(e % C);
        int64_t r = e / C;
        int w = (int)(r % W);
        r /= W;
        int h = (int)(r % H);
        int64_t n = r / H;
        float acc = 0.0f;
        int ho_lo = (h - k + stride) / stride;
        if (h - k + 1 < 0) ho_lo = 0;
        int wo_lo = (w - k + stride) / stride;
        if (w - k + 1 < 0) wo_lo = 0;
        for (int ho = ho_lo; ho < Ho && ho * stride <= h; ++ho)
            for (int wo = wo_lo; wo < Wo && wo * stride <= w; ++wo) {
                if (h - ho * stride >= k || w - wo * stride >= k) continue;
                float g = gy[((n * Ho + ho) * Wo + wo) * C + c];
                if (kind == SNN_POOL_MAX) {
                    // gradient goes to the FIRST maximal element of the window (ATen max_pool2d)
                    float best = -INFINITY;
                    int bi = 0, bj = 0;
                    for (int i = 0; i < k; ++i)
                        for (int j = 0; j < k; ++j) {
                            float v = x[((n * H + ho * stride + i) * W + wo * stride + j) * C + c];
                            if (v > best || v != v) { best = v; bi = i; bj = j; }
                        }
                    if (ho * stride + bi == h && wo * stride + bj == w) acc += g;
                } else if (kind == SNN_POOL_AVG) {
                    acc += g / (float)(k * k);
                } else {
                    acc += ((g * (float)k) * (float)k) / (float)(k * k);
                }
            }
        gx[e] = acc;
    }
}

__global__ void k_upsample_fwd(const float* __restrict__ x, float* __restrict__ y, int64_t N, int H, int W, int C,
                               int s) {
    const int Ho = H * s, Wo = W * s;
    const int64_t total = N * Ho * Wo * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        int c = (int)(e % C);
        int64_t r = e / C;
        int wo = (int)(r % Wo);
        r /= Wo;
        int ho = (int)(r % Ho);
        int64_t n = r / Ho;
        y[e] = x[((n * H + ho / s) * W + wo / s) * C + c];
    }
}
__global__ void k_upsample_bwd(const float* __restrict__ gy, float* __restrict__ gx, int64_t N, int H, int W, int C,
                               int s) {
    const int Ho = H * s, Wo = W * s;
    const int64_t total = N * H * W * C;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        int c = (int)(e % C);
        int64_t r = e / C;
        int w = (int)(r % W);
        r /= W;
        int h = (int)(r % H);
        int64_t n = r / H;
        float acc = 0.0f;
        for (int i = 0; i < s; ++i)
            for (int j = 0; j < s; ++j) acc += gy[((n * Ho + h * s + i) * Wo + w * s + j) * C + c];
        gx[e] = acc;
    }
}

// ------------------------------------------------------------------------------------------ optimizer
// One body, four kernels in front of it.  CTL = false is the plain step; CTL = true adds, in the order of clip_grad_* followed
// by torch.optim.Adamax: the control record's clip factor, the value clamp, the weight decay - and stores NOTHING when the
// record says the gradient was not finite (the moments would stay non-finite for ever: u = max(b2 * inf, ...) = inf).
// EMA = true moves the weight average towards the parameter it has just written, ema += ew * (p_new - ema) with
// ew = 1 - decay formed by the caller: 8 more bytes per element in the pass that holds p_new in a register anyway.  The
// parameter and both moments are computed by the same expressions in the same order whatever EMA is: the same bits.
template <bool CTL, bool EMA>
__device__ __forceinline__ void adamax_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr,
                                            float gscale, float wd, float clip, const snn_step_control* __restrict__ ctl,
                                            float* __restrict__ ema, float ew) {
    float cscale = 1.0f;
    if constexpr (CTL) {
        if (ctl) {
            if (!ctl->finite) return;
            cscale = ctl->scale;
        }
    }
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        float ge = g[e] * gscale;  // gscale = 1/world_size after a SUM all-reduce (exact for powers of two)
        if constexpr (CTL) {
            ge *= cscale;                                                      // clip_grad_norm_: grad.mul_(clip_coef)
            if (clip > 0.0f) ge = ge < -clip ? -clip : (ge > clip ? clip : ge);  // clip_grad_value_ (a NaN stays a NaN)
            if (wd != 0.0f) ge += wd * p[e];                                   // grad.add(param, alpha=weight_decay)
        }
        // torch.optim.Adamax single-tensor: exp_avg.lerp_(grad, 1-beta1); exp_inf = max(exp_inf*beta2, |g|+eps)
        float me = m[e] + w1 * (ge - m[e]);
        float ue = fmaxf(u[e] * b2, fabsf(ge) + eps);
        m[e] = me;
        u[e] = ue;
        const float pe = p[e] - clr * (me / ue);
        p[e] = pe;
        if constexpr (EMA) {
            const float a = ema[e];
            ema[e] = a + ew * (pe - a);
        }
    }
}
__global__ void k_adamax(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                         float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr, float gscale) {
    adamax_body<false, false>(p, g, m, u, n, w1, b2, eps, clr, gscale, 0.0f, 0.0f, nullptr, nullptr, 0.0f);
}
__global__ void k_adamax_ctl(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr, float gscale,
                             float wd, float clip, const snn_step_control* __restrict__ ctl) {
    adamax_body<true, false>(p, g, m, u, n, w1, b2, eps, clr, gscale, wd, clip, ctl, nullptr, 0.0f);
}
// CTL mirrors snn_adamax_step_ctl's choice between the two kernels above, so the parameter and the moments come out of the
// same instantiation of the arithmetic in either case.
template <bool CTL>
__global__ void k_adamax_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ u, float* __restrict__ ema, int64_t n, float w1, float b2, float eps,
                             float clr, float gscale, float wd, float clip, float ew,
                             const snn_step_control* __restrict__ ctl) {
    adamax_body<CTL, true>(p, g, m, u, n, w1, b2, eps, clr, gscale, wd, clip, ctl, ema, ew);
}
// The same update from an arbitrary source: parameters that received no gradient in a step (Adamax leaves them alone, the
// average does not) and the BatchNorm buffers.  A record that says "not finite" stores nothing here either.
__global__ void k_ema_update(float* __restrict__ ema, const float* __restrict__ src, int64_t n, float ew,
                             const snn_step_control* __restrict__ ctl) {
    if (ctl && !ctl->finite) return;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const float a = ema[e];
        ema[e] = a + ew * (src[e] - a);
    }
}

// ------------------------------------------------------------------------------------------ gradient norm
// sum g^2 over a flat gradient, bitwise reproducible: block b owns the kNormRun elements [b * kNormRun, (b + 1) * kNormRun)
// of the buffer counted from the 16-byte boundary at or below its first element (`shift` = 0..3 floats in front of it), so
// every full group of four is one aligned 16-byte load whatever the base pointer is; the groups cut by either end of the
// buffer (at most two in the whole launch) are read element by element.  A thread adds its squares in index order, the wave
// and the block combine in a fixed butterfly, and the second kernel adds the block partials in index order: no atomics,
// and nothing that depends on the device - the run length is a constant, not a function of the CU count.
constexpr int kNormRun = 8192;
constexpr int kNormGroups = kNormRun / (4 * kThreads);   // 16-byte groups per thread

__device__ __forceinline__ double block_sum_ordered(double acc) {
    __shared__ double wave_sum[kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += wave_sum[w];
    return s;   // the same value in every thread
}

__global__ void k_grad_norm_partial(const float* __restrict__ g, int64_t n, int shift, double* __restrict__ partial) {
    const int64_t end = n + shift;   // the buffer is [shift, end) on the aligned grid; g points at element `shift`
    const int64_t v0 = (int64_t)blockIdx.x * kNormRun;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kNormGroups; ++k) {
        const int64_t v = v0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
        if (v >= shift && v + 4 <= end) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(g + (v - shift));
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j >= shift && v + j < end) {
                    const double d = (double)g[v + j - shift];
                    acc += d * d;
                }
        }
    }
    const double s = block_sum_ordered(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void k_grad_norm_finish(const double* __restrict__ partial, int64_t blocks, float grad_scale, float max_norm,
                                   snn_step_control* __restrict__ ctl) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < blocks; i += kThreads) acc += partial[i];
    const double sum = block_sum_ordered(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)((double)grad_scale * sqrt(sum));
        float scale = 1.0f;
        if (max_norm > 0.0f) {   // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
            scale = max_norm / (norm + 1e-6f);
            if (scale > 1.0f) scale = 1.0f;
        }
        const int finite = isfinite(sum) ? 1 : 0;   // an inf or NaN element makes the fp64 sum of squares non-finite
        ctl->norm = norm;
        ctl->scale = scale;
        ctl->finite = finite;
        ctl->skipped += 1 - finite;
    }
}

// ------------------------------------------------------------------------------------------ events
__global__ void k_events(const int32_t* __restrict__ tb, const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                         const int32_t* __restrict__ ps, int64_t n, float* __restrict__ frames, int T, int H, int W) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        int t = tb[e], x = xs[e], y = ys[e], p = ps[e];
        if (t < 0 || t >= T || y < 0 || y >= H || p < 0 || p > 1) continue;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        frames[(((int64_t)t * H + y) * W + x) * 2 + p] = 1.0f;  // idempotent store: races are benign
    }
}

// Augmented event feed: the same scatter with the binning of the raw timestamps and a per-sample flip / zoom / shift /
// random drop inside it (include/snn_hip.h states the rules).  A thread finds the sample of its event by binary search
// over the batch's offsets; offsets, window starts and the transform table sit in LDS when the batch is small.
constexpr int kAugLdsB = 64;

__device__ __forceinline__ uint32_t fmix32(uint32_t u) {
    u ^= u >> 16;
    u *= 0x85EBCA6Bu;
    u ^= u >> 13;
    u *= 0xC2B2AE35u;
    u ^= u >> 16;
    return u;
}

__global__ __launch_bounds__(kThreads) void k_events_aug(
        const int64_t* __restrict__ ts, const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
        const int32_t* __restrict__ ps, const int64_t* __restrict__ offsets, const int64_t* __restrict__ t0s,
        const int32_t* __restrict__ aug, int64_t n, float* __restrict__ frames, int T, int B, int H, int W,
        int64_t step_us, uint64_t window_us) {
    __shared__ int64_t s_off[kAugLdsB + 1];
    __shared__ int64_t s_t0[kAugLdsB];
    __shared__ int32_t s_aug[kAugLdsB * 8];
    const int64_t* off = offsets;
    const int64_t* t0 = t0s;
    const int32_t* tab = aug;
    if (B <= kAugLdsB) {  // block-uniform
        for (int i = threadIdx.x; i <= B; i += kThreads) s_off[i] = offsets[i];
        for (int i = threadIdx.x; i < B; i += kThreads) s_t0[i] = t0s[i];
        for (int i = threadIdx.x; i < B * 8; i += kThreads) s_aug[i] = aug[i];
        __syncthreads();
        off = s_off, t0 = s_t0, tab = s_aug;
    }
    const bool narrow = window_us <= 0xFFFFFFFFull;  // the quotient of an event inside the window fits 32-bit division
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        int lo = 0, hi = B;  // the last sample whose slice starts at or before e (empty samples share a start)
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (off[mid] <= e) lo = mid; else hi = mid;
        }
        const int b = lo;
        const int64_t j = e - off[b];
        if (j < 0 || e >= off[b + 1]) continue;  // an event no slice owns
        // floor((t - t0) / step) in [0, T)  <=>  0 <= t - t0 < T * step
        const int64_t d = (int64_t)((uint64_t)ts[e] - (uint64_t)t0[b]);
        if (d < 0 || (uint64_t)d >= window_us) continue;
        const int t = narrow ? (int)((uint32_t)d / (uint32_t)step_us) : (int)(d / step_us);
        int x = xs[e];
        const int y = ys[e], p = ps[e];
        if (y < 0 || y >= H || p < 0 || p > 1) continue;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        const int32_t* row = tab + b * 8;
        const uint32_t drop = (uint32_t)row[4];
        if (drop) {
            const uint32_t k = fmix32((uint32_t)row[5] + 0x9E3779B9u * (uint32_t)((uint64_t)j >> 32));
            if (fmix32((uint32_t)j ^ k) < drop) continue;
        }
        if (row[0]) x = W - 1 - x;
        const int64_t a = row[1];
        const int64_t xo = (((int64_t)(2 * x + 1) * a) >> 17) + row[2];
        const int64_t yo = (((int64_t)(2 * y + 1) * a) >> 17) + row[3];
        if (xo < 0 || xo >= W || yo < 0 || yo >= H) continue;  // outside the frame: dropped, for any table contents
        frames[((((int64_t)t * B + b) * H + yo) * W + xo) * 2 + p] = 1.0f;  // idempotent store: races are benign
    }
}

// The boxes of the same transform.  One block per sample; a row is kept when enough of it stays visible and it stays
// large enough, the kept rows move to the front of the sample in their order (ballot + block scan), -1 rows behind.
__global__ __launch_bounds__(kThreads) void k_labels_aug(const float* __restrict__ in, float* __restrict__ out,
                                                         const int32_t* __restrict__ aug, int N, int width, float Wf,
                                                         float Hf, float min_visible, float min_size_px) {
    __shared__ int s_wave[kThreads / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* row = aug + (int64_t)b * 8;
    const bool flip = row[0] != 0;
    const float s = (float)row[1] * (1.0f / 65536.0f);
    const float dx = (float)row[2] / Wf, dy = (float)row[3] / Hf;
    const float* src = in + (int64_t)b * N * width;
    float* dst = out + (int64_t)b * N * width;
    const int c0 = width - 5;  // the class column
    int kept = 0;              // rows kept by the chunks before this one (block-uniform)
    for (int base = 0; base < N; base += kThreads) {
        const int i = base + threadIdx.x;
        float v[6];
        bool keep = false;
        if (i < N) {
            for (int c = 0; c < width; ++c) v[c] = src[(int64_t)i * width + c];
            if (v[c0] >= 0.0f) {
                float x1 = v[c0 + 1], y1 = v[c0 + 2], x2 = v[c0 + 3], y2 = v[c0 + 4];
                if (flip) {
                    const float f = x1;
                    x1 = 1.0f - x2;
                    x2 = 1.0f - f;
                }
                x1 = __fadd_rn(__fmul_rn(x1, s), dx), x2 = __fadd_rn(__fmul_rn(x2, s), dx);
                y1 = __fadd_rn(__fmul_rn(y1, s), dy), y2 = __fadd_rn(__fmul_rn(y2, s), dy);
                const float a0 = (x2 - x1) * (y2 - y1);
                x1 = fminf(fmaxf(x1, 0.0f), 1.0f), x2 = fminf(fmaxf(x2, 0.0f), 1.0f);
                y1 = fminf(fmaxf(y1, 0.0f), 1.0f), y2 = fminf(fmaxf(y2, 0.0f), 1.0f);
                const float w = x2 - x1, h = y2 - y1;
                keep = w * h >= min_visible * a0 && w * Wf >= min_size_px && h * Hf >= min_size_px;
                v[c0 + 1] = x1, v[c0 + 2] = y1, v[c0 + 3] = x2, v[c0 + 4] = y2;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = kept + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) pos += s_wave[w];
            total += s_wave[w];
        }
        if (keep)  // pos <= i < N
            for (int c = 0; c < width; ++c) dst[(int64_t)pos * width + c] = v[c];
        kept += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    for (int64_t k = (int64_t)kept * width + threadIdx.x; k < (int64_t)N * width; k += kThreads) dst[k] = -1.0f;
}

// ------------------------------------------------------------------------------------------ small GEMM
// C (+)= op(A) x op(B) for weight-sized matrices (<= a few hundred per side): the three products of a composed pair of
// 1x1 convolutions (functional._ComposedConv1x1: w2 w1, G w1^T, w2^T G).  32 x 32 tile per block, 2 x 2 per thread;
// K goes through LDS in chunks of 128 whose loads are all in flight at once (these launches are latency-, not
// throughput-bound: one memory round trip per chunk instead of one per 16 k); every element is an fp32 fmaf chain in
// k order (same arithmetic as the fp32 MFMA).
constexpr int GEMM_KC = 128;
template <bool TA, bool TB>
__device__ __forceinline__ void small_gemm_tile(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                int64_t ldb, float* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                int accumulate, float* __restrict__ Ct, int64_t ldct, int m0, int n0) {
    __shared__ float As[GEMM_KC][33], Bs[GEMM_KC][33];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int k0 = 0; k0 < K; k0 += GEMM_KC) {
        float ra[GEMM_KC * 32 / kThreads], rb[GEMM_KC * 32 / kThreads];
#pragma unroll
        for (int r = 0; r < GEMM_KC * 32 / kThreads; ++r) {   // lanes run along the contiguous dimension of each operand
            const int idx = threadIdx.x + r * kThreads;
            const int ak = TA ? idx >> 5 : idx & (GEMM_KC - 1), am = TA ? idx & 31 : idx / GEMM_KC;
            const int bk = TB ? idx & (GEMM_KC - 1) : idx >> 5, bn = TB ? idx / GEMM_KC : idx & 31;
            const int m = m0 + am, n = n0 + bn;
            ra[r] = (m < M && k0 + ak < K) ? (TA ? A[(int64_t)(k0 + ak) * lda + m] : A[(int64_t)m * lda + k0 + ak]) : 0.f;
            rb[r] = (n < N && k0 + bk < K) ? (TB ? B[(int64_t)n * ldb + k0 + bk] : B[(int64_t)(k0 + bk) * ldb + n]) : 0.f;
        }
        __syncthreads();   // the previous chunk has been consumed
#pragma unroll
        for (int r = 0; r < GEMM_KC * 32 / kThreads; ++r) {
            const int idx = threadIdx.x + r * kThreads;
            const int ak = TA ? idx >> 5 : idx & (GEMM_KC - 1), am = TA ? idx & 31 : idx / GEMM_KC;
            const int bk = TB ? idx & (GEMM_KC - 1) : idx >> 5, bn = TB ? idx / GEMM_KC : idx & 31;
            As[ak][am] = ra[r];
            Bs[bk][bn] = rb[r];
        }
        __syncthreads();
        const int kend = K - k0 < GEMM_KC ? K - k0 : GEMM_KC;
        for (int kk = 0; kk < kend; ++kk)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = fmaf(As[kk][ty + 16 * i], Bs[kk][tx + 16 * j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
            if (m < M && n < N) {
                float* c = C + (int64_t)m * ldc + n;
                *c = accumulate ? *c + acc[i][j] : acc[i][j];
                if (Ct) Ct[(int64_t)n * ldct + m] = acc[i][j];   // the transposed copy (weight-sized: strided stores are fine)
            }
        }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(kThreads) void k_small_gemm(const float* __restrict__ A, int64_t lda,
                                                         const float* __restrict__ B, int64_t ldb,
                                                         float* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                         int accumulate, float* __restrict__ Ct, int64_t ldct) {
    small_gemm_tile<TA, TB>(A, lda, B, ldb, C, ldc, M, N, K, accumulate, Ct, ldct, blockIdx.y * 32, blockIdx.x * 32);
}

// n independent products C_i = A_i B_i (+ the transposed copy) in one launch: table row {A offset, B offset, C offset, Ct
// offset, M, N, K, ldct} in floats relative to base_a / base_b / base_c / base_ct; blockIdx.y = the product, blockIdx.x = its
// tile (blocks past a product's last tile leave at once).  Dense row-major operands; ldct (0 = M) lets several products
// write column blocks of ONE transposed matrix (row-stacked sibling weights).
__global__ __launch_bounds__(kThreads) void k_small_gemm_batched(const float* __restrict__ base_a,
                                                                 const float* __restrict__ base_b,
                                                                 float* __restrict__ base_c, float* __restrict__ base_ct,
                                                                 const int64_t* __restrict__ table) {
    const int64_t* row = table + (int64_t)blockIdx.y * 8;
    const int M = (int)row[4], N = (int)row[5], K = (int)row[6];
    const int64_t ldct = row[7] > 0 ? row[7] : M;
    const int tn = (N + 31) / 32, tm = (M + 31) / 32;
    if ((int)blockIdx.x >= tn * tm) return;   // whole block, before any barrier
    small_gemm_tile<false, false>(base_a + row[0], K, base_b + row[1], N, base_c + row[2], N, M, N, K, 0,
                                  base_ct ? base_ct + row[3] : nullptr, ldct, ((int)blockIdx.x / tn) * 32,
                                  ((int)blockIdx.x % tn) * 32);
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
extern "C" int snn_nchw_to_nhwc(const float* src, float* dst, int64_t N, int C, int H, int W, void* stream) {
    SNN_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "snn_nchw_to_nhwc: bad arguments");
    const int64_t HW = (int64_t)H * W;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) {
        hipError_t ce = hipMemcpyAsync(dst, src, sizeof(float) * N * HW, hipMemcpyDeviceToDevice, st);
        SNN_REQUIRE(ce == hipSuccess, "snn_nchw_to_nhwc: copy failed: %s", hipGetErrorString(ce));
    } else if (C == 2) {
        hipLaunchKernelGGL(k_nchw_to_nhwc_small<2>, dim3(grid_for(N * HW)), dim3(kThreads), 0, st, src, dst, N, HW);
    } else if (C == 3) {
        hipLaunchKernelGGL(k_nchw_to_nhwc_small<3>, dim3(grid_for(N * HW)), dim3(kThreads), 0, st, src, dst, N, HW);
    } else if (C == 4) {
        hipLaunchKernelGGL(k_nchw_to_nhwc_small<4>, dim3(grid_for(N * HW)), dim3(kThreads), 0, st, src, dst, N, HW);
    } else {
        SNN_REQUIRE(N <= 65535, "snn_nchw_to_nhwc: more than 65535 frames");
        dim3 grid((unsigned)snn_ceil_div(HW, 32), (unsigned)snn_ceil_div(C, 32), (unsigned)N);
        hipLaunchKernelGGL(k_transpose_cp, grid, dim3(32, 8), 0, st, src, dst, C, (int)HW);
    }
    SNN_CHECK_LAUNCH("snn_nchw_to_nhwc");
    return 0;
}

extern "C" int snn_nhwc_to_nchw(const float* src, float* dst, int64_t N, int C, int H, int W, void* stream) {
    SNN_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0, "snn_nhwc_to_nchw: bad arguments");
    SNN_REQUIRE(N <= 65535, "snn_nhwc_to_nchw: more than 65535 frames");
    const int64_t HW = (int64_t)H * W;
    dim3 grid((unsigned)snn_ceil_div(C, 32), (unsigned)snn_ceil_div(HW, 32), (unsigned)N);
    hipLaunchKernelGGL(k_transpose_cp, grid, dim3(32, 8), 0, (hipStream_t)stream, src, dst, (int)HW, C);
    SNN_CHECK_LAUNCH("snn_nhwc_to_nchw");
    return 0;
}

extern "C" int snn_weight_transpose(const float* w, float* wt, int Cout, int KH, int KW, int Cin, void* stream) {
    SNN_REQUIRE(w && wt && Cout > 0 && KH > 0 && KW > 0 && Cin > 0, "snn_weight_transpose: bad arguments");
    int64_t n = (int64_t)Cout * KH * KW * Cin;
    hipLaunchKernelGGL(k_weight_transpose, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, w, wt, Cout,
                       KH * KW, Cin);
    SNN_CHECK_LAUNCH("snn_weight_transpose");
    return 0;
}

extern "C" int snn_weight_transpose_batched(const float* flat_w, float* flat_wt, const int64_t* table, int n_layers,
                                            void* stream) {
    SNN_REQUIRE(flat_w && flat_wt && table && n_layers > 0 && n_layers <= 65535,
                "snn_weight_transpose_batched: bad arguments");
    hipLaunchKernelGGL(k_weight_transpose_batched, dim3(64, (unsigned)n_layers), dim3(kThreads), 0, (hipStream_t)stream,
                       flat_w, flat_wt, table);
    SNN_CHECK_LAUNCH("snn_weight_transpose_batched");
    return 0;
}

static int channels_op(bool add, const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C,
                       void* stream) {
    SNN_REQUIRE(src && dst && M > 0 && C > 0 && lds >= C && ldd >= C, "snn_%s_channels: bad arguments",
                add ? "add" : "copy");
    bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(src) && aligned16(dst);
    int64_t n = M * (v4 ? C / 4 : C);
    hipStream_t st = (hipStream_t)stream;
    if (v4 && add) hipLaunchKernelGGL((k_channels<4, true>), dim3(grid_for(n)), dim3(kThreads), 0, st, src, lds, dst, ldd, M, C);
    else if (v4) hipLaunchKernelGGL((k_channels<4, false>), dim3(grid_for(n)), dim3(kThreads), 0, st, src, lds, dst, ldd, M, C);
    else if (add) hipLaunchKernelGGL((k_channels<1, true>), dim3(grid_for(n)), dim3(kThreads), 0, st, src, lds, dst, ldd, M, C);
    else hipLaunchKernelGGL((k_channels<1, false>), dim3(grid_for(n)), dim3(kThreads), 0, st, src, lds, dst, ldd, M, C);
    SNN_CHECK_LAUNCH("snn_channels");
    return 0;
}
extern "C" int snn_copy_channels(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream) {
    return channels_op(false, src, lds, dst, ldd, M, C, stream);
}
extern "C" int snn_add_channels(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream) {
    return channels_op(true, src, lds, dst, ldd, M, C, stream);
}

extern "C" int snn_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* dst, int64_t ldd, int64_t M,
                       int C, void* stream) {
    SNN_REQUIRE(a && b && dst && M > 0 && C > 0 && lda >= C && ldb >= C && ldd >= C, "snn_add: bad arguments");
    bool v4 = C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldd % 4 == 0 && aligned16(a) && aligned16(b) &&
              aligned16(dst);
    if (v4) hipLaunchKernelGGL(k_add<4>, dim3(grid_for(M * (C / 4))), dim3(kThreads), 0, (hipStream_t)stream, a, lda,
                               b, ldb, dst, ldd, M, C);
    else hipLaunchKernelGGL(k_add<1>, dim3(grid_for(M * C)), dim3(kThreads), 0, (hipStream_t)stream, a, lda, b, ldb,
                            dst, ldd, M, C);
    SNN_CHECK_LAUNCH("snn_add");
    return 0;
}

static bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

extern "C" int snn_copy_channels_bf16(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream) {
    SNN_REQUIRE(src && dst && M > 0 && C > 0 && lds >= C && ldd >= C, "snn_copy_channels_bf16: bad arguments");
    const bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned8(src) && aligned8(dst);
    if (v4) hipLaunchKernelGGL((k_merge_bf16<4, 0>), dim3(grid_for(M * (C / 4))), dim3(kThreads), 0, (hipStream_t)stream, src,
                               lds, nullptr, 0, dst, ldd, M, C);
    else hipLaunchKernelGGL((k_merge_bf16<1, 0>), dim3(grid_for(M * C)), dim3(kThreads), 0, (hipStream_t)stream, src, lds,
                            nullptr, 0, dst, ldd, M, C);
    SNN_CHECK_LAUNCH("snn_copy_channels_bf16");
    return 0;
}

extern "C" int snn_add_bf16(const float* a, int64_t lda, const float* b, int64_t ldb, float* dst, int64_t ldd, int64_t M,
                            int C, void* stream) {
    SNN_REQUIRE(a && b && dst && M > 0 && C > 0 && lda >= C && ldb >= C && ldd >= C, "snn_add_bf16: bad arguments");
    const bool v4 = C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldd % 4 == 0 && aligned8(a) && aligned8(b) && aligned8(dst);
    if (v4) hipLaunchKernelGGL((k_merge_bf16<4, 1>), dim3(grid_for(M * (C / 4))), dim3(kThreads), 0, (hipStream_t)stream, a,
                               lda, b, ldb, dst, ldd, M, C);
    else hipLaunchKernelGGL((k_merge_bf16<1, 1>), dim3(grid_for(M * C)), dim3(kThreads), 0, (hipStream_t)stream, a, lda, b,
                            ldb, dst, ldd, M, C);
    SNN_CHECK_LAUNCH("snn_add_bf16");
    return 0;
}

extern "C" int snn_convert_bf16(const void* src, void* dst, int64_t n, int to_bf16, void* stream) {
    SNN_REQUIRE(src && dst && n > 0, "snn_convert_bf16: bad arguments");
    if (to_bf16) hipLaunchKernelGGL(k_convert_bf16<true>, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, src, dst, n);
    else hipLaunchKernelGGL(k_convert_bf16<false>, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, src, dst, n);
    SNN_CHECK_LAUNCH("snn_convert_bf16");
    return 0;
}

extern "C" int snn_act_fwd(int act, const float* x, float* y, int64_t n, void* stream) {
    SNN_REQUIRE(x && y && n > 0 && act >= SNN_ACT_RELU && act <= SNN_ACT_TANH, "snn_act_fwd: bad arguments");
    hipLaunchKernelGGL(k_act_fwd, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, act, x, y, n);
    SNN_CHECK_LAUNCH("snn_act_fwd");
    return 0;
}
extern "C" int snn_act_bwd(int act, const float* x, const float* y, const float* gy, float* gx, int64_t n,
                           void* stream) {
    SNN_REQUIRE(x && y && gy && gx && n > 0 && act >= SNN_ACT_RELU && act <= SNN_ACT_TANH, "snn_act_bwd: bad arguments");
    hipLaunchKernelGGL(k_act_bwd, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, act, x, y, gy, gx, n);
    SNN_CHECK_LAUNCH("snn_act_bwd");
    return 0;
}

extern "C" int snn_small_gemm(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                              int64_t ldc, int M, int N, int K, int accumulate, float* Ct, int64_t ldct, void* stream) {
    SNN_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "snn_small_gemm: bad arguments");
    SNN_REQUIRE(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N, "snn_small_gemm: leading dimension "
                "smaller than the row length");
    SNN_REQUIRE(!Ct || (ldct >= M && !accumulate), "snn_small_gemm: the transposed copy needs ldct >= M and accumulate == 0");
    dim3 grid((unsigned)snn_ceil_div(N, 32), (unsigned)snn_ceil_div(M, 32));
    hipStream_t st = (hipStream_t)stream;
    if (transA && transB) hipLaunchKernelGGL((k_small_gemm<true, true>), grid, dim3(kThreads), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, Ct, ldct);
    else if (transA) hipLaunchKernelGGL((k_small_gemm<true, false>), grid, dim3(kThreads), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, Ct, ldct);
    else if (transB) hipLaunchKernelGGL((k_small_gemm<false, true>), grid, dim3(kThreads), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, Ct, ldct);
    else hipLaunchKernelGGL((k_small_gemm<false, false>), grid, dim3(kThreads), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, Ct, ldct);
    SNN_CHECK_LAUNCH("snn_small_gemm");
    return 0;
}

extern "C" int snn_small_gemm_batched(const float* base_a, const float* base_b, float* base_c, float* base_ct,
                                      const int64_t* table, int n, int max_tiles, void* stream) {
    SNN_REQUIRE(base_a && base_b && base_c && table && n > 0 && n <= 65535 && max_tiles > 0,
                "snn_small_gemm_batched: bad arguments");
    hipLaunchKernelGGL(k_small_gemm_batched, dim3((unsigned)max_tiles, (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream,
                       base_a, base_b, base_c, base_ct, table);
    SNN_CHECK_LAUNCH("snn_small_gemm_batched");
    return 0;
}

extern "C" int snn_lstm_cell_fwd(const float* gates, const float* c_prev, float* h, float* c, int64_t M, int C,
                                 void* stream) {
    SNN_REQUIRE(gates && h && c && M > 0 && C > 0, "snn_lstm_cell_fwd: bad arguments");
    hipLaunchKernelGGL(k_lstm_fwd, dim3(grid_for(M * C)), dim3(kThreads), 0, (hipStream_t)stream, gates, c_prev, h, c,
                       M, C);
    SNN_CHECK_LAUNCH("snn_lstm_cell_fwd");
    return 0;
}
extern "C" int snn_lstm_cell_bwd(const float* gates, const float* c_prev, const float* c, const float* gh,
                                 const float* gc, float* g_gates, float* g_c_prev, int64_t M, int C, void* stream) {
    SNN_REQUIRE(gates && c && g_gates && M > 0 && C > 0, "snn_lstm_cell_bwd: bad arguments");
    hipLaunchKernelGGL(k_lstm_bwd, dim3(grid_for(M * C)), dim3(kThreads), 0, (hipStream_t)stream, gates, c_prev, c,
                       gh, gc, g_gates, g_c_prev, M, C);
    SNN_CHECK_LAUNCH("snn_lstm_cell_bwd");
    return 0;
}

extern "C" int snn_pool_fwd(int kind, const float* x, float* y, int64_t N, int H, int W, int C, int Ho, int Wo, int k,
                            int stride, void* stream) {
    SNN_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0, "snn_pool_fwd: bad arguments");
    SNN_REQUIRE(kind >= SNN_POOL_AVG && kind <= SNN_POOL_SUM, "snn_pool_fwd: bad pool kind %d", kind);
    SNN_REQUIRE(Ho == (H - k) / stride + 1 && Wo == (W - k) / stride + 1 && Ho > 0 && Wo > 0,
                "snn_pool_fwd: output size mismatch");
    hipLaunchKernelGGL(k_pool_fwd, dim3(grid_for(N * Ho * Wo * C)), dim3(kThreads), 0, (hipStream_t)stream, kind, x, y,
                       N, H, W, C, Ho, Wo, k, stride);
    SNN_CHECK_LAUNCH("snn_pool_fwd");
    return 0;
}
extern "C" int snn_pool_bwd(int kind, const float* x, const float* gy, float* gx, int64_t N, int H, int W, int C,
                            int Ho, int Wo, int k, int stride, void* stream) {
    SNN_REQUIRE(gy && gx && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0, "snn_pool_bwd: bad arguments");
    SNN_REQUIRE(kind >= SNN_POOL_AVG && kind <= SNN_POOL_SUM, "snn_pool_bwd: bad pool kind %d", kind);
    SNN_REQUIRE(kind != SNN_POOL_MAX || x, "snn_pool_bwd: max pooling needs the forward input");
    hipLaunchKernelGGL(k_pool_bwd, dim3(grid_for(N * H * W * C)), dim3(kThreads), 0, (hipStream_t)stream, kind, x, gy,
                       gx, N, H, W, C, Ho, Wo, k, stride);
    SNN_CHECK_LAUNCH("snn_pool_bwd");
    return 0;
}

extern "C" int snn_upsample_fwd(const float* x, float* y, int64_t N, int H, int W, int C, int scale, void* stream) {
    SNN_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && scale > 0, "snn_upsample_fwd: bad arguments");
    hipLaunchKernelGGL(k_upsample_fwd, dim3(grid_for(N * H * scale * W * scale * C)), dim3(kThreads), 0,
                       (hipStream_t)stream, x, y, N, H, W, C, scale);
    SNN_CHECK_LAUNCH("snn_upsample_fwd");
    return 0;
}
extern "C" int snn_upsample_bwd(const float* gy, float* gx, int64_t N, int H, int W, int C, int scale, void* stream) {
    SNN_REQUIRE(gy && gx && N > 0 && H > 0 && W > 0 && C > 0 && scale > 0, "snn_upsample_bwd: bad arguments");
    hipLaunchKernelGGL(k_upsample_bwd, dim3(grid_for(N * H * W * C)), dim3(kThreads), 0, (hipStream_t)stream, gy, gx, N,
                       H, W, C, scale);
    SNN_CHECK_LAUNCH("snn_upsample_bwd");
    return 0;
}

extern "C" int snn_adamax_step(float* param, const float* grad, float* exp_avg, float* exp_inf, int64_t n, float lr,
                               float beta1, float beta2, float eps, int step, float grad_scale, void* stream) {
    SNN_REQUIRE(param && grad && exp_avg && exp_inf && n > 0 && step >= 1, "snn_adamax_step: bad arguments");
    // clr = lr / (1 - beta1^step)
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    hipLaunchKernelGGL(k_adamax, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_inf, n, w1, beta2, eps, clr, grad_scale);
    SNN_CHECK_LAUNCH("snn_adamax_step");
    return 0;
}

extern "C" int snn_adamax_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_inf, int64_t n, float lr,
                                   float beta1, float beta2, float eps, int step, float grad_scale, float weight_decay,
                                   float clip_value, const snn_step_control* ctl, void* stream) {
    SNN_REQUIRE(param && grad && exp_avg && exp_inf && n > 0 && step >= 1, "snn_adamax_step_ctl: bad arguments");
    SNN_REQUIRE(weight_decay >= 0.0f, "snn_adamax_step_ctl: negative weight_decay");   // (false for a NaN too)
    SNN_REQUIRE(aligned(4, {ctl}), "snn_adamax_step_ctl: the control record must be 4-byte aligned");
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    if (!ctl && weight_decay == 0.0f && !(clip_value > 0.0f))   // nothing to add: the plain kernel, the same bits
        hipLaunchKernelGGL(k_adamax, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_inf, n, w1, beta2, eps, clr, grad_scale);
    else
        hipLaunchKernelGGL(k_adamax_ctl, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_inf, n, w1, beta2, eps, clr, grad_scale, weight_decay, clip_value, ctl);
    SNN_CHECK_LAUNCH("snn_adamax_step_ctl");
    return 0;
}

// ema_weight = 1 - decay in (0, 1] (false for a NaN): 0 would never move the average, above 1 it would overshoot
static bool ema_weight_ok(float w) { return w > 0.0f && w <= 1.0f; }

extern "C" int snn_adamax_step_ema(float* param, const float* grad, float* exp_avg, float* exp_inf, float* ema, int64_t n,
                                   float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                                   float weight_decay, float clip_value, float ema_weight, const snn_step_control* ctl,
                                   void* stream) {
    SNN_REQUIRE(param, "snn_adamax_step_ema: param is NULL");
    SNN_REQUIRE(grad, "snn_adamax_step_ema: grad is NULL");
    SNN_REQUIRE(exp_avg, "snn_adamax_step_ema: exp_avg is NULL");
    SNN_REQUIRE(exp_inf, "snn_adamax_step_ema: exp_inf is NULL");
    SNN_REQUIRE(ema, "snn_adamax_step_ema: ema is NULL");
    SNN_REQUIRE(n > 0, "snn_adamax_step_ema: n = %lld must be positive", (long long)n);
    SNN_REQUIRE(step >= 1, "snn_adamax_step_ema: step = %d must be at least 1", step);
    SNN_REQUIRE(weight_decay >= 0.0f, "snn_adamax_step_ema: negative weight_decay");   // (false for a NaN too)
    SNN_REQUIRE(ema_weight_ok(ema_weight), "snn_adamax_step_ema: ema_weight = %g is outside (0, 1]", (double)ema_weight);
    SNN_REQUIRE(aligned(4, {ctl}), "snn_adamax_step_ema: the control record must be 4-byte aligned");
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    if (!ctl && weight_decay == 0.0f && !(clip_value > 0.0f))   // where snn_adamax_step_ctl launches the plain kernel
        hipLaunchKernelGGL(k_adamax_ema<false>, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad,
                           exp_avg, exp_inf, ema, n, w1, beta2, eps, clr, grad_scale, 0.0f, 0.0f, ema_weight, nullptr);
    else
        hipLaunchKernelGGL(k_adamax_ema<true>, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad,
                           exp_avg, exp_inf, ema, n, w1, beta2, eps, clr, grad_scale, weight_decay, clip_value, ema_weight,
                           ctl);
    SNN_CHECK_LAUNCH("snn_adamax_step_ema");
    return 0;
}

extern "C" int snn_ema_update(float* ema, const float* src, int64_t n, float ema_weight, const snn_step_control* ctl,
                              void* stream) {
    SNN_REQUIRE(ema, "snn_ema_update: ema is NULL");
    SNN_REQUIRE(src, "snn_ema_update: src is NULL");
    SNN_REQUIRE(n > 0, "snn_ema_update: n = %lld must be positive", (long long)n);
    SNN_REQUIRE(ema_weight_ok(ema_weight), "snn_ema_update: ema_weight = %g is outside (0, 1]", (double)ema_weight);
    SNN_REQUIRE(aligned(4, {ctl}), "snn_ema_update: the control record must be 4-byte aligned");
    hipLaunchKernelGGL(k_ema_update, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, ema, src, n, ema_weight,
                       ctl);
    SNN_CHECK_LAUNCH("snn_ema_update");
    return 0;
}

static int64_t grad_norm_blocks(int64_t n, int shift) { return snn_ceil_div(n + shift, kNormRun); }

extern "C" size_t snn_grad_norm_workspace_size(int64_t n) {
    return n > 0 ? (size_t)grad_norm_blocks(n, 3) * sizeof(double) : 0;   // (3: the largest shift of an unaligned base)
}

extern "C" int snn_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, void* ws,
                             snn_step_control* ctl, void* stream) {
    SNN_REQUIRE(grad && ws && ctl && n > 0, "snn_grad_norm: bad arguments");
    SNN_REQUIRE(aligned(4, {grad, ctl}) && aligned(8, {ws}),
                "snn_grad_norm: grad and ctl must be 4-byte aligned, the workspace 8-byte aligned");
    const int shift = (int)((reinterpret_cast<uintptr_t>(grad) & 15u) / 4);
    const int64_t blocks = grad_norm_blocks(n, shift);
    SNN_REQUIRE(blocks <= 0x7fffffff, "snn_grad_norm: %lld elements are more than one launch covers", (long long)n);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_grad_norm_partial, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, grad, n, shift,
                       partial);
    SNN_CHECK_LAUNCH("snn_grad_norm");
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partial, blocks, grad_scale,
                       max_norm, ctl);
    SNN_CHECK_LAUNCH("snn_grad_norm");
    return 0;
}

extern "C" int snn_events_to_frames(const int32_t* t_bin, const int32_t* x, const int32_t* y, const int32_t* p,
                                    int64_t n_events, float* frames, int T, int H, int W, void* stream) {
    SNN_REQUIRE(frames && T > 0 && H > 0 && W > 0 && n_events >= 0, "snn_events_to_frames: bad arguments");
    hipError_t me = hipMemsetAsync(frames, 0, sizeof(float) * (size_t)T * H * W * 2, (hipStream_t)stream);
    SNN_REQUIRE(me == hipSuccess, "snn_events_to_frames: memset failed: %s", hipGetErrorString(me));
    if (n_events == 0) return 0;
    SNN_REQUIRE(t_bin && x && y && p, "snn_events_to_frames: null event arrays");
    hipLaunchKernelGGL(k_events, dim3(grid_for(n_events)), dim3(kThreads), 0, (hipStream_t)stream, t_bin, x, y, p,
                       n_events, frames, T, H, W);
    SNN_CHECK_LAUNCH("snn_events_to_frames");
    return 0;
}

extern "C" int snn_events_to_frames_aug(const int64_t* t_us, const int32_t* x, const int32_t* y, const int32_t* p,
                                        const int64_t* offsets, const int64_t* t0, const int32_t* aug,
                                        int64_t n_events, float* frames, int T, int B, int H, int W, int64_t step_us,
                                        void* stream) {
    SNN_REQUIRE(frames && offsets && t0 && aug, "snn_events_to_frames_aug: null pointer");
    SNN_REQUIRE(T > 0 && B > 0 && H > 0 && W > 0 && n_events >= 0, "snn_events_to_frames_aug: bad shape");
    SNN_REQUIRE(step_us > 0, "snn_events_to_frames_aug: step_us must be positive, got %lld", (long long)step_us);
    SNN_REQUIRE(step_us <= INT64_MAX / T, "snn_events_to_frames_aug: T * step_us overflows 64 bits");
    // 2 T B H W < 2^31, asked without forming a product that could overflow
    SNN_REQUIRE((int64_t)T * B <= ((1ll << 30) - 1) / ((int64_t)H * W),
                "snn_events_to_frames_aug: a frame buffer of 2^31 elements or more");
    SNN_REQUIRE(n_events == 0 || (t_us && x && y && p), "snn_events_to_frames_aug: null event arrays");
    const int64_t cells = (int64_t)T * B * H * W;
    hipError_t me = hipMemsetAsync(frames, 0, sizeof(float) * (size_t)cells * 2, (hipStream_t)stream);
    SNN_REQUIRE(me == hipSuccess, "snn_events_to_frames_aug: memset failed: %s", hipGetErrorString(me));
    if (n_events == 0) return 0;
    hipLaunchKernelGGL(k_events_aug, dim3(grid_for(n_events)), dim3(kThreads), 0, (hipStream_t)stream, t_us, x, y, p,
                       offsets, t0, aug, n_events, frames, T, B, H, W, step_us, (uint64_t)(step_us * T));
    SNN_CHECK_LAUNCH("snn_events_to_frames_aug");
    return 0;
}

extern "C" int snn_labels_augment(const float* labels_in, float* labels_out, const int32_t* aug, int B, int N, int width,
                                  int W, int H, float min_visible, float min_size_px, void* stream) {
    SNN_REQUIRE(B > 0 && N >= 0 && W > 0 && H > 0, "snn_labels_augment: bad shape");
    SNN_REQUIRE(width == 5 || width == 6, "snn_labels_augment: rows of %d columns (5 or 6)", width);
    if (N == 0) return 0;
    SNN_REQUIRE(labels_in && labels_out && aug, "snn_labels_augment: null pointer");
    SNN_REQUIRE(labels_in != labels_out, "snn_labels_augment: in place is not supported");
    hipLaunchKernelGGL(k_labels_aug, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, labels_in, labels_out, aug, N,
                       width, (float)W, (float)H, min_visible, min_size_px);
    SNN_CHECK_LAUNCH("snn_labels_augment");
    return 0;
}
