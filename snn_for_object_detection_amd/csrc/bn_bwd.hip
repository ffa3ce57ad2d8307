// BatchNorm backward behind the reverse Norm -> neuron scan (gfx950): the scan's per-block partial sums -> raw sums ->
// coefficients and parameter gradients, and the apply pass dy = A*gx + B*y + C.
#include "scan_common.h"

namespace {

// reduce block partials -> raw[t][c] = (sum gx, sum gx*y).  32 lanes per (t,c): lane k sums blocks k, k+32, ...
// then a fixed xor tree combines the lanes.  `raw` must not alias the partial buffer (fp32 partials, fp64 result).
// from_state (the scan ran with SNN_SCAN_SUMS_FROM_STATE): the second partial is sum(gx * x); raw still receives sum(gx * y)
// = mean * sum(gx) + (sum(gx * x) - bias * sum(gx)) / (gamma * invstd) - what the all-reduce and k_bn_bwd_coef expect - and
// the sum itself, from gx and y, for a channel whose gamma is exactly 0 (see k_bn_bwd_finalize_fused).
__device__ __forceinline__ double sum_gx_y_from_state(double s1, double p, double mu, double is, double gam, double bnb) {
    return mu * s1 + (p - bnb * s1) / (gam * is);
}

__global__ __launch_bounds__(256) void k_bn_bwd_reduce(const double* __restrict__ sums_, int gx_blocks, int T, int C,
                                                       double* __restrict__ raw, int from_state, int64_t M,
                                                       const float* __restrict__ gamma, const float* __restrict__ bn_bias,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gx, const float* __restrict__ y,
                                                       int64_t ldy) {
    const float* __restrict__ sums = reinterpret_cast<const float*>(sums_);
    const int sub = threadIdx.x & 31;
    const int idx = blockIdx.x * (blockDim.x / 32) + (threadIdx.x >> 5);
    const bool live = idx < T * C;
    const int c = live ? idx % C : 0, t = live ? idx / C : 0;
    const double gam = (double)((from_state && gamma) ? gamma[c] : 1.0f);
    const bool direct = from_state && gam == 0.0;   // uniform over the 32 lanes of an (t, c)
    double s1 = 0.0, sy = 0.0;
    if (live) {
        for (int b = sub; b < gx_blocks; b += 32) {
            const float2 v = *reinterpret_cast<const float2*>(sums + ((int64_t)b * T * C + idx) * 2);
            s1 += (double)v.x;
            sy += (double)v.y;
        }
        if (direct) {
            sy = 0.0;
            for (int64_t m = sub; m < M; m += 32)
                sy += (double)gx[((int64_t)t * M + m) * C + c] * (double)y[((int64_t)t * M + m) * ldy + c];
        }
    }
    for (int stride = 16; stride >= 1; stride >>= 1) {
        s1 += __shfl_xor(s1, stride, 64);
        sy += __shfl_xor(sy, stride, 64);
    }
    if (!live || sub != 0) return;
    if (from_state && !direct)
        sy = sum_gx_y_from_state(s1, sy, (double)mean[idx], (double)invstd[idx], gam, (double)(bn_bias ? bn_bias[c] : 0.0f));
    raw[(int64_t)idx * 2 + 0] = s1;
    raw[(int64_t)idx * 2 + 1] = sy;
}

// raw sums over M pixels (all-reduced over the ranks under SyncBatchNorm) -> backward coefficients;
// raw_local (this rank's sums) -> (sum gx, sum gx*xhat) for the parameter gradients, written to `param_sums`
__global__ void k_bn_bwd_coef(const double* __restrict__ raw, const double* __restrict__ raw_local, int T, int64_t M,
                              int C, const float* __restrict__ gamma, const float* __restrict__ mean,
                              const float* __restrict__ invstd, float* __restrict__ coefA, float* __restrict__ coefB,
                              float* __restrict__ coefC, double* __restrict__ param_sums) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * C) return;
    const int c = idx % C;
    const double mu = (double)mean[idx], is = (double)invstd[idx];
    const double s1 = raw[(int64_t)idx * 2 + 0], sy = raw[(int64_t)idx * 2 + 1];
    const double l1 = raw_local[(int64_t)idx * 2 + 0], ly = raw_local[(int64_t)idx * 2 + 1];
    const double s2 = is * (sy - mu * s1);  // sum gx * xhat
    const double n = (double)M;
    const double a = (double)(gamma ? gamma[c] : 1.0f) * is;
    const double m1 = s1 / n, m2 = s2 / n;
    coefA[idx] = (float)a;
    coefB[idx] = (float)(-a * is * m2);
    coefC[idx] = (float)(-a * m1 + a * is * mu * m2);
    param_sums[(int64_t)idx * 2 + 0] = l1;
    param_sums[(int64_t)idx * 2 + 1] = is * (ly - mu * l1);
}

__global__ void k_bn_bwd_params(const double* __restrict__ sums, int T, int C, float* __restrict__ dgamma,
                                float* __restrict__ dbias, int accumulate) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double dg = 0.0, db = 0.0;
    for (int t = 0; t < T; ++t) {
        db += sums[((int64_t)t * C + c) * 2 + 0];
        dg += sums[((int64_t)t * C + c) * 2 + 1];
    }
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)dg : (float)dg;
    if (dbias) dbias[c] = accumulate ? dbias[c] + (float)db : (float)db;
}

// One launch for the BatchNorm-backward second phase of a layer (was: reduce + coefficients + parameter gradients).
// One block per channel; 32 lanes share the block partials of one (t, c) (lane k sums blocks k, k+32, ... in order,
// then a fixed xor tree), 32 timesteps per pass (1024 threads); thread 0 adds the per-timestep parameter sums in t order.
__global__ __launch_bounds__(1024) void k_bn_bwd_finalize_fused(
    const double* __restrict__ sums_, int gx_blocks, int T, int64_t M, int C, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ coefA,
    float* __restrict__ coefB, float* __restrict__ coefC, float* __restrict__ dgamma, float* __restrict__ dbias,
    int accumulate, int from_state, const float* __restrict__ bn_bias, const float* __restrict__ gx,
    const float* __restrict__ y, int64_t ldy) {
    // from_state (the scan ran with SNN_SCAN_SUMS_FROM_STATE): the second partial is sum(gx * x), x = gamma*xhat + bias the
    // neuron's input, so sum(gx * xhat) = (sum(gx * x) - bias * sum(gx)) / gamma.  A channel whose gamma is exactly 0 carries
    // no xhat in x: for it (and only for it) the sum is formed here from gx and y - slow, one block per such channel.
    const float* __restrict__ sums = reinterpret_cast<const float*>(sums_);  // fp32 block partials
    __shared__ double sm_b[32], sm_g[32];
    const int c = blockIdx.x;
    const int sub = threadIdx.x & 31, tl = threadIdx.x >> 5;
    double dg = 0.0, db = 0.0;
    const double gam = (double)(gamma ? gamma[c] : 1.0f);
    const double bnb = (double)((from_state && bn_bias) ? bn_bias[c] : 0.0f);
    const bool direct = from_state && gam == 0.0;
    for (int tb = 0; tb < T; tb += 32) {
        const int t = tb + tl;
        const int idx = t * C + c;
        double s1 = 0.0, sy = 0.0;
        if (t < T) {
#pragma unroll 4
            for (int bk = sub; bk < gx_blocks; bk += 32) {
                const float2 v = *reinterpret_cast<const float2*>(sums + ((int64_t)bk * T * C + idx) * 2);
                s1 += (double)v.x;
                sy += (double)v.y;
            }
        }
        if (direct) {   // uniform over the block
            sy = 0.0;
            if (t < T) {
                for (int64_t m = sub; m < M; m += 32)
                    sy += (double)gx[((int64_t)t * M + m) * C + c] * (double)y[((int64_t)t * M + m) * ldy + c];
            }
        }
        for (int stride = 16; stride >= 1; stride >>= 1) {
            s1 += __shfl_xor(s1, stride, 64);
            sy += __shfl_xor(sy, stride, 64);
        }
        if (sub == 0 && t < T) {
            const double mu = (double)mean[idx], is = (double)invstd[idx];
            if (from_state && !direct) sy = sum_gx_y_from_state(s1, sy, mu, is, gam, bnb);   // (as k_bn_bwd_reduce: same bits)
            const double s2 = is * (sy - mu * s1);  // sum gx * xhat
            const double n = (double)M;
            const double a = gam * is;
            const double m1 = s1 / n, m2 = s2 / n;
            coefA[idx] = (float)a;
            coefB[idx] = (float)(-a * is * m2);
            coefC[idx] = (float)(-a * m1 + a * is * mu * m2);
            sm_b[tl] = s1;
            sm_g[tl] = s2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nt = T - tb < 32 ? T - tb : 32;
            for (int k = 0; k < nt; ++k) {
                db += sm_b[k];
                dg += sm_g[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)dg : (float)dg;
        if (dbias) dbias[c] = accumulate ? dbias[c] + (float)db : (float)db;
    }
}

template <int VEC, bool SB = false>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_apply(const float* __restrict__ gx, const float* __restrict__ y,
                                                           int64_t ldy, const float* __restrict__ coefA,
                                                           const float* __restrict__ coefB,
                                                           const float* __restrict__ coefC, float* __restrict__ dy,
                                                           int64_t lddy, int T, int64_t M, int C, int accumulate) {
    typedef typename Vec<VEC>::type V;
    const int cv = C / VEC;
    const int64_t total = (int64_t)T * M * cv;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t row = e / cv;
        const int c = (int)(e % cv) * VEC;
        const int64_t t = row / M;
        V g = VecS<VEC, SB>::load_last(gx, row * C + c);      // last reads of both: dy is what the next kernels want cached
        V yv = VecS<VEC, SB>::load_last(y, row * ldy + c);
        V a = Vec<VEC>::load(coefA + t * C + c);
        V b = Vec<VEC>::load(coefB + t * C + c);
        V k = Vec<VEC>::load(coefC + t * C + c);
        V r;
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            lane<VEC>(r, j) = lane<VEC>(a, j) * lane<VEC>(g, j) + lane<VEC>(b, j) * lane<VEC>(yv, j) + lane<VEC>(k, j);
        if (accumulate) {
            V old = VecS<VEC, SB>::load(dy, row * lddy + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) lane<VEC>(r, j) += lane<VEC>(old, j);
        }
        VecS<VEC, SB>::store(dy, row * lddy + c, r);
    }
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
// block partials of the reverse scan -> raw (sum gx, sum gx*y) per (t, c); from_state: the scan ran with
// SNN_SCAN_SUMS_FROM_STATE and its second partial is sum(gx * x)
static int bn_bwd_reduce(const char* name, int from_state, const double* sums, int T, int64_t M, int C, const float* gamma,
                         const float* bias, const float* mean, const float* invstd, const float* gx, const float* y,
                         int64_t ldy, double* raw, void* stream) {
    SNN_REQUIRE(sums != raw, "%s: raw must not alias the partial sums", name);
    BwdPlan pl = bwd_plan(T, M, C, true);
    int n = T * C;
    hipLaunchKernelGGL(k_bn_bwd_reduce, dim3((n + 7) / 8), dim3(256), 0, (hipStream_t)stream, sums, pl.gx, T, C, raw,
                       from_state, M, gamma, bias, mean, invstd, gx, y, ldy);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_bn_bwd_reduce(const double* sums, int T, int64_t M, int C, double* raw, void* stream) {
    SNN_REQUIRE(sums && raw && T > 0 && M > 0 && C > 0, "snn_bn_bwd_reduce: bad arguments");
    return bn_bwd_reduce("snn_bn_bwd_reduce", 0, sums, T, M, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, raw,
                         stream);
}

extern "C" int snn_bn_bwd_reduce_from_state(const double* sums, int T, int64_t M, int C, const float* gamma, const float* bias,
                                            const float* mean, const float* invstd, const float* gx, const float* y,
                                            int64_t ldy, double* raw, void* stream) {
    SNN_REQUIRE(sums && raw && mean && invstd && gx && y && T > 0 && M > 0 && C > 0 && ldy >= C,
                "snn_bn_bwd_reduce_from_state: bad arguments");
    return bn_bwd_reduce("snn_bn_bwd_reduce_from_state", 1, sums, T, M, C, gamma, bias, mean, invstd, gx, y, ldy, raw, stream);
}

extern "C" int snn_bn_bwd_coef(const double* raw, const double* raw_local, double* param_sums, int T, int64_t M_total,
                               int C, const float* gamma, const float* mean, const float* invstd, float* coefA,
                               float* coefB, float* coefC, float* dgamma, float* dbias, int accumulate,
                               void* stream) {
    SNN_REQUIRE(raw && raw_local && param_sums && mean && invstd && coefA && coefB && coefC,
                "snn_bn_bwd_coef: null pointer");
    SNN_REQUIRE(T > 0 && M_total > 0 && C > 0, "snn_bn_bwd_coef: bad shape");
    int n = T * C;
    hipLaunchKernelGGL(k_bn_bwd_coef, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw, raw_local, T,
                       M_total, C, gamma, mean, invstd, coefA, coefB, coefC, param_sums);
    SNN_CHECK_LAUNCH("snn_bn_bwd_coef");
    if (dgamma || dbias) {
        hipLaunchKernelGGL(k_bn_bwd_params, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, param_sums, T, C,
                           dgamma, dbias, accumulate);
        SNN_CHECK_LAUNCH("snn_bn_bwd_params");
    }
    return 0;
}

// single-process form: reduce the block partials in place, then coefficients and parameter gradients; from_state: sums
// written by a scan that ran with SNN_SCAN_SUMS_FROM_STATE (second partial: sum(gx * x), see the kernel)
static int bn_bwd_finalize(const char* name, int from_state, double* sums, int T, int64_t M, int C, const float* gamma,
                           const float* bias, const float* mean, const float* invstd, const float* gx, const float* y,
                           int64_t ldy, float* coefA, float* coefB, float* coefC, float* dgamma, float* dbias,
                           int accumulate, void* stream) {
    SNN_REQUIRE(sums && mean && invstd && coefA && coefB && coefC && (!from_state || (gx && y)), "%s: null pointer", name);
    SNN_REQUIRE(T > 0 && M > 0 && C > 0 && (!from_state || ldy >= C), "%s: bad shape", name);
    BwdPlan pl = bwd_plan(T, M, C, true);
    hipLaunchKernelGGL(k_bn_bwd_finalize_fused, dim3(C), dim3(1024), 0, (hipStream_t)stream, sums, pl.gx, T, M, C, gamma,
                       mean, invstd, coefA, coefB, coefC, dgamma, dbias, accumulate, from_state, bias, gx, y, ldy);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_bn_bwd_finalize(double* sums, int T, int64_t M, int C, const float* gamma, const float* mean,
                                   const float* invstd, float* coefA, float* coefB, float* coefC, float* dgamma,
                                   float* dbias, int accumulate, void* stream) {
    return bn_bwd_finalize("snn_bn_bwd_finalize", 0, sums, T, M, C, gamma, nullptr, mean, invstd, nullptr, nullptr, 0, coefA,
                           coefB, coefC, dgamma, dbias, accumulate, stream);
}

extern "C" int snn_bn_bwd_finalize_from_state(double* sums, int T, int64_t M, int C, const float* gamma, const float* bias,
                                              const float* mean, const float* invstd, const float* gx, const float* y,
                                              int64_t ldy, float* coefA, float* coefB, float* coefC, float* dgamma,
                                              float* dbias, int accumulate, void* stream) {
    return bn_bwd_finalize("snn_bn_bwd_finalize_from_state", 1, sums, T, M, C, gamma, bias, mean, invstd, gx, y, ldy, coefA,
                           coefB, coefC, dgamma, dbias, accumulate, stream);
}

// dy = A*gx + B*y + C per (t, c); sb: gx, y and dy are bf16 tensors
static int bn_bwd_apply(const char* name, bool sb, const float* gx, const float* y, int64_t ldy, const float* coefA,
                        const float* coefB, const float* coefC, float* dy, int64_t lddy, int T, int64_t M, int C,
                        int accumulate, void* stream) {
    SNN_REQUIRE(gx && y && coefA && coefB && coefC && dy, "%s: null pointer", name);
    SNN_REQUIRE(T > 0 && M > 0 && C > 0 && ldy >= C && lddy >= C, "%s: bad shape", name);
    const int vec = (multiples(4, {C, ldy, lddy}) && aligned(sb ? 8 : 16, {gx, y, dy}) && aligned(16, {coefA, coefB, coefC}))
                        ? 4
                        : 1;
    SNN_REQUIRE(!sb || vec == 4, "%s: bad shape (C and strides multiples of 4, bf16 tensors 8-byte aligned)", name);
    int64_t total = (int64_t)T * M * (C / vec);
    int64_t blocks = snn_ceil_div(total, kThreads);
    if (blocks > snn_max_blocks()) blocks = snn_max_blocks();
    if (const char* force = snn_tuning_env("SNN_APPLY_CAP")) {   // tuning aid: blocks per launch of the apply pass
        if (atoi(force) > 0 && blocks > atoi(force)) blocks = atoi(force);
    }
    dispatch(
        [&](auto VEC, auto SB) {
            if constexpr (VEC() == 4 || !SB()) {
                hipLaunchKernelGGL((k_bn_bwd_apply<VEC(), SB()>), dim3((unsigned)blocks), dim3(kThreads), 0,
                                   (hipStream_t)stream, gx, y, ldy, coefA, coefB, coefC, dy, lddy, T, M, C, accumulate);
            }
            return true;
        },
        OneOf<1, 4>{vec}, Flag{sb});
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_bn_bwd_apply(const float* gx, const float* y, int64_t ldy, const float* coefA, const float* coefB,
                                const float* coefC, float* dy, int64_t lddy, int T, int64_t M, int C, int accumulate,
                                void* stream) {
    return bn_bwd_apply("snn_bn_bwd_apply", false, gx, y, ldy, coefA, coefB, coefC, dy, lddy, T, M, C, accumulate, stream);
}

extern "C" int snn_bn_bwd_apply_bf16(const float* gx, const float* y, int64_t ldy, const float* coefA, const float* coefB,
                                     const float* coefC, float* dy, int64_t lddy, int T, int64_t M, int C, int accumulate,
                                     void* stream) {
    return bn_bwd_apply("snn_bn_bwd_apply_bf16", true, gx, y, ldy, coefA, coefB, coefC, dy, lddy, T, M, C, accumulate, stream);
}
