// BatchNorm statistics of the Norm -> neuron scans (gfx950): per-timestep sums over the pixels, their second phase
// (mean / invstd / the affine the forward scan applies / running statistics) and the SyncBatchNorm forms.
//
// Reference semantics: layer_gen.py:211-214 (BatchNorm2d, per-timestep batch statistics).
#include "scan_common.h"

namespace {

// ------------------------------------------------------------------------------------------
// BatchNorm statistics: per (t, c) sum and sum of squares over the M pixels of timestep t.
// grid = (chunks, T, channel blocks); partial[t][c][chunk][2] in fp64.
// ------------------------------------------------------------------------------------------
struct StatsPlan {
    int vec, cvb, zblocks, chunks;
};

static StatsPlan stats_plan(int T, int64_t M, int C) {
    StatsPlan pl;
    pl.vec = (C % 4 == 0) ? 4 : 1;
    int cv = C / pl.vec;
    pl.cvb = cv < kThreads ? cv : kThreads;
    pl.zblocks = (int)snn_ceil_div(cv, pl.cvb);
    int P = kThreads / pl.cvb;
    int64_t want = snn_ceil_div(snn_max_blocks(), (int64_t)T * pl.zblocks);
    int64_t maxc = snn_ceil_div(M, (int64_t)P * 8);  // at least ~8 pixels per thread
    if (want > maxc) want = maxc;
    if (want < 1) want = 1;
    pl.chunks = (int)want;
    return pl;
}

template <int VEC, bool SB = false>
__global__ __launch_bounds__(kThreads) void k_bn_stats(const float* __restrict__ y, int64_t ldy, int64_t M, int C,
                                                       int cvb, double* __restrict__ partial) {
    __shared__ double red[kThreads * 2 * VEC];
    const int chunks = gridDim.x, chunk = blockIdx.x, t = blockIdx.y;
    const int cv = C / VEC;
    const int P = kThreads / cvb;
    const int tid = threadIdx.x;
    const int cgl = tid % cvb, ps = tid / cvb;
    const int cg = blockIdx.z * cvb + cgl;
    const bool active = (ps < P) && (cg < cv);
    const int64_t per = snn_ceil_div_dev(M, chunks);
    double s[VEC], q[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = q[j] = 0.0;
    if (active) {
        const int64_t m0 = (int64_t)chunk * per;
        int64_t m1 = m0 + per;
        if (m1 > M) m1 = M;
        const int64_t base = ((int64_t)t * M) * ldy + (int64_t)cg * VEC;   // element index (y: fp32, or bf16 with SB)
        for (int64_t m = m0 + ps; m < m1; m += P) {
            typename Vec<VEC>::type v = VecS<VEC, SB>::load(y, base + m * ldy);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                double d = (double)lane<VEC>(v, j);
                s[j] += d;
                q[j] += d * d;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        red[(tid * VEC + j) * 2 + 0] = s[j];
        red[(tid * VEC + j) * 2 + 1] = q[j];
    }
    __syncthreads();
    if (ps == 0 && cg < cv) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double ss = 0.0, qq = 0.0;
            for (int k = 0; k < P; ++k) {
                ss += red[((k * cvb + cgl) * VEC + j) * 2 + 0];
                qq += red[((k * cvb + cgl) * VEC + j) * 2 + 1];
            }
            double* dst = partial + snn_bn_partial_index(t, chunk, (int64_t)cg * VEC + j, chunks, C);
            dst[0] = ss;
            dst[1] = qq;
        }
    }
}

__global__ void k_bn_stats_finalize(const double* __restrict__ partial, int chunks, int T, int64_t M, int C,
                                    const float* __restrict__ gamma, const float* __restrict__ bias, float eps,
                                    const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                    int use_running, float* __restrict__ mean, float* __restrict__ invstd,
                                    float* __restrict__ alpha, float* __restrict__ beta,
                                    double* __restrict__ var_unbiased) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * C) return;
    int t = idx / C, c = idx % C;
    float mu, is;
    if (use_running) {
        mu = running_mean[c];
        is = 1.0f / sqrtf(running_var[c] + eps);  // ATen eval path: invstd in fp32
    } else {
        double s = 0.0, q = 0.0;
        for (int k = 0; k < chunks; ++k) {
            const double* src = partial + snn_bn_partial_index(t, k, c, chunks, C);
            s += src[0];
            q += src[1];
        }
        double n = (double)M;
        double m = s / n;
        double var = q / n - m * m;
        if (var < 0.0) var = 0.0;
        mu = (float)m;
        is = (float)(1.0 / sqrt(var + (double)eps));
        if (var_unbiased) var_unbiased[idx] = (M > 1) ? var * n / (n - 1.0) : var;
    }
    mean[idx] = mu;
    invstd[idx] = is;
    float g = gamma ? gamma[c] : 1.0f;
    float b = bias ? bias[c] : 0.0f;
    float a = is * g;
    alpha[idx] = a;
    beta[idx] = b - mu * a;
}

// Partials written by a convolution epilogue (conv_gather.hip) come in row tiles of `rows_per_chunk` output pixels that do
// not line up with the timesteps: chunk k of step t is the part of tile (first tile of t) + k that lies in t, so
// the number of written slots differs by one between steps.  rows_per_chunk == 0: every one of `chunks` is written.
__device__ __forceinline__ int chunks_of_step(int chunks, int rows_per_chunk, int t, int64_t M) {
    if (rows_per_chunk <= 0) return chunks;
    return (int)((((int64_t)t + 1) * M - 1) / rows_per_chunk - ((int64_t)t * M) / rows_per_chunk) + 1;
}

// One launch for the whole statistics second phase of a layer (was: finalize + running update, 27 us of two
// latency-bound kernels 22 times per step).  One block per channel; SUB lanes share the chunk partials of one
// (t, c) (each sums every SUB-th chunk in order, then a fixed xor tree), 32 timesteps per pass; thread 0 applies the T
// sequential running-stat updates of one reference forward from LDS.  Fixed summation order: deterministic.
// SUB = 8 for the few chunks snn_bn_stats writes, 32 for the hundreds of row tiles a convolution epilogue leaves.
template <int SUB>
__global__ __launch_bounds__(32 * SUB) void k_bn_stats_finalize_fused(
    const double* __restrict__ partial, int chunks, int rows_per_chunk, int T, int64_t M, int C,
    const float* __restrict__ gamma,
    const float* __restrict__ bias, float eps, float momentum, float* __restrict__ running_mean,
    float* __restrict__ running_var, int use_running, float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ alpha, float* __restrict__ beta) {
    __shared__ float sm_mean[32];
    __shared__ double sm_var[32];
    const int c = blockIdx.x;
    const int sub = threadIdx.x % SUB, tl = threadIdx.x / SUB;
    const bool update = !use_running && running_mean && running_var;
    float rm = 0.f, rv = 0.f;
    if (update && threadIdx.x == 0) {
        rm = running_mean[c];
        rv = running_var[c];
    }
    const float g = gamma ? gamma[c] : 1.0f;
    const float b = bias ? bias[c] : 0.0f;
    const double mom = (double)momentum;
    for (int tb = 0; tb < T; tb += 32) {
        const int t = tb + tl;
        double s = 0.0, q = 0.0;
        if (!use_running && t < T) {
            const int nk = chunks_of_step(chunks, rows_per_chunk, t, M);
            const double* base = partial;
            int k = sub;
            constexpr int U = SUB >= 32 ? 8 : 4;   // loads in flight (the loop is latency-bound), added in chunk order
            for (; k + (U - 1) * SUB < nk; k += U * SUB) {
                double2 p[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    p[u] = *reinterpret_cast<const double2*>(base + snn_bn_partial_index(t, k + u * SUB, c, chunks, C));
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    s += p[u].x;
                    q += p[u].y;
                }
            }
            for (; k < nk; k += SUB) {
                const double2 p0 = *reinterpret_cast<const double2*>(base + snn_bn_partial_index(t, k, c, chunks, C));
                s += p0.x; q += p0.y;
            }
        }
        for (int stride = SUB / 2; stride >= 1; stride >>= 1) {
            s += __shfl_xor(s, stride, 64);
            q += __shfl_xor(q, stride, 64);
        }
        if (sub == 0 && t < T) {
            const int idx = t * C + c;
            float mu, is;
            if (use_running) {
                mu = running_mean[c];
                is = 1.0f / sqrtf(running_var[c] + eps);  // ATen eval path: invstd in fp32
            } else {
                const double n = (double)M;
                const double m = s / n;
                double var = q / n - m * m;
                if (var < 0.0) var = 0.0;
                mu = (float)m;
                is = (float)(1.0 / sqrt(var + (double)eps));
                sm_mean[tl] = mu;
                sm_var[tl] = (M > 1) ? var * n / (n - 1.0) : var;
            }
            mean[idx] = mu;
            invstd[idx] = is;
            const float a = is * g;
            alpha[idx] = a;
            beta[idx] = b - mu * a;
        }
        if (update) {
            __syncthreads();
            if (threadIdx.x == 0) {
                const int nt = T - tb < 32 ? T - tb : 32;
                for (int k = 0; k < nt; ++k) {
                    rm = (float)(mom * (double)sm_mean[k] + (1.0 - mom) * (double)rm);
                    rv = (float)(mom * sm_var[k] + (1.0 - mom) * (double)rv);
                }
            }
            __syncthreads();
        }
    }
    if (update && threadIdx.x == 0) {
        running_mean[c] = rm;
        running_var[c] = rv;
    }
}

// chunk partials -> sums[t][c][2] (the quantity a SyncBatchNorm exchange all-reduces, config.yaml:76)
__global__ void k_bn_stats_reduce(const double* __restrict__ partial, int chunks, int rows_per_chunk, int T, int64_t M,
                                  int C, double* __restrict__ sums) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * C) return;
    int t = idx / C, c = idx % C;
    double s = 0.0, q = 0.0;
    const int nk = chunks_of_step(chunks, rows_per_chunk, t, M);
    for (int k = 0; k < nk; ++k) {
        const double* src = partial + snn_bn_partial_index(t, k, c, chunks, C);
        s += src[0];
        q += src[1];
    }
    sums[(int64_t)idx * 2 + 0] = s;
    sums[(int64_t)idx * 2 + 1] = q;
}

// T sequential running-stat updates of one reference forward (one BatchNorm call per timestep).
__global__ void k_bn_running_update(const float* __restrict__ mean, const double* __restrict__ var_unbiased, int T,
                                    int C, float momentum, float* __restrict__ running_mean,
                                    float* __restrict__ running_var) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float rm = running_mean[c], rv = running_var[c];
    const double mom = (double)momentum;
    for (int t = 0; t < T; ++t) {
        rm = (float)(mom * (double)mean[t * C + c] + (1.0 - mom) * (double)rm);
        rv = (float)(mom * var_unbiased[t * C + c] + (1.0 - mom) * (double)rv);
    }
    running_mean[c] = rm;
    running_var[c] = rv;
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
extern "C" size_t snn_bn_stats_partial_size(int T, int64_t M, int C) {
    if (T <= 0 || M <= 0 || C <= 0) return 0;
    StatsPlan pl = stats_plan(T, M, C);
    // partial sums followed by T*C unbiased variances (scratch of the finalize step)
    return (size_t)T * pl.chunks * C * 2 + (size_t)T * C;
}

static int bn_stats(const char* name, bool sb, const float* y, int64_t ldy, int T, int64_t M, int C, double* partial,
                    void* stream) {
    SNN_REQUIRE(y && partial, "%s: null pointer", name);
    SNN_REQUIRE(T > 0 && M > 0 && C > 0 && ldy >= C, "%s: bad shape T=%d M=%lld C=%d ldy=%lld", name, T, (long long)M, C,
                (long long)ldy);
    const StatsPlan pl = stats_plan(T, M, C);
    SNN_REQUIRE(!sb || (pl.vec == 4 && ldy % 4 == 0 && aligned(8, {y})),
                "%s: bad shape (C and ldy multiples of 4, y 8-byte aligned)", name);
    SNN_REQUIRE(sb || pl.vec == 1 || (ldy % 4 == 0 && aligned(16, {y})), "%s: y must be 16-byte aligned with ldy%%4==0", name);
    const dim3 grid(pl.chunks, T, pl.zblocks);
    dispatch(
        [&](auto VEC, auto SB) {
            if constexpr (VEC() == 4 || !SB()) {
                hipLaunchKernelGGL((k_bn_stats<VEC(), SB()>), grid, dim3(kThreads), 0, (hipStream_t)stream, y, ldy, M, C,
                                   pl.cvb, partial);
            }
            return true;
        },
        OneOf<1, 4>{pl.vec}, Flag{sb});
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_bn_stats(const float* y, int64_t ldy, int T, int64_t M, int C, double* partial, void* stream) {
    return bn_stats("snn_bn_stats", false, y, ldy, T, M, C, partial, stream);
}

extern "C" int snn_bn_stats_bf16(const float* y, int64_t ldy, int T, int64_t M, int C, double* partial, void* stream) {
    return bn_stats("snn_bn_stats_bf16", true, y, ldy, T, M, C, partial, stream);
}

extern "C" int snn_bn_stats_finalize(const double* partial, int chunks, int rows_per_chunk, int T, int64_t M, int C,
                                     const float* gamma,
                                     const float* bias, float eps, float momentum, float* running_mean,
                                     float* running_var, int use_running, float* mean, float* invstd, float* alpha,
                                     float* beta, void* stream) {
    SNN_REQUIRE(mean && invstd && alpha && beta, "snn_bn_stats_finalize: null output");
    SNN_REQUIRE(T > 0 && M > 0 && C > 0, "snn_bn_stats_finalize: bad shape");
    SNN_REQUIRE(use_running ? (running_mean && running_var) : (partial != nullptr),
                "snn_bn_stats_finalize: missing statistics source");
    SNN_REQUIRE(chunks >= 0 && rows_per_chunk >= 0 && (chunks > 0 || rows_per_chunk == 0),
                "snn_bn_stats_finalize: bad partial layout (chunks %d, rows per chunk %d)", chunks, rows_per_chunk);
    if (chunks == 0) chunks = stats_plan(T, M, C).chunks;   // the layout snn_bn_stats writes
    dispatch(
        [&](auto SUB) {
            hipLaunchKernelGGL(k_bn_stats_finalize_fused<SUB()>, dim3(C), dim3(32 * SUB()), 0, (hipStream_t)stream, partial,
                               chunks, rows_per_chunk, T, M, C, gamma, bias, eps, momentum, running_mean, running_var,
                               use_running, mean, invstd, alpha, beta);
            return true;
        },
        OneOf<8, 32>{(chunks > 64 && !use_running) ? 32 : 8});
    SNN_CHECK_LAUNCH("snn_bn_stats_finalize");
    return 0;
}

extern "C" int snn_bn_stats_reduce(const double* partial, int chunks, int rows_per_chunk, int T, int64_t M, int C,
                                   double* sums, void* stream) {
    SNN_REQUIRE(partial && sums && T > 0 && M > 0 && C > 0, "snn_bn_stats_reduce: bad arguments");
    SNN_REQUIRE(chunks >= 0 && rows_per_chunk >= 0 && (chunks > 0 || rows_per_chunk == 0),
                "snn_bn_stats_reduce: bad partial layout (chunks %d, rows per chunk %d)", chunks, rows_per_chunk);
    if (chunks == 0) chunks = stats_plan(T, M, C).chunks;
    int n = T * C;
    hipLaunchKernelGGL(k_bn_stats_reduce, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, partial, chunks,
                       rows_per_chunk, T, M, C, sums);
    SNN_CHECK_LAUNCH("snn_bn_stats_reduce");
    return 0;
}

extern "C" int snn_bn_stats_from_sums(const double* sums, int T, int64_t M_total, int C, const float* gamma,
                                      const float* bias, float eps, float momentum, float* running_mean,
                                      float* running_var, float* mean, float* invstd, float* alpha, float* beta,
                                      double* var_scratch, void* stream) {
    SNN_REQUIRE(sums && mean && invstd && alpha && beta && var_scratch, "snn_bn_stats_from_sums: null pointer");
    SNN_REQUIRE(T > 0 && M_total > 0 && C > 0, "snn_bn_stats_from_sums: bad shape");
    int n = T * C;
    hipLaunchKernelGGL(k_bn_stats_finalize, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums, 1, T,
                       M_total, C, gamma, bias, eps, running_mean, running_var, 0, mean, invstd, alpha, beta,
                       var_scratch);
    SNN_CHECK_LAUNCH("snn_bn_stats_from_sums");
    if (running_mean && running_var) {
        hipLaunchKernelGGL(k_bn_running_update, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean,
                           var_scratch, T, C, momentum, running_mean, running_var);
        SNN_CHECK_LAUNCH("snn_bn_running_update");
    }
    return 0;
}
