// C (+)= op(A) x op(B) for weight-sized matrices (<= a few hundred per side) on gfx950: the three products of a composed
// pair of 1x1 convolutions (functional._ComposedConv1x1: w2 w1, G w1^T, w2^T G), one product per launch or a table of
// them (k_small_gemm_batched) in one launch.
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;

// 32 x 32 tile per block, 2 x 2 per thread; K goes through LDS in chunks of 128 whose loads are all in flight at once
// (these launches are latency-, not throughput-bound: one memory round trip per chunk instead of one per 16 k); every
// element is an fp32 fmaf chain in k order (same arithmetic as the fp32 MFMA).
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
