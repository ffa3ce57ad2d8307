// Whole-sequence ConvLSTM with 1x1 gates (conv_lstm.py:51-78) for gfx950: a per-pixel temporal scan with a small
// matrix product inside each step.  A workgroup owns a tile of P = 16 or 32 pixels for all T steps and has one wave per
// 16 hidden channels; that wave holds all four gates of its channels, so the cell update needs no cross-wave exchange.
// The products run on the fp32 MFMA (v_mfma_f32_16x16x4_f32): exact fp32 products, fp32 accumulation, no operand split
// and no range contract.
//
// Fragment maps of the 16x16x4 form (lane l): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// D[i = 4 * (l >> 4) + reg][j = l & 15].  K is walked in blocks of 16: lane l takes the FOUR consecutive k
// 16 * blk + 4 * (l >> 4) + {0..3} of its row with one 16-byte read and feeds them to four MFMAs - a fixed permutation
// of the summation order, the same for A and B.
//
// The weight is not shared between the waves of a workgroup (each wave reads only the rows of its own channels), so it
// goes from L2 straight to registers, one block ahead of the MFMAs that use it; the [x ; h] operand tile lives in LDS,
// double-buffered, so a step costs one barrier.  No atomics, fixed reduction order: the same inputs give the same bits.
//
// In front of the scan: the single-step cell kernels (snn_lstm_cell_fwd / _bwd), pointwise over gates the caller's
// convolution has already formed.
#include <limits.h>
#include "snn_common.h"

namespace {

// ------------------------------------------------------------------------------------------ ConvLSTM cell
// gates[m][4C] = (input, forget, output, candidate) pre-activations, conv_lstm.py:66-76 (sigmoidf_: snn_common.h)
constexpr int kThreads = 256;   // (of the cell kernels; the scan's block is 4 * Ch threads)

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

// ------------------------------------------------------------------------------------------ sequence scan
constexpr int kMinCh = 16, kMaxCh = 256, kMaxCin = 256;
constexpr int kPad = 4;   // floats added to an LDS row: rows are = 4 (mod 16) floats apart, 16-byte row reads are conflict-free

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// w[off + col .. col + 3], zero from `limit` on (VEC: col and limit are multiples of 4 and the row is 16-byte aligned)
template <bool VEC>
__device__ __forceinline__ f32x4 ldw4(const float* __restrict__ w, int64_t off, int col, int limit) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC) {
        if (col < limit) v = *reinterpret_cast<const f32x4*>(w + off + col);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j < limit) v[j] = w[off + col + j];
    }
    return v;
}

// ------------------------------------------------------------------------------------------ forward
// (MT = 2 is planned for Ch <= 128 only: 512 threads, so 256 VGPRs per wave.)
// LDS: xs[2][P][SX] (x_t, Cin padded to 16 with zeros), hl[2][P][SH] (h_{t-1}); step t reads buffer t & 1 and writes
// x_{t+1} / h_t into the other one.
template <int MT, bool VEC>
__global__ __launch_bounds__(MT == 2 ? 512 : 1024) void k_convlstm_seq_fwd(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, const float* __restrict__ h0,
    const float* __restrict__ c0, float* __restrict__ hs, float* __restrict__ cT, float* __restrict__ save_g,
    float* __restrict__ save_c, int T, int64_t M, int Cin, int Ch) {
    constexpr int P = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = Cin + Ch, nxb = (Cin + 15) / 16, nb = nxb + Ch / 16;
    const int SX = nxb * 16 + kPad, SH = Ch + kPad;
    float* xs = lds;
    float* hl = lds + 2 * P * SX;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, g = tid >> 6, col = lane & 15, q = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * P;
    const int ch = g * 16 + col;

    for (int e = tid; e < 2 * P * SX; e += nthreads) xs[e] = 0.0f;   // (the K padding stays zero)
    __syncthreads();
    for (int e = tid; e < P * Cin; e += nthreads) {
        const int p = e / Cin, c = e - p * Cin;
        const int64_t m = m0 + p;
        xs[p * SX + c] = m < M ? x[m * ldx + c] : 0.0f;
    }
    for (int e = tid; e < P * Ch; e += nthreads) {
        const int p = e / Ch, c = e - p * Ch;
        const int64_t m = m0 + p;
        hl[p * SH + c] = (h0 && m < M) ? h0[m * Ch + c] : 0.0f;
    }
    f32x4 cst[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + mt * 16 + q * 4 + r;
            cst[mt][r] = (c0 && m < M) ? c0[m * Ch + ch] : 0.0f;
        }
    int64_t wrow[4];
#pragma unroll
    for (int gate = 0; gate < 4; ++gate) wrow[gate] = (int64_t)(gate * Ch + ch) * K;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* xc = xs + (t & 1) * P * SX;
        const float* hc = hl + (t & 1) * P * SH;
        float* xn = xs + ((t + 1) & 1) * P * SX;
        float* hn = hl + ((t + 1) & 1) * P * SH;
        if (t + 1 < T) {
            const float* xt = x + (int64_t)(t + 1) * M * ldx;
            for (int e = tid; e < P * Cin; e += nthreads) {
                const int p = e / Cin, c = e - p * Cin;
                const int64_t m = m0 + p;
                xn[p * SX + c] = m < M ? xt[m * ldx + c] : 0.0f;
            }
        }
        f32x4 acc[4][MT];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[gate][mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        auto load_b = [&](int i, f32x4(&b)[4]) {
            const bool in_x = i < nxb;
            const int c = in_x ? i * 16 + q * 4 : Cin + (i - nxb) * 16 + q * 4;
            const int limit = in_x ? Cin : K;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) b[gate] = ldw4<VEC>(w, wrow[gate], c, limit);
        };
        f32x4 bcur[4], bnext[4];
        load_b(0, bcur);
        for (int i = 0; i < nb; ++i) {
            if (i + 1 < nb) load_b(i + 1, bnext);
            const bool in_x = i < nxb;
            const float* abase = in_x ? xc + i * 16 + q * 4 : hc + (i - nxb) * 16 + q * 4;
            const int astride = in_x ? SX : SH;
            f32x4 a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                a[mt] = *reinterpret_cast<const f32x4*>(abase + (mt * 16 + col) * astride);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[gate][mt] = mfma4(a[mt][j], bcur[gate][j], acc[gate][mt]);
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) bcur[gate] = bnext[gate];
        }
        // the pointwise update of k_lstm_fwd, on the accumulators: lane (q, col) holds pixels 4q .. 4q + 3 of channel ch
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = mt * 16 + q * 4 + r;
                const int64_t m = m0 + p;
                const float I = sigmoidf_(acc[0][mt][r]), F = sigmoidf_(acc[1][mt][r]), O = sigmoidf_(acc[2][mt][r]);
                const float G = tanhf(acc[3][mt][r]);
                const float cn = F * cst[mt][r] + I * G;
                const float h = O * tanhf(cn);
                cst[mt][r] = cn;
                hn[p * SH + ch] = h;
                if (m < M) {
                    const int64_t row = (int64_t)t * M + m;
                    hs[row * Ch + ch] = h;
                    if (save_g) {
                        float* sg = save_g + row * 4 * Ch + ch;
                        sg[0] = I;
                        sg[Ch] = F;
                        sg[2 * Ch] = O;
                        sg[3 * Ch] = G;
                        save_c[row * Ch + ch] = cn;
                    }
                }
            }
        __syncthreads();
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + mt * 16 + q * 4 + r;
            if (m < M) cT[m * Ch + ch] = cst[mt][r];
        }
}

// ------------------------------------------------------------------------------------------ backward
// LDS: dg[P][4Ch + pad] (dgates_t, the A operand of d[x;h] = dgates_t . w), dhl[P][Ch] (the carried dh).  The cell
// backward runs thread-linear over (pixel, channel): 4Ch threads, thread (prow = tid / Ch, ch = tid % Ch) owns pixels
// prow + 4 i, and carries their dc in registers.  The product's 16-column output tiles go round the waves.
template <int MT>
__global__ __launch_bounds__(MT == 2 ? 512 : 1024) void k_convlstm_seq_bwd(
    const float* __restrict__ w, const float* __restrict__ save_g, const float* __restrict__ save_c,
    const float* __restrict__ c0, const float* __restrict__ gh, const float* __restrict__ ghT,
    const float* __restrict__ gcT, float* __restrict__ dgates, float* __restrict__ dx, int64_t lddx,
    float* __restrict__ dh0, float* __restrict__ dc0, int T, int64_t M, int Cin, int Ch) {
    constexpr int P = 16 * MT, NI = 4 * MT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int K = Cin + Ch, C4 = 4 * Ch, SG = C4 + kPad, NT = (K + 15) / 16;
    float* dg = lds;
    float* dhl = lds + P * SG;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, col = lane & 15, q = lane >> 4;
    const int ch = tid % Ch, prow = tid / Ch;
    const int64_t m0 = (int64_t)blockIdx.x * P;

    float dcar[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = i * 4 + prow;
        const int64_t m = m0 + p;
        const bool valid = m < M;
        dcar[i] = (gcT && valid) ? gcT[m * Ch + ch] : 0.0f;
        dhl[p * Ch + ch] = (ghT && valid) ? ghT[m * Ch + ch] : 0.0f;
    }
    // (each thread reads back only the dhl entries it wrote until the first product has run: no barrier needed here)

    for (int t = T - 1; t >= 0; --t) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int p = i * 4 + prow;
            const int64_t m = m0 + p;
            float dI = 0.0f, dF = 0.0f, dO = 0.0f, dG = 0.0f;
            if (m < M) {
                const int64_t row = (int64_t)t * M + m;
                const float* sg = save_g + row * C4 + ch;
                const float I = sg[0], F = sg[Ch], O = sg[2 * Ch], G = sg[3 * Ch];
                const float tc = tanhf(save_c[row * Ch + ch]);
                const float cp = t > 0 ? save_c[(row - M) * Ch + ch] : (c0 ? c0[m * Ch + ch] : 0.0f);
                const float dh = (gh ? gh[row * Ch + ch] : 0.0f) + dhl[p * Ch + ch];
                const float dc = dcar[i] + dh * O * (1.0f - tc * tc);
                dI = (dc * G) * (I * (1.0f - I));
                dF = (dc * cp) * (F * (1.0f - F));
                dO = (dh * tc) * (O * (1.0f - O));
                dG = (dc * I) * (1.0f - G * G);
                dcar[i] = dc * F;
                float* d = dgates + row * C4 + ch;
                d[0] = dI;
                d[Ch] = dF;
                d[2 * Ch] = dO;
                d[3 * Ch] = dG;
            }
            float* l = dg + p * SG + ch;
            l[0] = dI;
            l[Ch] = dF;
            l[2 * Ch] = dO;
            l[3 * Ch] = dG;
        }
        __syncthreads();
        const bool want_h = t > 0 || dh0 != nullptr;
        for (int nt = wave; nt < NT; nt += nwaves) {
            const int n0 = nt * 16;
            const bool has_x = n0 < Cin, has_h = n0 + 16 > Cin;
            if (!((has_x && dx) || (has_h && want_h))) continue;   // (uniform per wave)
            const int n = n0 + col;
            const bool nvalid = n < K;
            f32x4 acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const float* wn = w + (nvalid ? n : 0);
            for (int kb = 0; kb < C4 / 16; ++kb) {
                const int k = kb * 16 + q * 4;
                float b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = nvalid ? wn[(int64_t)(k + j) * K] : 0.0f;
                f32x4 a[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(dg + (mt * 16 + col) * SG + k);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma4(a[mt][j], b[j], acc[mt]);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int p = mt * 16 + q * 4 + r;
                    const int64_t m = m0 + p;
                    if (n < Cin) {
                        if (dx && m < M) dx[((int64_t)t * M + m) * lddx + n] = acc[mt][r];
                    } else if (nvalid) {
                        if (t > 0) dhl[p * Ch + (n - Cin)] = acc[mt][r];
                        else if (dh0 && m < M) dh0[m * Ch + (n - Cin)] = acc[mt][r];
                    }
                }
        }
        __syncthreads();
    }
    if (dc0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int64_t m = m0 + i * 4 + prow;
            if (m < M) dc0[m * Ch + ch] = dcar[i];
        }
    }
}

// ------------------------------------------------------------------------------------------ plan
// 32 pixels per workgroup halve the weight traffic per pixel, 16 give twice as many workgroups: 32 once they fill the
// chip, and only where the backward operand tile (P x 4Ch floats beside the carried dh) fits the 160 KiB of LDS.
int tile_mt(int Ch, int64_t M) { return (Ch <= 128 && snn_ceil_div(M, 32) >= snn_num_cu()) ? 2 : 1; }

size_t fwd_lds_bytes(int P, int Cin, int Ch) {
    return sizeof(float) * 2 * P * ((size_t)snn_ceil_div(Cin, 16) * 16 + kPad + Ch + kPad);
}
size_t bwd_lds_bytes(int P, int Ch) { return sizeof(float) * P * ((size_t)4 * Ch + kPad + Ch); }

template <class Kernel> int allow_lds(Kernel kernel, size_t bytes, const char* name) {
    if (bytes <= 64 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e != hipSuccess) {
        snn_set_error("%s: %zu bytes of LDS refused: %s", name, bytes, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

}  // namespace

extern "C" int snn_lstm_cell_fwd(const float* gates, const float* c_prev, float* h, float* c, int64_t M, int C,
                                 void* stream) {
    SNN_REQUIRE(gates && h && c && M > 0 && C > 0, "snn_lstm_cell_fwd: bad arguments");
    hipLaunchKernelGGL(k_lstm_fwd, dim3(snn_grid_for(M * C, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gates,
                       c_prev, h, c, M, C);
    SNN_CHECK_LAUNCH("snn_lstm_cell_fwd");
    return 0;
}
extern "C" int snn_lstm_cell_bwd(const float* gates, const float* c_prev, const float* c, const float* gh,
                                 const float* gc, float* g_gates, float* g_c_prev, int64_t M, int C, void* stream) {
    SNN_REQUIRE(gates && c && g_gates && M > 0 && C > 0, "snn_lstm_cell_bwd: bad arguments");
    hipLaunchKernelGGL(k_lstm_bwd, dim3(snn_grid_for(M * C, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gates,
                       c_prev, c, gh, gc, g_gates, g_c_prev, M, C);
    SNN_CHECK_LAUNCH("snn_lstm_cell_bwd");
    return 0;
}

extern "C" int snn_convlstm_seq_supported(int Cin, int Ch, int64_t ldx) {
    return Ch >= kMinCh && Ch <= kMaxCh && Ch % 16 == 0 && Cin >= 1 && Cin <= kMaxCin && ldx >= Cin;
}

extern "C" int snn_convlstm_seq_tile(int Cin, int Ch, int64_t M) {
    if (!snn_convlstm_seq_supported(Cin, Ch, Cin) || M < 1) return 0;
    return 16 * tile_mt(Ch, M);
}

extern "C" int snn_convlstm_seq_fwd(const float* x, int64_t ldx, const float* w, const float* h0, const float* c0,
                                    float* hs, float* cT, float* save_gates, float* save_c, int T, int64_t M, int Cin,
                                    int Ch, void* stream) {
    SNN_REQUIRE(x && w && hs && cT && T > 0 && M > 0, "snn_convlstm_seq_fwd: bad arguments");
    SNN_REQUIRE(snn_convlstm_seq_supported(Cin, Ch, ldx), "snn_convlstm_seq_fwd: Cin=%d Ch=%d ldx=%lld not supported", Cin,
                Ch, (long long)ldx);
    SNN_REQUIRE((save_gates == nullptr) == (save_c == nullptr), "snn_convlstm_seq_fwd: save_gates and save_c go together");
    const int mt = tile_mt(Ch, M), P = 16 * mt;
    const int64_t blocks = snn_ceil_div(M, P);
    SNN_REQUIRE(blocks <= INT_MAX, "snn_convlstm_seq_fwd: M=%lld too large", (long long)M);
    const size_t lds = fwd_lds_bytes(P, Cin, Ch);
    const bool vec = Cin % 4 == 0 && aligned(16, {w});
    const bool ok = dispatch(
        [&](auto MT, auto VEC) {
            auto kernel = k_convlstm_seq_fwd<decltype(MT)::value, decltype(VEC)::value>;
            if (allow_lds(kernel, lds, "snn_convlstm_seq_fwd")) return false;
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(4 * Ch), lds, (hipStream_t)stream, x, ldx, w, h0, c0, hs,
                               cT, save_gates, save_c, T, M, Cin, Ch);
            return true;
        },
        OneOf<1, 2>{mt}, Flag{vec});
    if (!ok) return 2;
    SNN_CHECK_LAUNCH("snn_convlstm_seq_fwd");
    return 0;
}

extern "C" int snn_convlstm_seq_bwd(const float* w, const float* save_gates, const float* save_c, const float* c0,
                                    const float* gh, const float* ghT, const float* gcT, float* dgates, float* dx,
                                    int64_t lddx, float* dh0, float* dc0, int T, int64_t M, int Cin, int Ch,
                                    void* stream) {
    SNN_REQUIRE(w && save_gates && save_c && dgates && T > 0 && M > 0, "snn_convlstm_seq_bwd: bad arguments");
    SNN_REQUIRE(snn_convlstm_seq_supported(Cin, Ch, Cin), "snn_convlstm_seq_bwd: Cin=%d Ch=%d not supported", Cin, Ch);
    SNN_REQUIRE(!dx || lddx >= Cin, "snn_convlstm_seq_bwd: lddx=%lld < Cin=%d", (long long)lddx, Cin);
    const int mt = tile_mt(Ch, M), P = 16 * mt;
    const int64_t blocks = snn_ceil_div(M, P);
    SNN_REQUIRE(blocks <= INT_MAX, "snn_convlstm_seq_bwd: M=%lld too large", (long long)M);
    const size_t lds = bwd_lds_bytes(P, Ch);
    const bool ok = dispatch(
        [&](auto MT) {
            auto kernel = k_convlstm_seq_bwd<decltype(MT)::value>;
            if (allow_lds(kernel, lds, "snn_convlstm_seq_bwd")) return false;
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(4 * Ch), lds, (hipStream_t)stream, w, save_gates, save_c,
                               c0, gh, ghT, gcT, dgates, dx, lddx, dh0, dc0, T, M, Cin, Ch);
            return true;
        },
        OneOf<1, 2>{mt});
    if (!ok) return 2;
    SNN_CHECK_LAUNCH("snn_convlstm_seq_bwd");
    return 0;
}
