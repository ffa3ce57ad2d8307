// Fused BatchNorm-apply + spiking-neuron temporal scan, BPTT backward (gfx950): the reverse scan, the LIF scan from
// checkpoints, and the gradients of per-channel time constants.  Forward: scan_fwd.hip; what the two share: scan_common.h.
//
// Reference semantics: layer_gen.py:232-235 / 252-254 (norse LIFCell / LICell), tiny_yolo.py:39-44 (LI -> Tanh).
#include <algorithm>
#include "scan_common.h"

#ifdef SNN_TUNING
// tuning builds only: timing experiments on the reverse scan's BatchNorm sums (WRONG results): bit 0 no LDS accumulation,
// bit 1 no shuffles either, bit 2 no slab zeroing / write-out
__device__ int g_bwd_abl = 0;
extern "C" int snn_debug_set_bwd_abl(int v) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_bwd_abl), &v, sizeof(int)); }
#define BWD_ABL(bit) ((g_bwd_abl >> (bit)) & 1)
#else
#define BWD_ABL(bit) 0
#endif

namespace {

// value of the partner lane l ^ 32 (valid in the UPPER 32 lanes) / l ^ 16 (valid in the odd 16-lane rows)
__device__ __forceinline__ float swap32_partner(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_permlane32_swap(u, u, false, false)[0]);
}
__device__ __forceinline__ float swap16_partner(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_permlane16_swap(u, u, false, false)[0]);
}

// Wave-level combine of the per-thread BatchNorm partial sums: lanes l and l ^ stride (stride a multiple of cvb)
// hold the same channels.  The two wide strides go through the permute-swap VALU instructions of gfx950
// (v_permlane32_swap / v_permlane16_swap) instead of ds_bpermute shuffles - one dependent LDS round trip per value and
// stride less in a latency-bound scan (36 -> 30.5 us on the 19x15 and 10x8 maps).  The sum therefore ends up in the
// TOP lanes of the wave (row 3, or the upper half when cvb = 32): wave_sum_owner() names them.  Both reverse scans use
// this pair, so their sums associate identically (the checkpointed scan is tested bit-equal to the plain one).
template <int VEC>
__device__ __forceinline__ void wave_sum_channels(float (&s1)[VEC], float (&s2)[VEC], int cvb) {
    if (cvb >= 64) return;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        s1[j] += swap32_partner(s1[j]);
        s2[j] += swap32_partner(s2[j]);
        if (cvb < 32) {
            s1[j] += swap16_partner(s1[j]);
            s2[j] += swap16_partner(s2[j]);
        }
        for (int stride = cvb; stride < 16; stride <<= 1) {   // (inside a 16-lane row)
            s1[j] += __shfl_xor(s1[j], stride, 64);
            s2[j] += __shfl_xor(s2[j], stride, 64);
        }
    }
}
__device__ __forceinline__ bool wave_sum_owner(int lane, int cvb) {
    const int own_lo = cvb >= 32 ? 64 - cvb : 48;   // (cvb >= 64: every lane owns its channels)
    return cvb >= 64 || (lane >= own_lo && lane < own_lo + cvb);
}

// ------------------------------------------------------------------------------------------
// Backward (reverse-time) scan with per-(t,c) partial sums for the BatchNorm backward.
// grid = (GX pixel groups, GY channel blocks).  A thread owns NP pixels x VEC channels; per timestep it
// sums its NP contributions in registers, lanes of a wave that share channels combine with xor-shuffles,
// and one lane per (wave, channel) adds into that wave's private LDS slab red[wave][T][cb][2] (plain
// read-modify-write, fixed order).  Waves and blocks are combined in fixed order afterwards, so the
// BatchNorm gradients are bitwise reproducible.  (Channel counts whose per-block group count is not a
// power of two fall back to LDS float atomics on one shared slab.)
// ------------------------------------------------------------------------------------------
#ifndef SNN_BWD_NP
#define SNN_BWD_NP 4
#endif
constexpr int kBwdNP = SNN_BWD_NP;
#ifndef SNN_BWD_SB_DEPTH
#define SNN_BWD_SB_DEPTH 3   // operand sets in flight in the bf16-storage reverse scan (2 or 3)
#endif

// BUF (VEC = 4 only): the per-timestep operands are addressed through raw buffer resources - one per tensor and
// timestep, lane offset -1 for lanes outside the tensor, so loads return zeros and stores are dropped by the hardware
// range check.  The time loop is then straight-line code.  With per-pixel `if (ok)` branches the compiler's waitcnt
// pass could not tell the prefetched loads of step t-1 from the ones step t needs and waited for ALL of them before
// every pixel (vmcnt(0)): the prefetch bought nothing and the kernel ran at 3.9 TB/s with the texture addresser 16 %
// busy.  Host-checked: one timestep of every tensor is < 2 GiB.
// SB (SNN_SCAN_BF16_STORAGE): g_out, state, y and gx are bf16 tensors (pointers passed as float*, strides in elements).
// YF (SNN_SCAN_SUMS_FROM_STATE; LIF, MODE 1, BUF, fp32 tensors, initial state (v_leak, 0)): y is NOT read.  The only use the
// scan has for y is the BatchNorm statistic sum(gx * y), and the neuron's input x[t] = alpha*y[t] + beta - which carries the
// same information, sum(gx * x) = alpha * sum(gx * y) + beta * sum(gx) - can be rebuilt from the saved potentials the scan
// reads anyway: with v[t-1] = (vd[t-1] > v_th ? v_reset : vd[t-1]) the forward step vd[t] = v[t-1] + c_mem*((v_leak - v[t-1])
// + i'[t]) gives i'[t], and x[t] = i'[t] - (i'[t-1] + c_syn*i'[t-1]).  Walking backwards, step t holds vd[t] and has kept
// vd[t+1]: it forms i'[t+1], with the i'[t+2] of the step before x[t+2], and adds gx[t+2] * x[t+2] (kept two steps) to the
// slab row of step t+2; x[1] and x[0] follow after the loop from the initial state.  4 of the 16 bytes per neuron-timestep
// are never read; the second value of a sums pair is then sum(gx * x) (snn_bn_bwd_finalize_from_state converts).
// GR (LIF, fp32 tensors): the general gradient rule - p.surrogate and p.reset_detached, the same for every lane, are read in
// the step; false compiles the SuperSpike / reset-not-detached arm alone, the code the default rule has always run.
// PC (LIF, fp32 tensors, GR arm, y-reading; snn_lif_tau_bwd): the time constants are the per-channel arrays cmem_pc[C] /
// csyn_pc[C], loaded once per lane, and (tau_part != NULL) the scan forms their gradients
//   dL/dc_mem[c] = sum_{t,m} g_vd[t] (vd[t] - v[t-1]) / c_mem[c],   dL/dc_syn[c] = sum_{t,m} g_i[t] i'[t]
// (g_i[t]: the current's gradient as it ARRIVES at step t; i'[t] = (vd[t] - v[t-1]) / c_mem - (v_leak - v[t-1])) from the
// potentials it reads anyway.  v[t-1] needs vd[t-1], which the walk meets one step LATER: step t keeps (vd[t], g_vd[t],
// g_i[t]) and step t-1 adds step t's two terms - no operand of the prefetched set is touched early; step 0's terms follow
// behind the loop from the initial potential (v0_pc, or v_leak).  A thread's two sums stay in registers over the time loop
// and over its pixel rows; at the end of the block: the lanes that share channels (wave_sum_channels), the waves in order
// through LDS, one double pair per (pixel block, channel) into tau_part[gx][C][2].  tau_ordered = 0 (a channel-group count
// that is not a power of two, the LDS-atomics plan): LDS float atomics on one slab instead.  The other instances never read
// the five trailing arguments.
// TS (PC only): the two sums are formed (tau_part is given); without it nothing of them is compiled - a layer with fixed
// per-channel constants pays no register for them.  The twelve kept registers per pixel do not fit beside four pixels'
// operand sets in the 256 registers of two waves per SIMD (350 measured, one block per CU where the plan counts on two):
// the buffer-addressed TS instances take three pixels per thread, as the from-state scan does, and two waves per SIMD.
template <int NEURON, int VEC, int MODE, bool BUF, int NP, bool SB = false, bool YF = false, bool GR = false, bool PC = false,
          bool TS = false>
__global__ __launch_bounds__(kThreads, (YF || (TS && NP <= 3)) ? 2 : 1) void k_affine_neuron_bwd(
    const float* __restrict__ g_out, int64_t ldg, const float* __restrict__ state, const float* __restrict__ y,
    int64_t ldy, const float* __restrict__ g_vT, const float* __restrict__ g_iT, const float* __restrict__ alpha,
    const float* __restrict__ beta, int apply_scale, float* __restrict__ gx, float* __restrict__ g_v0,
    float* __restrict__ g_i0, double* __restrict__ sums, int T, int64_t M, int C, int cvb, snn_neuron_params p,
    int last_only_or_lookback, const float* __restrict__ cmem_pc = nullptr, const float* __restrict__ csyn_pc = nullptr,
    const float* __restrict__ v0_pc = nullptr, double* __restrict__ tau_part = nullptr, int tau_ordered = 0) {
    // last_only (SNN_SCAN_LAST_STEP_ONLY; LIF / LI / LI+Tanh): g_out (and LI+Tanh's saved output) are [M][..] tensors of
    // the LAST timestep; the output gradient of every earlier step is zero and nothing is read for it.
    // YF instances (never last_only) take SNN_SCAN_STATE_LOOKBACK in the same argument slot.
    const int last_only = YF ? 0 : last_only_or_lookback;
    [[maybe_unused]] const int lookback = YF ? last_only_or_lookback : 0;
    typedef typename Vec<VEC>::type V;
    constexpr int ES = SnnStore<SB>::ES;   // bytes per element of the activation tensors
    constexpr bool kNeedsX = (NEURON == SNN_NEURON_SLI || NEURON == SNN_NEURON_SYNAPSE);
    constexpr bool kNeedsState = (NEURON == SNN_NEURON_LIF || NEURON == SNN_NEURON_LI_TANH || kNeedsX);
    extern __shared__ __attribute__((aligned(16))) float red[];  // MODE 1: [wave][T][cb][2]; MODE 2: [T][cb][2]
    const int cv = C / VEC;
    const int P = kThreads / cvb;
    const int tid = threadIdx.x;
    const int cgl = tid % cvb, ps = tid / cvb;
    const int cg = blockIdx.y * cvb + cgl;
    const int cb = cvb * VEC;
    const bool lane_ok = (ps < P) && (cg < cv);
    const int c = lane_ok ? cg * VEC : 0;
    const int wave = tid >> 6;
    if (MODE != 0 && !BWD_ABL(2)) {
        const int n = (MODE == 1 ? kWaves : 1) * T * cb * 2;
        for (int k = tid; k < n; k += kThreads) red[k] = 0.0f;
        __syncthreads();
    }
    static_assert(!YF || (NEURON == SNN_NEURON_LIF && MODE == 1 && BUF && VEC == 4 && !SB), "sums from the saved state: LIF, ordered sums");
    static_assert(!GR || (NEURON == SNN_NEURON_LIF && !SB), "selectable gradient rule: LIF on fp32 tensors");
    static_assert(!PC || (GR && !YF), "per-channel time constants: the general-rule arm of the y-reading LIF scan");
    static_assert(!TS || PC, "the sums of the time constants' gradients belong to the per-channel instances");
    const float one_m_cmem = 1.0f - p.c_mem;
    const float one_p_csyn = 1.0f + p.c_syn;
    [[maybe_unused]] const float inv_cmem = 1.0f / p.c_mem;
    // PC: this lane's constants (c = 0 for a lane without channels: finite values, its sums stay 0) and its two sums
    [[maybe_unused]] float pc_cm[VEC], pc_omc[VEC], pc_opc[VEC], pc_icm[VEC], tau_m[VEC], tau_s[VEC];
    if constexpr (PC) {
        V cmv = Vec<VEC>::load(cmem_pc + c), csv = Vec<VEC>::load(csyn_pc + c);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            pc_cm[j] = lane<VEC>(cmv, j);
            pc_omc[j] = 1.0f - pc_cm[j];
            pc_opc[j] = 1.0f + lane<VEC>(csv, j);
            if constexpr (TS) {
                pc_icm[j] = 1.0f / pc_cm[j];
                tau_m[j] = tau_s[j] = 0.0f;
            }
        }
    }
    const int64_t rows = (M + P - 1) / P;
    const int64_t rpb = (rows + gridDim.x - 1) / gridDim.x;  // pixel rows per block (see bwd_plan)
    const int64_t row_lo = (int64_t)blockIdx.x * rpb;
    const int64_t row_hi = row_lo + rpb < rows ? row_lo + rpb : rows;
    for (int64_t rb = row_lo; rb < row_hi; rb += NP) {
        int64_t mq[NP];
        bool ok[NP];
        V gv[NP], gi[NP];
        // YF: what a step keeps for the statistic of two steps later - vd[t+1], i'[t+2], gx[t+1], gx[t+2]
        [[maybe_unused]] V yf_vd1[YF ? NP : 1], yf_in2[YF ? NP : 1], yf_g1[YF ? NP : 1], yf_g2[YF ? NP : 1];
        // PC: what a step keeps for the two sums' terms of its own step, formed one step later - vd[t+1], g_vd[t+1], g_i[t+1]
        [[maybe_unused]] V pc_vd1[TS ? NP : 1], pc_gvd1[TS ? NP : 1], pc_gi1[TS ? NP : 1];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            mq[q] = (rb + q) * P + ps;
            ok[q] = lane_ok && rb + q < row_hi && mq[q] < M;
#pragma unroll
            for (int j = 0; j < VEC; ++j) lane<VEC>(gv[q], j) = lane<VEC>(gi[q], j) = 0.0f;
            if constexpr (TS) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(pc_vd1[q], j) = lane<VEC>(pc_gvd1[q], j) = lane<VEC>(pc_gi1[q], j) = 0.0f;
            }
            if constexpr (YF) {
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    lane<VEC>(yf_vd1[q], j) = lane<VEC>(yf_in2[q], j) = lane<VEC>(yf_g1[q], j) = lane<VEC>(yf_g2[q], j) = 0.0f;
            }
            if (NEURON != SNN_NEURON_NONE && ok[q]) {
                if (g_vT) gv[q] = Vec<VEC>::load(g_vT + mq[q] * C + c);
                if (g_iT) gi[q] = Vec<VEC>::load(g_iT + mq[q] * C + c);
            }
        }
        // Two register sets: the loads of timestep t-1 are in flight while timestep t is processed.
        int og[NP], os[NP], oy[NP];  // BUF: byte offsets inside one timestep of g_out / (state, gx) / y; -1 = no pixel
        if constexpr (BUF) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                og[q] = ok[q] ? (int)((mq[q] * ldg + c) * ES) : -1;
                os[q] = ok[q] ? (int)((mq[q] * C + c) * ES) : -1;
                oy[q] = ok[q] ? (int)((mq[q] * ldy + c) * ES) : -1;
            }
        }
        auto slab = [&](const float* base, int t, int64_t ld) {  // buffer resource of timestep t of a [T][M][ld] tensor
            char* b = reinterpret_cast<char*>(const_cast<float*>(base)) + (int64_t)t * M * ld * ES;
            return __builtin_amdgcn_make_buffer_rsrc(b, 0, (int)(M * ld * ES), 0x00020000);
        };
        auto slab_out = [&](const float* base, int t, int64_t ld) {  // g_out / saved output: all steps, or the last one only
            if (!last_only) return slab(base, t, ld);
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, t == T - 1 ? (int)(M * ld * ES) : 0,
                                                     0x00020000);   // zero records: every load returns 0
        };
        // Operand sets in flight hold what the loads return: fp32 quads, or (bf16 storage) the 8 raw bytes of 4 bf16 values -
        // half the registers, which pays for a THIRD set: with half the bytes per step, one step of prefetch no longer
        // covers the memory latency (3.0 - 4.5 TB/s measured with two sets against 5 TB/s on fp32 tensors).
        using R = typename std::conditional<(SB && BUF), snn_u32x2, V>::type;
        constexpr int DEPTH = (SB && BUF) ? SNN_BWD_SB_DEPTH : 2;
        auto widen = [](const R& r) -> V {
            if constexpr (SB && BUF) return snn_unpack_bf16x4(r);
            else return r;
        };
        auto bload = [&](const auto& rs, int off) -> R {   // 4 elements of a storage-type tensor (generic: BUF instances only)
            if constexpr (SB && BUF) return __builtin_bit_cast(snn_u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
            else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        };
        auto bload_last = [&](const auto& rs, int off) -> R {   // the same for a tensor nobody reads again (aux 2 = nt)
            if constexpr (SB && BUF) return __builtin_bit_cast(snn_u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, SNN_SCAN_NT_AUX));
            else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, SNN_SCAN_NT_AUX));
        };
        // eval-mode BatchNorm scale alpha[t][c] (apply_scale): fetched with the operand set - a load inside a branch of the
        // time loop makes the compiler's wait-count pass fall back to small vmcnt values for the whole step (it cannot
        // know whether the load was issued), which stalls on the prefetched set.  Zero records when unused.
        [[maybe_unused]] __amdgpu_buffer_rsrc_t rsc;
        if constexpr (BUF)
            rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(apply_scale ? alpha : g_out), 0,
                                                    apply_scale ? (int)((int64_t)T * C * 4) : 0, 0x00020000);
        auto fetch = [&](int t, R (&go)[NP], R (&st)[NP], R (&yv)[NP], V& sc) {
            if constexpr (BUF) {
                sc = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rsc, lane_ok ? (t * C + c) * 4 : -1, 0, 0));
                const __amdgpu_buffer_rsrc_t rg = slab_out(g_out, t, ldg);
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    go[q] = bload_last(rg, og[q]);
                if (kNeedsState) {
                    const __amdgpu_buffer_rsrc_t rs = (NEURON == SNN_NEURON_LI_TANH) ? slab_out(state, t, C) : slab(state, t, C);
#pragma unroll
                    for (int q = 0; q < NP; ++q)
                        st[q] = bload_last(rs, os[q]);
                }
                if ((MODE != 0 && !YF) || kNeedsX) {
                    const __amdgpu_buffer_rsrc_t ry = slab(y, t, ldy);
#pragma unroll
                    for (int q = 0; q < NP; ++q)
                        yv[q] = bload(ry, oy[q]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    if (ok[q]) {
                        const int64_t row = (int64_t)t * M + mq[q];
                        const int64_t row_o = last_only ? mq[q] : row;
                        const bool live = !last_only || t == T - 1;
#pragma unroll
                        for (int j = 0; j < VEC; ++j) lane<VEC>(go[q], j) = lane<VEC>(st[q], j) = 0.0f;
                        if (live) go[q] = VecS<VEC, SB>::load(g_out, row_o * ldg + c);
                        if (kNeedsState) {
                            if (NEURON != SNN_NEURON_LI_TANH) st[q] = VecS<VEC, SB>::load(state, row * C + c);
                            else if (live) st[q] = VecS<VEC, SB>::load(state, row_o * C + c);
                        }
                        if (MODE != 0 || kNeedsX) yv[q] = VecS<VEC, SB>::load(y, row * ldy + c);
                    }
                }
            }
        };
        auto process = [&](int t, R (&go_r)[NP], R (&st_r)[NP], R (&yv_r)[NP], const V& sc_set) {
            float s1[VEC], s2[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0f;
            V xa[NP];
            if (kNeedsX) {  // x[t] = y[t]*alpha + beta, as the forward computed it
                V a1, b1;
                if (alpha) {
                    a1 = Vec<VEC>::load(alpha + (int64_t)t * C + c);
                    b1 = Vec<VEC>::load(beta + (int64_t)t * C + c);
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    V yq = widen(yv_r[q]);
#pragma unroll
                    for (int j = 0; j < VEC; ++j)
                        lane<VEC>(xa[q], j) = alpha ? lane<VEC>(yq, j) * lane<VEC>(a1, j) + lane<VEC>(b1, j) : lane<VEC>(yq, j);
                }
            }
            [[maybe_unused]] __amdgpu_buffer_rsrc_t rgx;
            if constexpr (BUF) rgx = slab(gx, t, C);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (!BUF && !ok[q]) continue;  // BUF: lanes without a pixel compute on zeros, their store is dropped
                const int64_t row = (int64_t)t * M + mq[q];
                V g;
                V go_q = widen(go_r[q]);
                [[maybe_unused]] V st_q, yv_q;
                if (kNeedsState) st_q = widen(st_r[q]);
                if (MODE != 0 && !YF) yv_q = widen(yv_r[q]);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    float goj = lane<VEC>(go_q, j);
                    if (NEURON == SNN_NEURON_NONE) {
                        lane<VEC>(g, j) = goj;
                    } else if (NEURON == SNN_NEURON_LIF) {
                        float vd = lane<VEC>(st_q, j);
                        float u = vd - p.v_th;
                        float z = (u > 0.0f) ? 1.0f : 0.0f;
                        float gvj = lane<VEC>(gv[q], j);
                        float sg, gz;
                        if constexpr (!GR) {
                            float den = p.alpha * fabsf(u) + 1.0f;
                            // bf16 storage: the 1-ulp hardware reciprocal (the result is rounded to 8 bits on its way out; the
                            // IEEE division is ten VALU instructions and made this instance VALU-bound at 3.3 TB/s)
                            sg = SB ? __builtin_amdgcn_rcpf(den * den) : 1.0f / (den * den);
                            gz = goj + gvj * (p.v_reset - vd);
                        } else {
                            // every surrogate is num / d with s(0) = 1: the branches (scalar: the rule is a kernel argument)
                            // pick the two, ONE division serves all four.  SUPER: 1 / d, the default arm's value bit for bit.
                            // SIGMOID: 4 s(x)(1 - s(x)) = 4e / (1 + e)^2 with e = exp(-|x|) - even in x, e in (0, 1]
                            const float ax = p.alpha * fabsf(u);
                            float num = 1.0f, d;
                            if (p.surrogate == SNN_SURR_TRIANGLE) {
                                num = fmaxf(0.0f, 1.0f - ax);
                                d = 1.0f;
                            } else if (p.surrogate == SNN_SURR_SIGMOID) {
                                const float e = expf(-ax);
                                const float q1 = 1.0f + e;
                                num = 4.0f * e;
                                d = q1 * q1;
                            } else if (p.surrogate == SNN_SURR_ATAN) {
                                d = 1.0f + ax * ax;
                            } else {
                                const float den = ax + 1.0f;
                                d = den * den;
                            }
                            sg = num / d;
                            // detached reset: v = (1 - z) v_dec + z v_reset with z a constant - no gradient reaches z through it
                            gz = p.reset_detached ? goj : goj + gvj * (p.v_reset - vd);
                        }
                        float g_vd = gvj * (1.0f - z) + gz * sg;
                        float g_in;
                        if constexpr (PC) {
                            const float gi_old = lane<VEC>(gi[q], j);
                            g_in = pc_cm[j] * g_vd + gi_old * pc_opc[j];
                            lane<VEC>(gv[q], j) = g_vd * pc_omc[j];
                            if constexpr (TS) {
                                // the two terms of step t+1, now that v[t] is known (zero gradients until step t+1 exists)
                                const float vprev = (u > 0.0f) ? p.v_reset : vd;                       // v[t]
                                const float dlt = (lane<VEC>(pc_vd1[q], j) - vprev) * pc_icm[j];      // (vd[t+1] - v[t]) / c_mem
                                tau_m[j] += lane<VEC>(pc_gvd1[q], j) * dlt;
                                tau_s[j] += lane<VEC>(pc_gi1[q], j) * (dlt - (p.v_leak - vprev));      // g_i[t+1] i'[t+1]
                                lane<VEC>(pc_vd1[q], j) = vd;
                                lane<VEC>(pc_gvd1[q], j) = g_vd;
                                lane<VEC>(pc_gi1[q], j) = gi_old;
                            }
                        } else {
                            g_in = p.c_mem * g_vd + lane<VEC>(gi[q], j) * one_p_csyn;
                            lane<VEC>(gv[q], j) = g_vd * one_m_cmem;
                        }
                        lane<VEC>(gi[q], j) = g_in;
                        lane<VEC>(g, j) = g_in;
                        if constexpr (YF) {   // x[t+2] from vd[t+2], vd[t+1], vd[t] (zero gradient slots until t+2 exists)
                            const float vprev = (u > 0.0f) ? p.v_reset : vd;                       // v[t]
                            const float in1 = (lane<VEC>(yf_vd1[q], j) - vprev) * inv_cmem - (p.v_leak - vprev);   // i'[t+1]
                            const float x2 = lane<VEC>(yf_in2[q], j) - (in1 + p.c_syn * in1);
                            s2[j] += lane<VEC>(yf_g2[q], j) * x2;
                            lane<VEC>(yf_in2[q], j) = in1;
                            lane<VEC>(yf_vd1[q], j) = vd;
                            lane<VEC>(yf_g2[q], j) = lane<VEC>(yf_g1[q], j);
                            lane<VEC>(yf_g1[q], j) = g_in;
                        }
                    } else if (NEURON == SNN_NEURON_SLI) {
                        const float v_old = lane<VEC>(st_q, j);
                        const float xj = lane<VEC>(xa[q], j);
                        const float s = 1.0f / (1.0f + expf(-(p.v_st - fabsf(v_old))));
                        const float sgn = (v_old > 0.0f) ? 1.0f : ((v_old < 0.0f) ? -1.0f : 0.0f);
                        float g_vn = goj + lane<VEC>(gv[q], j);
                        float g_ij = p.c_mem * g_vn + lane<VEC>(gi[q], j) * one_p_csyn;
                        lane<VEC>(gv[q], j) = g_vn * one_m_cmem + g_ij * xj * (s * (1.0f - s)) * (-sgn);
                        lane<VEC>(gi[q], j) = g_ij;
                        lane<VEC>(g, j) = g_ij * s;
                    } else if (NEURON == SNN_NEURON_SYNAPSE) {
                        const float p_new = lane<VEC>(st_q, j);
                        const float xj = lane<VEC>(xa[q], j);
                        const float td = ((xj > 0.0f) ? p.tau_sec : p.tau_dis) * p.dt;
                        float gpre = p_new, dg = 1.0f;
                        if (p.sigma != 0.0f) {
                            gpre = (4.0f * p.sigma) * (p_new - p.sigma * (p_new * p_new));
                            dg = (4.0f * p.sigma) * (1.0f - 2.0f * p.sigma * p_new);
                        }
                        const float g_pn = goj * ((gpre >= 0.0f) ? dg : 0.0f) + lane<VEC>(gv[q], j);
                        lane<VEC>(gv[q], j) = g_pn * (1.0f - td);
                        lane<VEC>(g, j) = g_pn * td;
                    } else {
                        float d = 1.0f;
                        if (NEURON == SNN_NEURON_LI_TANH) {
                            float o = lane<VEC>(st_q, j);
                            d = 1.0f - o * o;
                        }
                        float g_vn = goj * d + lane<VEC>(gv[q], j);
                        float g_in = p.c_mem * g_vn + lane<VEC>(gi[q], j) * one_p_csyn;
                        lane<VEC>(gv[q], j) = g_vn * one_m_cmem;
                        lane<VEC>(gi[q], j) = g_in;
                        lane<VEC>(g, j) = g_in;
                    }
                    if (MODE != 0) {
                        s1[j] += lane<VEC>(g, j);
                        if constexpr (!YF) s2[j] += lane<VEC>(g, j) * lane<VEC>(yv_q, j);
                    }
                }
                if (apply_scale) {
                    V sc = sc_set;
                    if constexpr (!BUF) sc = Vec<VEC>::load(alpha + (int64_t)t * C + c);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) lane<VEC>(g, j) = lane<VEC>(g, j) * lane<VEC>(sc, j);
                }
                if constexpr (BUF && SB)
                    __builtin_amdgcn_raw_buffer_store_b64(
                        __builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(rgx, 0, 0, 0)), snn_pack_bf16x4(g)), rgx,
                        os[q], 0, 0);
                else if constexpr (BUF)
                    __builtin_amdgcn_raw_buffer_store_b128(
                        __builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(rgx, 0, 0, 0)), g), rgx, os[q],
                        0, 0);
                else
                    VecS<VEC, SB>::store(gx, row * C + c, g);
            }
            if (MODE == 1) {
                if (!BWD_ABL(1)) wave_sum_channels<VEC>(s1, s2, cvb);
                if (wave_sum_owner(tid & 63, cvb) && lane_ok && !BWD_ABL(0)) {
                    float* r = red + (((int64_t)wave * T + t) * cb + cgl * VEC) * 2;
                    if constexpr (YF) {   // s2 belongs to step t + 2
#pragma unroll
                        for (int j = 0; j < VEC; ++j) r[j * 2 + 0] += s1[j];
                        if (t + 2 < T) {
#pragma unroll
                            for (int j = 0; j < VEC; ++j) r[(2 * cb + j) * 2 + 1] += s2[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            r[j * 2 + 0] += s1[j];
                            r[j * 2 + 1] += s2[j];
                        }
                    }
                }
            } else if (MODE == 2) {
                if (lane_ok) {
                    float* r = red + ((int64_t)t * cb + cgl * VEC) * 2;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        atomicAdd(r + j * 2 + 0, s1[j]);
                        atomicAdd(r + j * 2 + 1, s2[j]);
                    }
                }
            }
                };
        R goA[NP], stA[NP], yvA[NP], goB[NP], stB[NP], yvB[NP];
        V scA, scB;
        // steps below 0 re-read step 0: no branch around the loads of the BUF form (see the note on `rsc`)
        auto fetch0 = [&](int t, R (&go)[NP], R (&st)[NP], R (&yv)[NP], V& sc) { fetch(t > 0 ? t : 0, go, st, yv, sc); };
        if constexpr (DEPTH == 3) {
            // three sets, two steps ahead
            R goC[NP], stC[NP], yvC[NP];
            V scC;
            fetch(T - 1, goA, stA, yvA, scA);
            fetch0(T - 2, goB, stB, yvB, scB);
            for (int t = T - 1; t >= 0; t -= 3) {
                fetch0(t - 2, goC, stC, yvC, scC);
                process(t, goA, stA, yvA, scA);
                if (t >= 1) {
                    fetch0(t - 3, goA, stA, yvA, scA);
                    process(t - 1, goB, stB, yvB, scB);
                }
                if (t >= 2) {
                    fetch0(t - 4, goB, stB, yvB, scB);
                    process(t - 2, goC, stC, yvC, scC);
                }
            }
        } else if constexpr (BUF) {
            fetch(T - 1, goA, stA, yvA, scA);
            for (int t = T - 1; t >= 0; t -= 2) {
                fetch0(t - 1, goB, stB, yvB, scB);
                process(t, goA, stA, yvA, scA);
                if (t >= 1) {
                    fetch0(t - 2, goA, stA, yvA, scA);
                    process(t - 1, goB, stB, yvB, scB);
                }
            }
        } else {
            fetch(T - 1, goA, stA, yvA, scA);
            for (int t = T - 1; t >= 0; t -= 2) {
                if (t >= 1) fetch(t - 1, goB, stB, yvB, scB);
                process(t, goA, stA, yvA, scA);
                if (t >= 1) {
                    if (t >= 2) fetch(t - 2, goA, stA, yvA, scA);
                    process(t - 1, goB, stB, yvB, scB);
                }
            }
        }
        if constexpr (YF) {
            // the two statistics the loop still owes: x[1] = i'[1] - i[0] and x[0] = i'[0] - i[-1] (after the loop: vd1 =
            // vd[0], in2 = i'[1], g1 = gx[0], g2 = gx[1]).  The state before step 0 is the initial one, (v_leak, 0) - or,
            // for a segment of a longer scan (SNN_SCAN_STATE_LOOKBACK), what the two saved potentials in front of the
            // segment say: v[-1] from vd[-1], i[-1] from vd[-1] and vd[-2].
            V vm1[NP], vm2[NP];
            if (lookback) {
                const __amdgpu_buffer_rsrc_t rs1 = slab(state, -1, C), rs2 = slab(state, -2, C);
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    vm1[q] = bload(rs1, os[q]);
                    vm2[q] = bload(rs2, os[q]);
                }
            }
            float sa[VEC], sb0[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) sa[j] = sb0[j] = 0.0f;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    float vp1 = p.v_leak, ip = 0.0f;
                    if (lookback) {
                        const float a = lane<VEC>(vm1[q], j), b = lane<VEC>(vm2[q], j);
                        const float vp2 = (b - p.v_th > 0.0f) ? p.v_reset : b;
                        const float im1 = (a - vp2) * inv_cmem - (p.v_leak - vp2);
                        ip = im1 + p.c_syn * im1;
                        vp1 = (a - p.v_th > 0.0f) ? p.v_reset : a;
                    }
                    const float in0 = (lane<VEC>(yf_vd1[q], j) - vp1) * inv_cmem - (p.v_leak - vp1);
                    const float x1 = lane<VEC>(yf_in2[q], j) - (in0 + p.c_syn * in0);
                    sa[j] += lane<VEC>(yf_g2[q], j) * x1;
                    sb0[j] += lane<VEC>(yf_g1[q], j) * (in0 - ip);
                }
            }
            wave_sum_channels<VEC>(sa, sb0, cvb);
            if (wave_sum_owner(tid & 63, cvb) && lane_ok) {
                float* r = red + (((int64_t)wave * T) * cb + cgl * VEC) * 2;
#pragma unroll
                for (int j = 0; j < VEC; ++j) r[j * 2 + 1] += sb0[j];
                if (T >= 2) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) r[(cb + j) * 2 + 1] += sa[j];
                }
            }
        }
        if constexpr (TS) {
            // step 0's two terms: v[-1] is the initial potential (a pixel slot without a pixel kept zeros: no terms)
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                V v0v;
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(v0v, j) = p.v_leak;
                if (v0_pc && ok[q]) v0v = Vec<VEC>::load(v0_pc + mq[q] * C + c);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float vprev = lane<VEC>(v0v, j);
                    const float dlt = (lane<VEC>(pc_vd1[q], j) - vprev) * pc_icm[j];
                    tau_m[j] += lane<VEC>(pc_gvd1[q], j) * dlt;
                    tau_s[j] += lane<VEC>(pc_gi1[q], j) * (dlt - (p.v_leak - vprev));
                }
            }
        }
        if (NEURON != SNN_NEURON_NONE) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (!ok[q]) continue;
                if (g_v0) Vec<VEC>::store(g_v0 + mq[q] * C + c, gv[q]);
                if (g_i0) Vec<VEC>::store(g_i0 + mq[q] * C + c, gi[q]);
            }
        }
    }
    if (MODE != 0 && !BWD_ABL(2)) {
        __syncthreads();
        // sums[bx][t][c][2], stored as fp32 (the block sums ARE fp32; doubles would only double the bytes the
        // finalize kernel reads back: up to 512 x T x C x 2 values per layer)
        float* dst = reinterpret_cast<float*>(sums) + (int64_t)blockIdx.x * T * C * 2;
        const int c_lo = blockIdx.y * cb;
        for (int k = tid; k < T * cb; k += kThreads) {
            int t = k / cb, cl = k % cb;
            if (c_lo + cl < C) {
                float a = 0.0f, b = 0.0f;
                if (MODE == 1) {
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) {
                        a += red[((int64_t)w * T * cb + k) * 2 + 0];
                        b += red[((int64_t)w * T * cb + k) * 2 + 1];
                    }
                } else {
                    a = red[k * 2 + 0];
                    b = red[k * 2 + 1];
                }
                dst[((int64_t)t * C + c_lo + cl) * 2 + 0] = a;
                dst[((int64_t)t * C + c_lo + cl) * 2 + 1] = b;
            }
        }
    }
    if constexpr (TS) {
        {
            // the block's two sums per channel, through the LDS the BatchNorm sums no longer need (the host sizes it for
            // both): red[slab][cb][2], one slab per wave (ordered) or one for all (atomics)
            const int nslab = tau_ordered ? kWaves : 1;
            __syncthreads();
            for (int k = tid; k < nslab * cb * 2; k += kThreads) red[k] = 0.0f;
            __syncthreads();
            if (tau_ordered) {
                wave_sum_channels<VEC>(tau_m, tau_s, cvb);
                if (wave_sum_owner(tid & 63, cvb) && lane_ok) {
                    float* r = red + ((int64_t)wave * cb + cgl * VEC) * 2;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        r[j * 2 + 0] = tau_m[j];
                        r[j * 2 + 1] = tau_s[j];
                    }
                }
            } else if (lane_ok) {
                float* r = red + (int64_t)(cgl * VEC) * 2;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    atomicAdd(r + j * 2 + 0, tau_m[j]);
                    atomicAdd(r + j * 2 + 1, tau_s[j]);
                }
            }
            __syncthreads();
            const int c_lo = blockIdx.y * cb;
            for (int k = tid; k < cb; k += kThreads) {
                if (c_lo + k < C) {
                    double a = 0.0, b = 0.0;
                    for (int w = 0; w < nslab; ++w) {
                        a += (double)red[((int64_t)w * cb + k) * 2 + 0];
                        b += (double)red[((int64_t)w * cb + k) * 2 + 1];
                    }
                    double* dst = tau_part + ((int64_t)blockIdx.x * C + c_lo + k) * 2;
                    dst[0] = a;
                    dst[1] = b;
                }
            }
        }
    }
}

// Second phase of the time constants' gradients (snn_lif_tau_finalize): the per-block partials of k_affine_neuron_bwd<PC>
// -> dL/dw_mem, dL/dw_syn under c_mem = sigmoid(w_mem), 1 + c_syn = sigmoid(w_syn).  One wave per channel: lane k adds the
// pixel blocks k, k + 64, ... in order, a fixed xor tree combines the lanes, then the chain rule c (1 - c).  per_layer (one
// block): a wave adds its channels w, w + waves, ... in order, thread 0 the waves in order - one pair for the layer.
__global__ __launch_bounds__(1024) void k_lif_tau_finalize(const double* __restrict__ part, int gx_blocks, int C,
                                                           const float* __restrict__ c_mem, const float* __restrict__ c_syn,
                                                           int per_layer, float* __restrict__ d_wmem,
                                                           float* __restrict__ d_wsyn, int accumulate) {
    __shared__ double sm[16][2];
    const int ln = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double tm = 0.0, ts = 0.0;
    const int c_first = per_layer ? w : blockIdx.x * nw + w;
    const int c_step = per_layer ? nw : C;   // (per channel: one channel per wave)
    for (int c = c_first; c < C; c += c_step) {
        double a = 0.0, b = 0.0;
        for (int bk = ln; bk < gx_blocks; bk += 64) {
            const double2 v = *reinterpret_cast<const double2*>(part + ((int64_t)bk * C + c) * 2);
            a += v.x;
            b += v.y;
        }
        for (int stride = 32; stride >= 1; stride >>= 1) {
            a += __shfl_xor(a, stride, 64);
            b += __shfl_xor(b, stride, 64);
        }
        const double cm = (double)c_mem[c], s = (double)(1.0f + c_syn[c]);
        a *= cm * (1.0 - cm);
        b *= s * (1.0 - s);
        if (per_layer) {
            tm += a;
            ts += b;
        } else if (ln == 0) {
            if (d_wmem) d_wmem[c] = accumulate ? d_wmem[c] + (float)a : (float)a;
            if (d_wsyn) d_wsyn[c] = accumulate ? d_wsyn[c] + (float)b : (float)b;
        }
    }
    if (!per_layer) return;
    if (ln == 0) {
        sm[w][0] = tm;
        sm[w][1] = ts;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < nw; ++k) {
            a += sm[k][0];
            b += sm[k][1];
        }
        if (d_wmem) d_wmem[0] = accumulate ? d_wmem[0] + (float)a : (float)a;
        if (d_wsyn) d_wsyn[0] = accumulate ? d_wsyn[0] + (float)b : (float)b;
    }
}

// The parametrisation (snn_lif_tau_param): c_mem[c] = sigmoid(w_mem), c_syn[c] = sigmoid(w_syn) - 1, from one value per
// layer (n = 1) or per channel (n = C).
__global__ void k_lif_tau_param(const float* __restrict__ w_mem, const float* __restrict__ w_syn, int n, int C,
                                float* __restrict__ c_mem, float* __restrict__ c_syn) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int k = n == 1 ? 0 : c;
    c_mem[c] = 1.0f / (1.0f + expf(-w_mem[k]));
    c_syn[c] = 1.0f / (1.0f + expf(-w_syn[k])) - 1.0f;
}

// LIF backward scan from checkpoints (forward SAVE mode 2).  Same grid, block roles, reduction order and outputs as
// k_affine_neuron_bwd<LIF>; per chunk of kCkpt steps (last chunk first) a thread re-runs the forward recurrence from
// the chunk's saved (v, i) - the very expressions of k_affine_neuron_fwd, so the recomputed membrane values are the
// forward's bit for bit - and then walks the chunk backwards.  The next chunk's loads are issued before the current
// chunk is processed.
constexpr int kCkptNP = 2;
template <int VEC, int MODE>
__global__ __launch_bounds__(kThreads) void k_lif_bwd_ckpt(
    const float* __restrict__ g_out, int64_t ldg, const float* __restrict__ ckpt, const float* __restrict__ y,
    int64_t ldy, const float* __restrict__ g_vT, const float* __restrict__ g_iT, const float* __restrict__ alpha,
    const float* __restrict__ beta, int apply_scale, float* __restrict__ gx, float* __restrict__ g_v0,
    float* __restrict__ g_i0, double* __restrict__ sums, int T, int64_t M, int C, int cvb, snn_neuron_params p) {
    typedef typename Vec<VEC>::type V;
    constexpr int NP = kCkptNP;
    constexpr int K = kCkpt;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int cv = C / VEC;
    const int P = kThreads / cvb;
    const int tid = threadIdx.x;
    const int cgl = tid % cvb, ps = tid / cvb;
    const int cg = blockIdx.y * cvb + cgl;
    const int cb = cvb * VEC;
    const bool lane_ok = (ps < P) && (cg < cv);
    const int c = lane_ok ? cg * VEC : 0;
    const int wave = tid >> 6;
    if (MODE != 0) {
        const int n = (MODE == 1 ? kWaves : 1) * T * cb * 2;
        for (int k = tid; k < n; k += kThreads) red[k] = 0.0f;
        __syncthreads();
    }
    const float one_m_cmem = 1.0f - p.c_mem;
    const float one_p_csyn = 1.0f + p.c_syn;
    const int64_t rows = (M + P - 1) / P;
    const int64_t rpb = (rows + gridDim.x - 1) / gridDim.x;
    const int64_t row_lo = (int64_t)blockIdx.x * rpb;
    const int64_t row_hi = row_lo + rpb < rows ? row_lo + rpb : rows;
    const int nchunks = (T + K - 1) / K;
    struct Set {
        V v[NP], i[NP], yv[K][NP], go[K][NP];
    };
    for (int64_t rb = row_lo; rb < row_hi; rb += NP) {
        int64_t mq[NP];
        bool ok[NP];
        V gv[NP], gi[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            mq[q] = (rb + q) * P + ps;
            ok[q] = lane_ok && rb + q < row_hi && mq[q] < M;
#pragma unroll
            for (int j = 0; j < VEC; ++j) lane<VEC>(gv[q], j) = lane<VEC>(gi[q], j) = 0.0f;
            if (ok[q]) {
                if (g_vT) gv[q] = Vec<VEC>::load(g_vT + mq[q] * C + c);
                if (g_iT) gi[q] = Vec<VEC>::load(g_iT + mq[q] * C + c);
            }
        }
        auto fetch = [&](int ch, Set& s) {
            const int t0 = ch * K;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (!ok[q]) continue;
                const float* ck = ckpt + ((int64_t)ch * 2 * M + mq[q]) * C + c;
                s.v[q] = Vec<VEC>::load(ck);
                s.i[q] = Vec<VEC>::load(ck + M * C);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (t0 + k < T) {
                        const int64_t row = (int64_t)(t0 + k) * M + mq[q];
                        s.yv[k][q] = Vec<VEC>::load(y + row * ldy + c);
                        s.go[k][q] = Vec<VEC>::load(g_out + row * ldg + c);
                    }
                }
            }
        };
        auto process = [&](int ch, Set& s) {
            const int t0 = ch * K;
            V vd[K][NP];
            // forward recurrence of the chunk (k_affine_neuron_fwd, LIF branch)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (t0 + k >= T) continue;
                V a1, b1;
                if (alpha) {
                    a1 = Vec<VEC>::load(alpha + (int64_t)(t0 + k) * C + c);
                    b1 = Vec<VEC>::load(beta + (int64_t)(t0 + k) * C + c);
                }
#pragma unroll
                for (int q = 0; q < NP; ++q)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        float xj = lane<VEC>(s.yv[k][q], j);
                        if (alpha) xj = xj * lane<VEC>(a1, j) + lane<VEC>(b1, j);
                        const float vj = lane<VEC>(s.v[q], j), ij = lane<VEC>(s.i[q], j);
                        const float i_new = ij + xj;
                        const float dv = p.c_mem * ((p.v_leak - vj) + i_new);
                        const float v_dec = vj + dv;
                        const float di = p.c_syn * i_new;
                        lane<VEC>(s.i[q], j) = i_new + di;
                        const float u = v_dec - p.v_th;
                        const float z = (u > 0.0f) ? 1.0f : 0.0f;
                        lane<VEC>(s.v[q], j) = (1.0f - z) * v_dec + z * p.v_reset;
                        lane<VEC>(vd[k][q], j) = v_dec;
                    }
            }
            // reverse-time walk of the chunk (k_affine_neuron_bwd, LIF branch)
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                const int t = t0 + k;
                if (t >= T) continue;
                float s1[VEC], s2[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0f;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    if (!ok[q]) continue;
                    const int64_t row = (int64_t)t * M + mq[q];
                    V g;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float goj = lane<VEC>(s.go[k][q], j);
                        const float vdj = lane<VEC>(vd[k][q], j);
                        const float u = vdj - p.v_th;
                        const float z = (u > 0.0f) ? 1.0f : 0.0f;
                        const float den = p.alpha * fabsf(u) + 1.0f;
                        const float sg = 1.0f / (den * den);
                        const float gvj = lane<VEC>(gv[q], j);
                        const float gz = goj + gvj * (p.v_reset - vdj);
                        const float g_vd = gvj * (1.0f - z) + gz * sg;
                        const float g_in = p.c_mem * g_vd + lane<VEC>(gi[q], j) * one_p_csyn;
                        lane<VEC>(gv[q], j) = g_vd * one_m_cmem;
                        lane<VEC>(gi[q], j) = g_in;
                        lane<VEC>(g, j) = g_in;
                        if (MODE != 0) {
                            s1[j] += g_in;
                            s2[j] += g_in * lane<VEC>(s.yv[k][q], j);
                        }
                    }
                    if (apply_scale) {
                        V sc = Vec<VEC>::load(alpha + (int64_t)t * C + c);
#pragma unroll
                        for (int j = 0; j < VEC; ++j) lane<VEC>(g, j) = lane<VEC>(g, j) * lane<VEC>(sc, j);
                    }
                    Vec<VEC>::store(gx + row * C + c, g);
                }
                if (MODE == 1) {
                    wave_sum_channels<VEC>(s1, s2, cvb);
                    if (wave_sum_owner(tid & 63, cvb) && lane_ok) {
                        float* r = red + (((int64_t)wave * T + t) * cb + cgl * VEC) * 2;
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            r[j * 2 + 0] += s1[j];
                            r[j * 2 + 1] += s2[j];
                        }
                    }
                } else if (MODE == 2) {
                    if (lane_ok) {
                        float* r = red + ((int64_t)t * cb + cgl * VEC) * 2;
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            atomicAdd(r + j * 2 + 0, s1[j]);
                            atomicAdd(r + j * 2 + 1, s2[j]);
                        }
                    }
                }
            }
        };
        Set A, B;
        fetch(nchunks - 1, A);
        for (int ch = nchunks - 1; ch >= 0; ch -= 2) {
            if (ch >= 1) fetch(ch - 1, B);
            process(ch, A);
            if (ch >= 1) {
                if (ch >= 2) fetch(ch - 2, A);
                process(ch - 1, B);
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (!ok[q]) continue;
            if (g_v0) Vec<VEC>::store(g_v0 + mq[q] * C + c, gv[q]);
            if (g_i0) Vec<VEC>::store(g_i0 + mq[q] * C + c, gi[q]);
        }
    }
    if (MODE != 0) {
        __syncthreads();
        float* dst = reinterpret_cast<float*>(sums) + (int64_t)blockIdx.x * T * C * 2;
        const int c_lo = blockIdx.y * cb;
        for (int k = tid; k < T * cb; k += kThreads) {
            int t = k / cb, cl = k % cb;
            if (c_lo + cl < C) {
                float a = 0.0f, b = 0.0f;
                if (MODE == 1) {
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) {
                        a += red[((int64_t)w * T * cb + k) * 2 + 0];
                        b += red[((int64_t)w * T * cb + k) * 2 + 1];
                    }
                } else {
                    a = red[k * 2 + 0];
                    b = red[k * 2 + 1];
                }
                dst[((int64_t)t * C + c_lo + cl) * 2 + 0] = a;
                dst[((int64_t)t * C + c_lo + cl) * 2 + 1] = b;
            }
        }
    }
}

// ---------------------------------------------------------------------------------- host side: plans and dispatch
const char* const kBadSurrogate = "unknown surrogate code (SNN_SURR_SUPER / _TRIANGLE / _SIGMOID / _ATAN)";
const char* const kGradientRuleCovers =
    "a non-default gradient rule (surrogate != SNN_SURR_SUPER or reset_detached != 0) is for SNN_NEURON_LIF";
const char* const kGradientRuleNoBf16 =
    "a non-default gradient rule (surrogate != SNN_SURR_SUPER or reset_detached != 0) has no bf16-storage scan";
const char* const kSumsFromStateCovers =
    "SNN_SCAN_SUMS_FROM_STATE not covered (ask snn_affine_neuron_bwd_sums_from_state; LIF from the initial state, sums "
    "wanted, train-mode BatchNorm)";
const char* const kTauNoLastStep =
    "SNN_SCAN_LAST_STEP_ONLY is not built together with the sums of the time constants' gradients";

// ---- reverse scan: everything snn_affine_neuron_bwd / snn_lif_tau_bwd decide from shape and flags, pointer values apart.
// The launch consumes it and the host-only queries snn_affine_neuron_bwd_plan / snn_lif_tau_bwd_plan export it, so a test
// that asks a query asserts the instance that really runs.
// The kernel's gradient arm, one chain in which each step compiles more in: the default rule, the general rule (GR), with
// per-channel time constants (GR, PC), with those and the two sums of their gradients (GR, PC, TS).  A call asks for
// kRuleDefault (the neuron parameters decide between the first two), kRuleTau or kRuleTauSums.
enum ScanRule { kRuleDefault = 0, kRuleGeneral, kRuleTau, kRuleTauSums };
struct ScanBwdPlan {
    BwdPlan pl;
    bool buf, sb, yf;         // BUF / SB / YF of the kernel
    ScanRule rule;            // GR / PC / TS of the kernel
    int np;                   // NP: pixel rows per thread
    int lookback, last_only;
    bool ordered;             // per-channel constants: their two sums combine lanes and waves in fixed order (false: LDS
                              // float atomics, the channel-group count is no power of two)
    size_t lds_bytes;         // of the launch: the BatchNorm slabs, or the two sums' slabs where those are larger
    const char* refusal;      // what shape and flags alone rule out (nullptr: nothing)
};
static ScanBwdPlan scan_bwd_plan(int neuron, int T, int64_t M, int C, int64_t ldg, int64_t ldy, bool with_sums,
                                 const snn_neuron_params* p, int flags, ScanRule ask = kRuleDefault) {
    ScanBwdPlan sp = {};
    auto refuse = [&sp](const char* why) {
        sp.refusal = why;
        return sp;
    };
    const bool pc = ask >= kRuleTau, ts = ask == kRuleTauSums;
    if (pc && (neuron != SNN_NEURON_LIF || (flags & (SNN_SCAN_BF16_STORAGE | SNN_SCAN_SUMS_FROM_STATE | SNN_SCAN_STATE_LOOKBACK))))
        return refuse(kTauCovers);
    if (ts && (flags & SNN_SCAN_LAST_STEP_ONLY)) return refuse(kTauNoLastStep);
    if (!p) return refuse("null neuron parameters");
    if (flags & ~(SNN_SCAN_WIDE_ADDRESSING | SNN_SCAN_LAST_STEP_ONLY | SNN_SCAN_BF16_STORAGE | SNN_SCAN_SUMS_FROM_STATE |
                  SNN_SCAN_STATE_LOOKBACK))
        return refuse("unknown flags");
    const bool wide = (flags & SNN_SCAN_WIDE_ADDRESSING) != 0;
    sp.last_only = (flags & SNN_SCAN_LAST_STEP_ONLY) != 0;
    sp.sb = (flags & SNN_SCAN_BF16_STORAGE) != 0;   // g_out, state, y, gx are bf16 tensors
    sp.yf = (flags & SNN_SCAN_SUMS_FROM_STATE) != 0;
    sp.lookback = (flags & SNN_SCAN_STATE_LOOKBACK) != 0;
    if (sp.lookback && !sp.yf) return refuse("SNN_SCAN_STATE_LOOKBACK belongs to SNN_SCAN_SUMS_FROM_STATE");
    if (!(T > 0 && M > 0 && C > 0 && ldg >= C)) return refuse("bad shape");
    if (neuron < SNN_NEURON_NONE || neuron > SNN_NEURON_SYNAPSE) return refuse("bad neuron");
    if (sp.last_only && !last_step_neuron(neuron)) return refuse("SNN_SCAN_LAST_STEP_ONLY is for LIF / LI / LI+Tanh");
    if (p->surrogate < SNN_SURR_SUPER || p->surrogate > SNN_SURR_ATAN) return refuse(kBadSurrogate);
    const bool gr = p->surrogate != SNN_SURR_SUPER || p->reset_detached != 0;
    if (gr && neuron != SNN_NEURON_LIF) return refuse(kGradientRuleCovers);
    if (gr && sp.sb) return refuse(kGradientRuleNoBf16);
    // (the per-channel family is one: its general arm serves the default rule too)
    sp.rule = pc ? ask : gr ? kRuleGeneral : kRuleDefault;
    sp.pl = bwd_plan(T, M, C, with_sums);
    if (sp.sb && !(sp.pl.vec == 4 && bf16_neuron(neuron))) return refuse(kBf16Covers);
    // buffer addressing (see k_affine_neuron_bwd): one timestep of every tensor must fit a 31-bit byte offset
    const int64_t ld_max = std::max({ldg, sp.yf ? 0 : ldy, (int64_t)C});   // (the y-free scan does not address y)
    sp.buf = sp.pl.vec == 4 && !wide && M * ld_max * 4 < 0x7fffffffLL;
    if (sp.yf) {
        // LIF with the ordered sums, buffer addressing, fp32 tensors, all T gradients; the rebuilt input divides by
        // c_mem: keep the amplification of the potentials' rounding error bounded
        const bool ok = neuron == SNN_NEURON_LIF && with_sums && sp.buf && sp.pl.mode == 1 && ldg % 4 == 0 && !sp.last_only &&
                        !sp.sb && p->c_mem >= 1.0f / 64.0f && p->c_mem <= 1.0f;
        if (!ok) return refuse(kSumsFromStateCovers);
        // three pixels per thread: the four values a pixel keeps for the statistic of two steps later do not fit the
        // 256 registers of two waves per SIMD beside four pixels' operand sets (287, or 21 spilled)
        sp.np = sp.pl.rpb < 3 ? (int)sp.pl.rpb : 3;
    } else {
        // (blocks with a single pixel row take the one-pixel-per-thread instance: the three empty pixel slots of the
        // four-pixel one are computed and issued in straight-line code - measured 58 us against 45 for the branchy kernel)
        sp.np = (sp.buf && sp.pl.rpb == 1) ? 1 : kBwdNP;
        // with the two sums: three pixels per thread where the plain scan takes four (see the kernel's note on TS)
        if (ts && sp.buf && sp.np == kBwdNP) sp.np = 3;
    }
    sp.lds_bytes = sp.pl.lds_bytes;
    const BwdPlan& pl = sp.pl;
    sp.ordered = pc && (pl.mode == 1 || (pl.mode == 0 && (is_pow2(pl.cvb) || pl.cvb >= 64)));
    if (ts) sp.lds_bytes = std::max(pl.lds_bytes, (size_t)(sp.ordered ? kWaves : 1) * pl.cvb * pl.vec * 2 * sizeof(float));
    return sp;
}

constexpr bool bwd_instance(int neuron, int vec, int mode, bool buf, int np, bool sb, bool yf, bool gr, bool pc = false,
                            bool ts = false) {
    if (pc && !(gr && !yf)) return false;                       // per-channel constants: the general arm, y-reading
    if (ts) return pc && neuron == SNN_NEURON_LIF && !sb && (buf ? (vec == 4 && (np == 1 || np == 3)) : np == kBwdNP);
    if (gr && (neuron != SNN_NEURON_LIF || sb)) return false;   // one general instance per fp32 LIF instance, no others
    if (yf) return neuron == SNN_NEURON_LIF && vec == 4 && mode == 1 && buf && np <= 3 && !sb;
    return (np == 1 ? buf : np == kBwdNP) && (vec == 4 || !(buf || sb)) && (!sb || bf16_neuron(neuron));
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
extern "C" size_t snn_affine_neuron_bwd_sums_size(int T, int64_t M, int C) {
    if (T <= 0 || M <= 0 || C <= 0) return 0;
    BwdPlan pl = bwd_plan(T, M, C, true);
    return (size_t)pl.gx * T * C * 2;
}

extern "C" int snn_affine_neuron_bwd_sums_from_state(int neuron, int T, int64_t M, int C, int64_t ldg,
                                                     const snn_neuron_params* p, int flags) {
    return scan_bwd_plan(neuron, T, M, C, ldg, C, true, p, flags | SNN_SCAN_SUMS_FROM_STATE).refusal ? 0 : 1;
}

// The ten words both plan queries export: vec, mode, BUF, NP, cvb, gy, gx, rpb, partial last pixel row, LDS bytes of the
// BatchNorm slabs.
static void export_scan_bwd_plan(const ScanBwdPlan& sp, int64_t M, int64_t* out) {
    const int P = kThreads / sp.pl.cvb;
    const int64_t words[10] = {sp.pl.vec, sp.pl.mode, sp.buf, sp.np, sp.pl.cvb, sp.pl.gy, sp.pl.gx, sp.pl.rpb, (M % P) != 0,
                               (int64_t)sp.pl.lds_bytes};
    std::copy(words, words + 10, out);
}

// The plan snn_affine_neuron_bwd launches this call with (host-only), out[10].  Returns 0, or 1 (message in snn_last_error)
// for a call snn_affine_neuron_bwd refuses by its shape or flags alone.
extern "C" int snn_affine_neuron_bwd_plan(int neuron, int T, int64_t M, int C, int64_t ldg, int64_t ldy, int with_sums,
                                          const snn_neuron_params* p, int flags, int64_t* out) {
    SNN_REQUIRE(out && p, "snn_affine_neuron_bwd_plan: null pointer");
    const ScanBwdPlan sp = scan_bwd_plan(neuron, T, M, C, ldg, ldy, with_sums != 0, p, flags);
    SNN_REQUIRE(!sp.refusal, "snn_affine_neuron_bwd_plan: %s (neuron %d, flags 0x%x)", sp.refusal, neuron, flags);
    export_scan_bwd_plan(sp, M, out);
    return 0;
}

// Every reverse-scan launch.  fn: the entry point the messages name.  c_mem / c_syn / v0 / tau_partial (snn_lif_tau_bwd):
// per-channel time constants, the initial potential their sums start from, and where those sums go.
static int scan_bwd(const char* fn, int neuron, const float* g_out, int64_t ldg, const float* state, const float* y,
                    int64_t ldy, const float* g_vT, const float* g_iT, const float* alpha, const float* beta, int apply_scale,
                    float* gx, float* g_v0, float* g_i0, double* sums, int T, int64_t M, int C, const snn_neuron_params* p,
                    int flags, void* stream, const float* c_mem = nullptr, const float* c_syn = nullptr,
                    const float* v0 = nullptr, double* tau_partial = nullptr) {
    SNN_REQUIRE(g_out && gx && p, "%s: null pointer", fn);
    const ScanBwdPlan sp = scan_bwd_plan(neuron, T, M, C, ldg, ldy, sums != nullptr, p, flags,
                                         !c_mem ? kRuleDefault : tau_partial ? kRuleTauSums : kRuleTau);
    SNN_REQUIRE(!sp.refusal, "%s: %s (neuron %d, flags 0x%x)", fn, sp.refusal, neuron, flags);
    const bool reads_y = !sp.yf && (sums || rebuilds_x(neuron));
    if (sp.yf) {
        SNN_REQUIRE(state && !apply_scale, "%s: %s", fn, kSumsFromStateCovers);
        y = g_out;   // never read: the kernel's y operand only has to be a valid tensor
        ldy = ldg;
    } else {
        SNN_REQUIRE(!(neuron == SNN_NEURON_LIF || neuron == SNN_NEURON_LI_TANH || rebuilds_x(neuron)) || state,
                    "%s: saved state required", fn);
        SNN_REQUIRE(!reads_y || (y && ldy >= C), "%s: y required", fn);
        SNN_REQUIRE((alpha == nullptr) == (beta == nullptr), "%s: alpha/beta must come together", fn);
        SNN_REQUIRE(!apply_scale || alpha, "%s: apply_scale needs alpha", fn);
    }
    if (sp.pl.vec == 4) {   // 4 channels per access: 16 bytes of fp32, 8 of the bf16 activation tensors
        const bool ok = ldg % 4 == 0 && (!reads_y || ldy % 4 == 0) &&
                        aligned(sp.sb ? 8 : 16, {g_out, state, gx, reads_y ? y : nullptr}) &&
                        aligned(16, {g_vT, g_iT, alpha, beta, g_v0, g_i0, c_mem, c_syn, v0});
        SNN_REQUIRE(ok, "%s: %s", fn, sp.sb ? kBf16Covers : "buffers must be 16-byte aligned when C%4==0");
    }
    // SB, YF and the rule travel as ONE dispatched value: of their sixteen combinations seven have instances (bf16 storage
    // runs the default rule only, the from-state sums the first two rules), and every combination the dispatcher visits
    // costs compile time whether bwd_instance keeps it or not (with the whole scan family in one source: 190 s with three
    // values, 156 s with one; this file alone, as it is: 104 s).
    enum { kArmBf16 = kRuleTauSums + 1, kArmFromState, kArmFromStateGeneral };
    const int arm = sp.sb ? kArmBf16 : sp.yf ? kArmFromState + sp.rule : sp.rule;
    const bool launched = dispatch(
        [&](auto NEURON, auto VEC, auto MODE, auto BUF, auto NP, auto ARM) {
            constexpr bool SB = ARM() == kArmBf16, YF = ARM() >= kArmFromState;
            constexpr int RULE = SB ? kRuleDefault : YF ? ARM() - kArmFromState : ARM();
            constexpr bool GR = RULE >= kRuleGeneral, PC = RULE >= kRuleTau, TS = RULE == kRuleTauSums;
            if constexpr (bwd_instance(NEURON(), VEC(), MODE(), BUF(), NP(), SB, YF, GR, PC, TS)) {
                // (the instances without per-channel constants never read the five trailing arguments: NULL and 0 there)
                hipLaunchKernelGGL((k_affine_neuron_bwd<NEURON(), VEC(), MODE(), BUF(), NP(), SB, YF, GR, PC, TS>),
                                   dim3(sp.pl.gx, sp.pl.gy), dim3(kThreads), sp.lds_bytes, (hipStream_t)stream, g_out, ldg,
                                   state, y, ldy, g_vT, g_iT, alpha, beta, apply_scale, gx, g_v0, g_i0, sums, T, M, C,
                                   sp.pl.cvb, *p, sp.yf ? sp.lookback : sp.last_only, c_mem, c_syn, v0, tau_partial,
                                   sp.ordered ? 1 : 0);
                return true;
            } else {
                return false;
            }
        },
        AnyNeuron{neuron}, OneOf<1, 4>{sp.pl.vec}, OneOf<0, 1, 2>{sp.pl.mode}, Flag{sp.buf}, OneOf<1, 2, 3, kBwdNP>{sp.np},
        OneOf<0, 1, 2, 3, 4, 5, 6>{arm});
    SNN_REQUIRE(launched, "%s: no kernel instance (neuron %d, vec %d, mode %d, BUF %d, NP %d, GR %d)", fn, neuron, sp.pl.vec,
                sp.pl.mode, (int)sp.buf, sp.np, (int)(sp.rule != kRuleDefault));
    SNN_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int snn_affine_neuron_bwd(int neuron, const float* g_out, int64_t ldg, const float* state, const float* y,
                                     int64_t ldy, const float* g_vT, const float* g_iT, const float* alpha,
                                     const float* beta, int apply_scale, float* gx, float* g_v0, float* g_i0,
                                     double* sums, int T, int64_t M, int C, const snn_neuron_params* p,
                                     int flags, void* stream) {
    return scan_bwd("snn_affine_neuron_bwd", neuron, g_out, ldg, state, y, ldy, g_vT, g_iT, alpha, beta, apply_scale, gx, g_v0,
                    g_i0, sums, T, M, C, p, flags, stream);
}

// ---- LIF with per-channel time constants (c_mem[C], c_syn[C]) and their gradients
extern "C" int snn_lif_tau_param(const float* w_mem, const float* w_syn, int n, int C, float* c_mem, float* c_syn,
                                 void* stream) {
    SNN_REQUIRE(w_mem && w_syn && c_mem && c_syn, "snn_lif_tau_param: null pointer");
    SNN_REQUIRE(C > 0 && (n == 1 || n == C), "snn_lif_tau_param: n (%d) must be 1 or C (%d)", n, C);
    hipLaunchKernelGGL(k_lif_tau_param, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_mem, w_syn, n, C, c_mem,
                       c_syn);
    SNN_CHECK_LAUNCH("snn_lif_tau_param");
    return 0;
}

extern "C" size_t snn_lif_tau_bwd_partial_size(int T, int64_t M, int C, int with_sums) {
    if (T <= 0 || M <= 0 || C <= 0) return 0;
    return (size_t)bwd_plan(T, M, C, with_sums != 0).gx * C * 2;
}

// out[12]: the ten values of snn_affine_neuron_bwd_plan, then 1 when the two sums are combined in fixed order (0: LDS float
// atomics) and the LDS bytes of the launch
extern "C" int snn_lif_tau_bwd_plan(int neuron, int T, int64_t M, int C, int64_t ldg, int64_t ldy, int with_sums,
                                    int with_tau_sums, const snn_neuron_params* p, int flags, int64_t* out) {
    SNN_REQUIRE(out && p, "snn_lif_tau_bwd_plan: null pointer");
    const ScanBwdPlan sp =
        scan_bwd_plan(neuron, T, M, C, ldg, ldy, with_sums != 0, p, flags, with_tau_sums ? kRuleTauSums : kRuleTau);
    SNN_REQUIRE(!sp.refusal, "snn_lif_tau_bwd_plan: %s (neuron %d, flags 0x%x)", sp.refusal, neuron, flags);
    export_scan_bwd_plan(sp, M, out);
    out[10] = sp.ordered ? 1 : 0;
    out[11] = (int64_t)sp.lds_bytes;
    return 0;
}

extern "C" int snn_lif_tau_bwd(int neuron, const float* g_out, int64_t ldg, const float* state, const float* y, int64_t ldy,
                               const float* g_vT, const float* g_iT, const float* alpha, const float* beta, int apply_scale,
                               float* gx, float* g_v0, float* g_i0, double* sums, int T, int64_t M, int C,
                               const snn_neuron_params* p, const float* c_mem, const float* c_syn, const float* v0,
                               double* tau_partial, int flags, void* stream) {
    SNN_REQUIRE(g_out && gx && p && state && c_mem && c_syn, "snn_lif_tau_bwd: null pointer");
    return scan_bwd("snn_lif_tau_bwd", neuron, g_out, ldg, state, y, ldy, g_vT, g_iT, alpha, beta, apply_scale, gx, g_v0, g_i0,
                    sums, T, M, C, p, flags, stream, c_mem, c_syn, v0, tau_partial);
}

// per-block partials of snn_lif_tau_bwd -> dL/dw_mem, dL/dw_syn ([C], or [1] with per_layer), stored or accumulated
extern "C" int snn_lif_tau_finalize(const double* tau_partial, int T, int64_t M, int C, int with_sums, const float* c_mem,
                                    const float* c_syn, int per_layer, float* d_wmem, float* d_wsyn, int accumulate,
                                    void* stream) {
    SNN_REQUIRE(tau_partial && c_mem && c_syn && (d_wmem || d_wsyn), "snn_lif_tau_finalize: null pointer");
    SNN_REQUIRE(T > 0 && M > 0 && C > 0, "snn_lif_tau_finalize: bad shape");
    const int gx = bwd_plan(T, M, C, with_sums != 0).gx;
    constexpr int kFinWaves = 16;
    hipLaunchKernelGGL(k_lif_tau_finalize, dim3(per_layer ? 1 : (C + kFinWaves - 1) / kFinWaves), dim3(64 * kFinWaves), 0,
                       (hipStream_t)stream, tau_partial, gx, C, c_mem, c_syn, per_layer ? 1 : 0, d_wmem, d_wsyn, accumulate);
    SNN_CHECK_LAUNCH("snn_lif_tau_finalize");
    return 0;
}

// LIF backward from the checkpoints of snn_lif_fwd_ckpt; sums / outputs exactly as snn_affine_neuron_bwd(LIF)
extern "C" int snn_lif_bwd_ckpt(const float* g_out, int64_t ldg, const float* ckpt, const float* y, int64_t ldy,
                                const float* g_vT, const float* g_iT, const float* alpha, const float* beta,
                                int apply_scale, float* gx, float* g_v0, float* g_i0, double* sums, int T, int64_t M,
                                int C, const snn_neuron_params* p, void* stream) {
    SNN_REQUIRE(g_out && gx && p && ckpt && y, "snn_lif_bwd_ckpt: null pointer");
    SNN_REQUIRE(T > 0 && M > 0 && C > 0 && ldg >= C && ldy >= C, "snn_lif_bwd_ckpt: bad shape");
    SNN_REQUIRE((alpha == nullptr) == (beta == nullptr), "snn_lif_bwd_ckpt: alpha/beta must come together");
    SNN_REQUIRE(!apply_scale || alpha, "snn_lif_bwd_ckpt: apply_scale needs alpha");
    SNN_REQUIRE(p->surrogate == SNN_SURR_SUPER && p->reset_detached == 0,
                "snn_lif_bwd_ckpt: the checkpointed pair has the default gradient rule only (surrogate %d, reset_detached %d): "
                "use snn_affine_neuron_fwd / _bwd", p->surrogate, p->reset_detached);
    const BwdPlan pl = scan_bwd_plan(SNN_NEURON_LIF, T, M, C, ldg, ldy, sums != nullptr, p, 0).pl;   // (nothing left to refuse)
    SNN_REQUIRE(pl.vec == 1 || (multiples(4, {ldg, ldy}) && aligned(16, {g_out, ckpt, y, g_vT, g_iT, alpha, beta, gx, g_v0, g_i0})),
                "snn_lif_bwd_ckpt: buffers must be 16-byte aligned when C%%4==0");
    dispatch(
        [&](auto VEC, auto MODE) {
            hipLaunchKernelGGL((k_lif_bwd_ckpt<VEC(), MODE()>), dim3(pl.gx, pl.gy), dim3(kThreads), pl.lds_bytes,
                               (hipStream_t)stream, g_out, ldg, ckpt, y, ldy, g_vT, g_iT, alpha, beta, apply_scale, gx, g_v0,
                               g_i0, sums, T, M, C, pl.cvb, *p);
            return true;
        },
        OneOf<1, 4>{pl.vec}, OneOf<0, 1, 2>{pl.mode});
    SNN_CHECK_LAUNCH("snn_lif_bwd_ckpt");
    return 0;
}
