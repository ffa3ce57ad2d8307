// What the Norm -> neuron scan family shares (gfx950): the fused BatchNorm-apply + spiking-neuron temporal scan, forward
// and BPTT backward, with the BatchNorm statistics before it and the BatchNorm backward behind it.
//
//   bn_stats.hip   BatchNorm statistics (per-timestep sums, finalize, running update)
//   scan_fwd.hip   forward scan k_affine_neuron_fwd
//   scan_bwd.hip   reverse scan k_affine_neuron_bwd / k_lif_bwd_ckpt, the time constants' gradients
//   bn_bwd.hip     BatchNorm backward (reduce, coefficients, apply)
//
// Memory-bound kernels: one thread owns VEC(=4) consecutive channels of one pixel and walks the
// T timesteps with the membrane state (v, i) in registers; every HBM access is a 16-byte
// lane-contiguous vector.  Compiled with -ffp-contract=off so each statement rounds like the
// reference's unfused torch ops (oracle/neurons.py).
//
// Only what two or more of the four sources use lives here, and no kernels; everything has internal linkage.
#pragma once
#include <stdlib.h>
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;
#ifndef SNN_SCAN_NT_AUX
#define SNN_SCAN_NT_AUX 2   // cache-policy operand of the reverse scan's last-use loads (gfx950: bit 1 = nt)
#endif

template <int VEC> struct Vec;
template <> struct Vec<4> {
    typedef f32x4 type;
    static __device__ __forceinline__ f32x4 load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void store(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
};
// 8 channels per thread: the bf16-storage scans (16 bytes of bf16 per access; fp32 side tensors as two 16-byte halves)
typedef float f32x8 __attribute__((ext_vector_type(8)));
template <> struct Vec<8> {
    typedef f32x8 type;
    static __device__ __forceinline__ f32x8 load(const float* p) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ void store(float* p, f32x8 v) {
        *reinterpret_cast<f32x4*>(p) = __builtin_shufflevector(v, v, 0, 1, 2, 3);
        *reinterpret_cast<f32x4*>(p + 4) = __builtin_shufflevector(v, v, 4, 5, 6, 7);
    }
};
template <> struct Vec<1> {
    typedef float type;
    static __device__ __forceinline__ float load(const float* p) { return *p; }
    static __device__ __forceinline__ void store(float* p, float v) { *p = v; }
};
// activation tensors in the storage type (fp32, or bf16 in the bf16-storage mode: snn_common.h SnnStore): element index
template <int VEC, bool SB> struct VecS;
template <bool SB> struct VecS<4, SB> {
    static __device__ __forceinline__ f32x4 load(const float* base, int64_t i) { return SnnStore<SB>::ld4(base, i); }
    // the same for a tensor nobody reads again soon (non-temporal: what stays in L2 / the memory-side cache should be the
    // tensors that go from a producer straight to its consumer - conv -> scan -> conv, scan -> apply -> data gradient)
    static __device__ __forceinline__ f32x4 load_last(const float* base, int64_t i) {
        if constexpr (SNN_SCAN_NT_AUX == 0) return SnnStore<SB>::ld4(base, i);
        else if constexpr (SB) return snn_unpack_bf16x4(__builtin_nontemporal_load(
                                   reinterpret_cast<const snn_u32x2*>(reinterpret_cast<const unsigned short*>(base) + i)));
        else return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + i));
    }
    static __device__ __forceinline__ void store(float* base, int64_t i, f32x4 v) { SnnStore<SB>::st4(base, i, v); }
};
template <> struct VecS<8, true> {   // 8 bf16 values = 16 bytes
    static __device__ __forceinline__ f32x8 load(const float* base, int64_t i) {
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        const u32x4_ r = *reinterpret_cast<const u32x4_*>(reinterpret_cast<const unsigned short*>(base) + i);
        const f32x4 a = snn_unpack_bf16x4(snn_u32x2{r[0], r[1]}), b = snn_unpack_bf16x4(snn_u32x2{r[2], r[3]});
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ f32x8 load_last(const float* base, int64_t i) {
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        const u32x4_* src = reinterpret_cast<const u32x4_*>(reinterpret_cast<const unsigned short*>(base) + i);
        const u32x4_ r = SNN_SCAN_NT_AUX == 0 ? *src : __builtin_nontemporal_load(src);
        const f32x4 a = snn_unpack_bf16x4(snn_u32x2{r[0], r[1]}), b = snn_unpack_bf16x4(snn_u32x2{r[2], r[3]});
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    static __device__ __forceinline__ void store(float* base, int64_t i, f32x8 v) {
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        const snn_u32x2 a = snn_pack_bf16x4(__builtin_shufflevector(v, v, 0, 1, 2, 3));
        const snn_u32x2 b = snn_pack_bf16x4(__builtin_shufflevector(v, v, 4, 5, 6, 7));
        *reinterpret_cast<u32x4_*>(reinterpret_cast<unsigned short*>(base) + i) = u32x4_{a[0], a[1], b[0], b[1]};
    }
};
template <bool SB> struct VecS<1, SB> {
    static __device__ __forceinline__ float load(const float* base, int64_t i) { return SnnStore<SB>::ld1(base, i); }
    static __device__ __forceinline__ float load_last(const float* base, int64_t i) { return SnnStore<SB>::ld1(base, i); }
    static __device__ __forceinline__ void store(float* base, int64_t i, float v) { SnnStore<SB>::st1(base, i, v); }
};
template <int VEC> __device__ __forceinline__ float& lane(typename Vec<VEC>::type& v, int j);
template <> __device__ __forceinline__ float& lane<4>(f32x4& v, int j) { return reinterpret_cast<float*>(&v)[j]; }
template <> __device__ __forceinline__ float& lane<8>(f32x8& v, int j) { return reinterpret_cast<float*>(&v)[j]; }
template <> __device__ __forceinline__ float& lane<1>(float& v, int) { return v; }

// the checkpointed LIF pair: the forward scan (SAVE mode 2, scan_fwd.hip) saves the state before every kCkpt-th step, the
// backward scan from checkpoints (k_lif_bwd_ckpt, scan_bwd.hip) recomputes the steps of a chunk from it
constexpr int kCkpt = 4;

// ---- the reverse scan's block plan: the scan launches with it, the BatchNorm backward reads the scan's block partials by it
constexpr int kWaves = kThreads / 64;

struct BwdPlan {
    int vec, cvb, gy, gx, mode;  // mode 0: no sums, 1: ordered (shuffle + per-wave slabs), 2: LDS atomics
    size_t lds_bytes;
    int64_t rpb;                 // pixel rows per block
};

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// (Measured and rejected: a smaller slab budget - 32 / 16 KiB, more blocks of fewer channels - for the mid-size maps whose
// 64 KiB plan leaves CUs idle.  The 30x38 x 128-channel scan alone went 81 -> 59 us in isolation, but inside the step the
// family average rose from 98 to 125 us (bf16 storage) and 147 to 151 us (fp32): narrower channel runs per pixel and a
// second round of blocks on the small maps cost more than the shorter serial chains gain.)
static BwdPlan bwd_plan(int T, int64_t M, int C, bool with_sums) {
    constexpr int lds_kib = 64;
    BwdPlan pl;
    pl.vec = (C % 4 == 0) ? 4 : 1;
    int cv = C / pl.vec;
    int cvb = cv < kThreads ? cv : kThreads;
    pl.mode = 0;
    pl.lds_bytes = 0;
    if (with_sums) {
        const bool ordered = is_pow2(cvb) || cvb >= 64;
        pl.mode = ordered ? 1 : 2;
        const int slabs = ordered ? kWaves : 1;
        // LDS budget: slabs * T * cb * 2 floats
        int64_t max_cvb = ((int64_t)lds_kib * 1024) / ((int64_t)slabs * T * 8 * pl.vec);
        if (max_cvb < 1) max_cvb = 1;
        if (cvb > max_cvb) {
            cvb = (int)max_cvb;
            if (ordered) {  // keep a power of two
                int p2 = 1;
                while (p2 * 2 <= cvb) p2 *= 2;
                cvb = p2;
            }
        }
        pl.lds_bytes = (size_t)slabs * T * cvb * pl.vec * 2 * sizeof(float);
    }
    pl.cvb = cvb;
    pl.gy = (int)snn_ceil_div(cv, cvb);
    int P = kThreads / cvb;
    // Every block owns a contiguous run of pixel rows (P pixels each) of EQUAL length, processed kBwdNP rows at a
    // time with the tail masked: all blocks are resident at once and finish together.  (A grid-stride loop over
    // kBwdNP-row groups left e.g. 713 groups on 512 blocks: 2 rounds for 1.4 rounds of work.)
    const int64_t rows = snn_ceil_div(M, (int64_t)P);
    // blocks resident per CU by LDS (160 KiB per CU; 64 KiB slabs: 2, 32 KiB: 4, 16 KiB: 8 = the wave limit)
    int64_t cap = with_sums ? (int64_t)(128 / lds_kib) * snn_num_cu() : snn_max_blocks();
    if (const char* force = snn_tuning_env("SNN_BWD_CAP")) cap = atoi(force) > 0 ? atoi(force) : cap;  // tuning aid
    cap = cap / pl.gy;
    if (cap < 1) cap = 1;
    const int64_t rpb = snn_ceil_div(rows, rows < cap ? rows : cap);
    pl.gx = (int)snn_ceil_div(rows, rpb);
    pl.rpb = rpb;
    return pl;
}

using AnyNeuron = OneOf<(int)SNN_NEURON_NONE, (int)SNN_NEURON_LIF, (int)SNN_NEURON_LI, (int)SNN_NEURON_LI_TANH,
                        (int)SNN_NEURON_SLI, (int)SNN_NEURON_SYNAPSE>;

constexpr bool bf16_neuron(int n) {   // the neurons with a bf16-storage scan
    return n == SNN_NEURON_NONE || n == SNN_NEURON_LIF || n == SNN_NEURON_LI || n == SNN_NEURON_LI_TANH;
}
constexpr bool last_step_neuron(int n) { return n == SNN_NEURON_LIF || n == SNN_NEURON_LI || n == SNN_NEURON_LI_TANH; }
constexpr bool rebuilds_x(int n) { return n == SNN_NEURON_SLI || n == SNN_NEURON_SYNAPSE; }
const char* const kBf16Covers =
    "bf16 storage covers NONE / LIF / LI / LI+Tanh on channel counts and strides that are multiples of 4 (8-byte aligned "
    "tensors)";
const char* const kTauCovers =
    "per-channel time constants are for SNN_NEURON_LIF on fp32 tensors (no SNN_SCAN_BF16_STORAGE), with the y-reading scan "
    "(no SNN_SCAN_SUMS_FROM_STATE / SNN_SCAN_STATE_LOOKBACK)";

}  // namespace
