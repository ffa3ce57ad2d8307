// Fused BatchNorm-apply + spiking-neuron temporal scan, forward (gfx950).  Backward: scan_bwd.hip; what the two share:
// scan_common.h.
//
// Reference semantics: layer_gen.py:211-214 (BatchNorm2d, per-timestep batch statistics),
// layer_gen.py:232-235 / 252-254 (norse LIFCell / LICell), tiny_yolo.py:39-44 (LI -> Tanh).
#include "scan_common.h"

namespace {

// ------------------------------------------------------------------------------------------
// Forward scan
// ------------------------------------------------------------------------------------------
// SAVE: 0 nothing for the backward pass; 1 the per-step state (vdec); 2 (LIF) the state (v, i) BEFORE every kCkpt-th step
// into vdec = ckpt[chunk][2][M][C]: the backward scan recomputes the steps of a chunk from it (k_lif_bwd_ckpt) instead
// of reading one saved value per step.  Half the saved-state memory of mode 1 at the same speed (forward faster,
// backward slower by about as much); opt-in from functional.LIF_CHECKPOINT_BYTES.
#ifndef SNN_SCAN_PREFETCH
#define SNN_SCAN_PREFETCH 2   // steps of operands in flight ahead of the recurrence (forward scan)
#endif
// SB (SNN_SCAN_BF16_STORAGE): y, out, addend and vdec are bf16 tensors (pointers passed as float*, strides in elements)
// PC (LIF, fp32 tensors; snn_lif_tau_fwd): the two time constants are per-channel arrays cmem_pc[C] / csyn_pc[C] instead of
// the struct's scalars; a lane loads its VEC channels' pair once, before the time loop.  The other instances never read the
// two pointers.
template <int NEURON, int VEC, int SAVE, bool SB = false, bool PC = false>
__global__ __launch_bounds__(kThreads) void k_affine_neuron_fwd(
    const float* __restrict__ y, int64_t ldy, const float* __restrict__ alpha, const float* __restrict__ beta,
    const float* __restrict__ v0, const float* __restrict__ i0, float* __restrict__ out, int64_t ldo,
    const float* __restrict__ addend, int64_t ld_add, float* __restrict__ vT, float* __restrict__ iT,
    float* __restrict__ vdec, int T, int64_t M, int C, snn_neuron_params p, int last_only,
    const float* __restrict__ cmem_pc = nullptr, const float* __restrict__ csyn_pc = nullptr,
    uint32_t* __restrict__ mask = nullptr, int64_t ld_mask = 0) {
    // last_only (SNN_SCAN_LAST_STEP_ONLY): `out` is [M][ldo], only the last timestep's output is kept (the detection
    // head: soda.py:141-144 returns the predictions of the last step) - T-1 of T output stores never happen
    typedef typename Vec<VEC>::type V;
    static_assert(!SB || SAVE != 2, "the checkpointed scan keeps fp32 checkpoints: not combined with bf16 storage");
    static_assert(!PC || (NEURON == SNN_NEURON_LIF && !SB && SAVE != 2), "per-channel time constants: LIF on fp32 tensors");
    const int cv = C / VEC;
    const int64_t total = M * cv;
    for (int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x; col < total;
         col += (int64_t)gridDim.x * kThreads) {
        const int64_t m = col / cv;
        const int c = (int)(col % cv) * VEC;
        V v, i;
        [[maybe_unused]] V cmv, csv;
        if constexpr (PC) {
            cmv = Vec<VEC>::load(cmem_pc + c);
            csv = Vec<VEC>::load(csyn_pc + c);
        }
        if (NEURON != SNN_NEURON_NONE) {
            if (v0) v = Vec<VEC>::load(v0 + m * C + c);
            else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(v, j) = p.v_leak;
            }
            if (i0) i = Vec<VEC>::load(i0 + m * C + c);
            else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(i, j) = 0.0f;
            }
        }
        // The operands of a step - y, the BatchNorm affine (alpha, beta)[t][c], the shortcut - are requested kPrefetch steps
        // ahead of the recurrence and rotate through registers: with the loads inside the step every iteration waited for
        // its own alpha / beta loads (s_waitcnt vmcnt(0): a full memory latency per timestep, whatever was prefetched
        // before them).  Steps past the end re-read the last one.  The pipelined loop must be free of branches around its
        // memory operations (at a control-flow join the compiler's wait-count pass falls back to vmcnt(0)), so it exists
        // in the two forms the layer-major step uses - BatchNorm affine, all T outputs, with / without a shortcut - and
        // everything else (no affine, last step only) takes the plain loop with its run-time checks.
        auto time_loop = [&](auto piped_c, auto add_c, auto noout_c, auto last_c, auto mask_c) {
        constexpr bool PIPED = decltype(piped_c)::value;       // affine present, ADD known, outputs: all steps or (LAST) one
        // LAST (PIPED only; SNN_SCAN_LAST_STEP_ONLY, the detection heads' LI + Tanh): nothing is stored inside the loop, the
        // last step's output once behind it - the plain loop below waited for every step's own loads, 32 dependent memory
        // round trips (66 us for the 30x38 head at 2.9 TB/s)
        constexpr bool LAST = decltype(last_c)::value;
        constexpr bool ADD = decltype(add_c)::value;
        // NOOUT (SNN_SCAN_SPIKES_FROM_VDEC; LIF without a shortcut, v_dec saved): no output tensor at all - the consumer
        // forms the spikes itself, z = (v_dec > v_th), while it reads the saved potentials (snn_conv1x1_spikes_*)
        constexpr bool NOOUT = decltype(noout_c)::value;
        // MASK (NOOUT only; SNN_SCAN_SPIKE_MASK): the spikes z = (v_dec > v_th) additionally leave as one bit per neuron,
        // mask[t][m][c >> 5] bit c & 31 - what snn_conv1x1_mask_* read instead of 32 bits of potential.  A lane holds 4
        // channels, 8 neighbouring lanes (one pixel: C % 32 == 0, so a group of 8 never straddles a row or the tail of the
        // grid-stride loop) make one word: three DPP OR steps inside the group, then all 8 lanes store the same word to the
        // same address - no branch around the store (see above), and one wave instruction per 64 * 4 neurons.
        constexpr bool MASK = decltype(mask_c)::value;
        constexpr int kPrefetch = PIPED ? SNN_SCAN_PREFETCH : 0;
        struct StepOps { V x, a, b, ad; };
        auto fetch_step = [&](int t) {
            const int tc = t < T ? t : T - 1;
            const int64_t row = (int64_t)tc * M + m;
            StepOps o;
            o.x = VecS<VEC, SB>::load_last(y, row * ldy + c);   // (the convolution's output: next read in the backward pass)
            if (PIPED || alpha) {
                o.a = Vec<VEC>::load(alpha + (int64_t)tc * C + c);
                o.b = Vec<VEC>::load(beta + (int64_t)tc * C + c);
            }
            if (PIPED ? ADD : addend != nullptr) o.ad = VecS<VEC, SB>::load_last(addend, row * ld_add + c);   // (as y)
            return o;
        };
        StepOps sq[kPrefetch > 0 ? kPrefetch : 1];
        if constexpr (kPrefetch > 0) {
#pragma unroll
            for (int k = 0; k < kPrefetch; ++k) sq[k] = fetch_step(k);
        }
        [[maybe_unused]] V o_keep;
        for (int t = 0; t < T; ++t) {
            const int64_t row = (int64_t)t * M + m;
            if (SAVE == 2 && NEURON == SNN_NEURON_LIF && (t % kCkpt) == 0) {
                float* ck = vdec + ((int64_t)(t / kCkpt) * 2 * M + m) * C + c;
                Vec<VEC>::store(ck, v);
                Vec<VEC>::store(ck + M * C, i);
            }
            StepOps cur;
            if constexpr (kPrefetch > 0) {
                cur = sq[0];
#pragma unroll
                for (int k = 0; k + 1 < kPrefetch; ++k) sq[k] = sq[k + 1];
                sq[kPrefetch - 1] = fetch_step(t + kPrefetch);
            } else {
                cur = fetch_step(t);
            }
            V x = cur.x;
            if (PIPED || alpha) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(x, j) = lane<VEC>(x, j) * lane<VEC>(cur.a, j) + lane<VEC>(cur.b, j);
            }
            V o, vd;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float xj = lane<VEC>(x, j);
                if (NEURON == SNN_NEURON_NONE) {
                    lane<VEC>(o, j) = xj;
                } else {
                    float vj = lane<VEC>(v, j), ij = lane<VEC>(i, j);
                    if (NEURON == SNN_NEURON_SYNAPSE) {
                        const float tau = (xj > 0.0f) ? p.tau_sec : p.tau_dis;
                        const float p_new = vj + ((xj - vj) * tau) * p.dt;
                        float gsyn = p_new;
                        if (p.sigma != 0.0f) gsyn = (4.0f * p.sigma) * (p_new - p.sigma * (p_new * p_new));
                        lane<VEC>(v, j) = p_new;
                        lane<VEC>(o, j) = gsyn < 0.0f ? 0.0f : gsyn;
                        lane<VEC>(vd, j) = p_new;
                        continue;
                    }
                    float xin = xj;
                    if (NEURON == SNN_NEURON_SLI) {
                        xin = xj * (1.0f / (1.0f + expf(-(p.v_st - fabsf(vj)))));
                        lane<VEC>(vd, j) = vj;
                    }
                    float i_new = ij + xin;
                    float c_mem = p.c_mem, c_syn = p.c_syn;
                    if constexpr (PC) {
                        c_mem = lane<VEC>(cmv, j);
                        c_syn = lane<VEC>(csv, j);
                    }
                    float dv = c_mem * ((p.v_leak - vj) + i_new);
                    float v_dec = vj + dv;
                    float di = c_syn * i_new;
                    lane<VEC>(i, j) = i_new + di;
                    if (NEURON == SNN_NEURON_LIF) {
                        float u = v_dec - p.v_th;
                        float z = (u > 0.0f) ? 1.0f : 0.0f;
                        lane<VEC>(v, j) = (1.0f - z) * v_dec + z * p.v_reset;
                        lane<VEC>(o, j) = z;
                        lane<VEC>(vd, j) = v_dec;
                    } else {
                        lane<VEC>(v, j) = v_dec;
                        lane<VEC>(o, j) = (NEURON == SNN_NEURON_LI_TANH) ? tanhf(v_dec) : v_dec;
                    }
                }
            }
            if (PIPED ? ADD : addend != nullptr) {  // residual shortcut folded into the store
#pragma unroll
                for (int j = 0; j < VEC; ++j) lane<VEC>(o, j) += lane<VEC>(cur.ad, j);
            }
            if constexpr (LAST) {
                o_keep = o;   // stored once behind the loop (no branch around a memory operation inside it)
            } else if constexpr (!NOOUT) {
                if (PIPED || !last_only) VecS<VEC, SB>::store(out, row * ldo + c, o);
                else if (t == T - 1) VecS<VEC, SB>::store(out, m * ldo + c, o);
            }
            if (SAVE == 1 && (NEURON == SNN_NEURON_LIF || NEURON == SNN_NEURON_SLI || NEURON == SNN_NEURON_SYNAPSE)) {
                // (non-temporal where the access is one plain 16-byte store: nobody reads v_dec before the backward pass,
                // while `out` is the next convolution's operand and should be what stays in the caches)
                if constexpr (VEC == 4 && !SB && SNN_SCAN_NT_AUX != 0) __builtin_nontemporal_store(vd, reinterpret_cast<f32x4*>(vdec + row * C + c));
                else VecS<VEC, SB>::store(vdec, row * C + c, vd);
            }
            if constexpr (MASK && VEC == 4) {
                unsigned wd = 0;   // taken from the very values stored to vdec; strict comparison, like the consumers'
#pragma unroll
                for (int j = 0; j < VEC; ++j) wd |= (lane<VEC>(vd, j) > p.v_th ? 1u : 0u) << j;
                wd <<= (c & 31);
                wd |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)wd, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]: lane ^ 1
                wd |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)wd, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]: lane ^ 2
                wd |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)wd, 0x141, 0xf, 0xf, true);   // row_half_mirror: the other quad
                // (one lane of the 8 storing it, under a lane test, compiles to a branch and s_waitcnt vmcnt(0) at the loop top)
                mask[row * ld_mask + (c >> 5)] = wd;
            }
        }
        if constexpr (LAST) VecS<VEC, SB>::store(out, m * ldo + c, o_keep);
        };
        if constexpr (VEC > 1 && SAVE != 2) {
            if (alpha && !last_only) {
                constexpr std::true_type yes{};
                constexpr std::false_type no{};
                if (addend) time_loop(yes, yes, no, no, no);
                else if (SAVE == 1 && NEURON == SNN_NEURON_LIF && !SB && !PC && VEC == 4 && out == nullptr && mask != nullptr)
                    time_loop(yes, no, yes, no, yes);
                else if (SAVE == 1 && NEURON == SNN_NEURON_LIF && !SB && out == nullptr) time_loop(yes, no, yes, no, no);
                else time_loop(yes, no, no, no, no);
            } else if (alpha && last_only && !addend) {
                time_loop(std::true_type{}, std::false_type{}, std::false_type{}, std::true_type{}, std::false_type{});
            } else {
                time_loop(std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
            }
        } else {
            time_loop(std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
        }
        if (NEURON != SNN_NEURON_NONE) {
            if (vT) Vec<VEC>::store(vT + m * C + c, v);
            if (iT) Vec<VEC>::store(iT + m * C + c, i);
        }
    }
}

// ---------------------------------------------------------------------------------- host side: plans and dispatch
// ---- forward scan: which k_affine_neuron_fwd instance on which grid
struct FwdPlan {
    int vec, save;   // channels per access (1 / 4, bf16 tensors 4 / 8); SAVE of the kernel
    unsigned blocks;
};
// lanes: the widest channel group (1 / 4 / 8) the strides and pointers of the call allow in one access
static FwdPlan fwd_plan(int neuron, int64_t M, int C, int lanes, bool saves, bool ckpt) {
    FwdPlan fp;
    // 8 channels (16 bytes of bf16) per access when the layout allows: the scan is bound by the number of memory
    // instructions, not by their bytes (8-byte accesses: 3.3 TB/s of bf16 against 5.1 TB/s with fp32 tensors)
    static const bool no_v8 = snn_tuning_env("SNN_SCAN_NO_VEC8") != nullptr;   // tuning / bisecting aid
    fp.vec = (lanes == 8 && no_v8) ? 4 : lanes;   // (8 is offered for bf16 tensors only)
    const bool step_state = neuron == SNN_NEURON_LIF || rebuilds_x(neuron);   // the others save nothing per step
    fp.save = (saves && step_state) ? (ckpt ? 2 : 1) : 0;
    // every thread scans the same number of (pixel, channel group) items over all T (grid-stride, tail masked) and
    // all blocks are resident at once: a capped grid with 1.4 items per thread would run 2 rounds for 1.4 of work
    const int64_t total = M * (C / fp.vec);
    const int64_t per_thread = snn_ceil_div(total, (int64_t)snn_max_blocks() * kThreads);
    fp.blocks = (unsigned)snn_ceil_div(total, kThreads * per_thread);
    return fp;
}
constexpr bool fwd_instance(int neuron, int vec, int save, bool sb, bool pc = false) {
    if (pc && (neuron != SNN_NEURON_LIF || sb || save == 2)) return false;   // per-channel constants: fp32 LIF, plain scan
    return (sb ? (vec != 1 && bf16_neuron(neuron) && save != 2) : vec != 8) &&
           (save == 0 || neuron == SNN_NEURON_LIF || (save == 1 && rebuilds_x(neuron)));
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
static int neuron_fwd(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta, const float* v0,
                      const float* i0, float* out, int64_t ldo, const float* addend, int64_t ld_addend, float* vT,
                      float* iT, float* vdec, bool ckpt, int T, int64_t M, int C, const snn_neuron_params* p,
                      int flags, void* stream, const float* cmem_pc = nullptr, const float* csyn_pc = nullptr,
                      uint32_t* mask = nullptr, int64_t ld_mask = 0) {
    // cmem_pc / csyn_pc (snn_lif_tau_fwd, which has checked neuron and flags): per-channel time constants
    const bool pc = cmem_pc != nullptr;
    const char* const fn = pc ? "snn_lif_tau_fwd" : (mask ? "snn_affine_neuron_fwd_mask" : "snn_affine_neuron_fwd");   // the entry point the messages name
    SNN_REQUIRE((flags & ~(SNN_SCAN_LAST_STEP_ONLY | SNN_SCAN_BF16_STORAGE | SNN_SCAN_SPIKES_FROM_VDEC | SNN_SCAN_SPIKE_MASK)) == 0,
                "%s: unknown flags 0x%x", fn, flags);
    const bool with_mask = (flags & SNN_SCAN_SPIKE_MASK) != 0;   // the spikes also leave as one bit per neuron
    SNN_REQUIRE(with_mask == (mask != nullptr) && (!with_mask || !pc),
                "%s: SNN_SCAN_SPIKE_MASK comes with a mask buffer, through snn_affine_neuron_fwd_mask only", fn);
    const int last_only = (flags & SNN_SCAN_LAST_STEP_ONLY) != 0;
    const bool sb = (flags & SNN_SCAN_BF16_STORAGE) != 0;   // y, out, addend, vdec are bf16 tensors
    const bool no_out = (flags & SNN_SCAN_SPIKES_FROM_VDEC) != 0;   // no output tensor: the consumer thresholds vdec
    SNN_REQUIRE(y && p && (out || no_out), "%s: null pointer", fn);
    if (no_out) {
        SNN_REQUIRE(neuron == SNN_NEURON_LIF && vdec && !ckpt && !addend && !last_only && !sb && alpha && !out &&
                        multiples(4, {C, ldy}) && aligned(16, {y, vdec}),
                    "%s: SNN_SCAN_SPIKES_FROM_VDEC is for Norm -> LIF with saved potentials, no shortcut, "
                    "all T steps, fp32 tensors, 4-channel groups; out must be NULL", fn);
        ldo = C;   // (unused; keeps the checks below meaningful)
    }
    SNN_REQUIRE(!last_only || (last_step_neuron(neuron) && !addend),
                "%s: SNN_SCAN_LAST_STEP_ONLY is for LIF / LI / LI+Tanh without a shortcut", fn);
    SNN_REQUIRE(!addend || (ld_addend >= C && neuron != SNN_NEURON_LI_TANH),
                "%s: addend needs ld_addend >= C and is not allowed with LI_TANH", fn);
    SNN_REQUIRE(T > 0 && M > 0 && C > 0 && ldy >= C && ldo >= C, "%s: bad shape", fn);
    SNN_REQUIRE((alpha == nullptr) == (beta == nullptr), "%s: alpha/beta must come together", fn);
    SNN_REQUIRE(neuron >= SNN_NEURON_NONE && neuron <= SNN_NEURON_SYNAPSE, "%s: bad neuron %d", fn,
                neuron);
    // n channels per access: the activation tensors (bf16: 2 bytes per element) and the fp32 per-pixel / per-channel ones
    auto lanes_ok = [&](int n, size_t act_bytes) {
        return multiples(n, {C, ldy, ldo, addend ? ld_addend : 0}) && aligned(act_bytes, {y, out, vdec, addend}) &&
               aligned(16, {alpha, beta, v0, i0, vT, iT, cmem_pc, csyn_pc});
    };
    SNN_REQUIRE(!sb || (lanes_ok(4, 8) && !ckpt && bf16_neuron(neuron)), "%s: %s, without checkpointing", fn, kBf16Covers);
    const int lanes = sb ? (lanes_ok(8, 16) ? 8 : 4) : (lanes_ok(4, 16) ? 4 : 1);
    SNN_REQUIRE(!with_mask || (no_out && C % 32 == 0 && ld_mask >= C / 32 && aligned(4, {mask}) && lanes == 4),
                "%s: SNN_SCAN_SPIKE_MASK needs SNN_SCAN_SPIKES_FROM_VDEC, C a multiple of 32, ld_mask >= C / 32 and 16-byte "
                "aligned operands", fn);
    const FwdPlan fp = fwd_plan(neuron, M, C, lanes, vdec != nullptr, ckpt);
    const bool launched = dispatch(
        [&](auto NEURON, auto VEC, auto SAVE, auto SB, auto PC) {
            if constexpr (fwd_instance(NEURON(), VEC(), SAVE(), SB(), PC())) {
                hipLaunchKernelGGL((k_affine_neuron_fwd<NEURON(), VEC(), SAVE(), SB(), PC()>), dim3(fp.blocks), dim3(kThreads), 0,
                                   (hipStream_t)stream, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld_addend, vT, iT,
                                   vdec, T, M, C, *p, last_only, cmem_pc, csyn_pc, mask, ld_mask);
                return true;
            } else {
                return false;
            }
        },
        AnyNeuron{neuron}, OneOf<1, 4, 8>{fp.vec}, OneOf<0, 1, 2>{fp.save}, Flag{sb}, Flag{pc});
    SNN_REQUIRE(launched, "%s: no kernel instance (neuron %d, vec %d, save %d)", fn, neuron, fp.vec, fp.save);
    SNN_CHECK_LAUNCH(fn);
    return 0;
}

extern "C" int snn_affine_neuron_fwd(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta,
                                     const float* v0, const float* i0, float* out, int64_t ldo, const float* addend,
                                     int64_t ld_addend, float* vT, float* iT, float* vdec, int T, int64_t M, int C,
                                     const snn_neuron_params* p, int flags, void* stream) {
    return neuron_fwd(neuron, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld_addend, vT, iT, vdec, false, T, M, C, p,
                      flags, stream);
}

// the same scan; with SNN_SCAN_SPIKE_MASK (and SNN_SCAN_SPIKES_FROM_VDEC) it also writes the spike bit mask (include/snn_hip.h)
extern "C" int snn_affine_neuron_fwd_mask(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta,
                                          const float* v0, const float* i0, float* out, int64_t ldo, const float* addend,
                                          int64_t ld_addend, float* vT, float* iT, float* vdec, int T, int64_t M, int C,
                                          const snn_neuron_params* p, int flags, void* stream, uint32_t* mask,
                                          int64_t ld_mask) {
    SNN_REQUIRE(((flags & SNN_SCAN_SPIKE_MASK) != 0) == (mask != nullptr),
                "snn_affine_neuron_fwd_mask: SNN_SCAN_SPIKE_MASK and the mask buffer come together");
    return neuron_fwd(neuron, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld_addend, vT, iT, vdec, false, T, M, C, p,
                      flags, stream, nullptr, nullptr, mask, ld_mask);
}

extern "C" int snn_lif_ckpt_interval(void) { return kCkpt; }

extern "C" int snn_lif_fwd_ckpt(const float* y, int64_t ldy, const float* alpha, const float* beta, const float* v0,
                                const float* i0, float* out, int64_t ldo, const float* addend, int64_t ld_addend,
                                float* vT, float* iT, float* ckpt, int T, int64_t M, int C, const snn_neuron_params* p,
                                void* stream) {
    SNN_REQUIRE(ckpt, "snn_lif_fwd_ckpt: null checkpoint buffer");
    return neuron_fwd(SNN_NEURON_LIF, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld_addend, vT, iT, ckpt, true, T, M,
                      C, p, 0, stream);
}

// the forward scan with per-channel time constants (c_mem[C], c_syn[C]); their parametrisation and gradients: scan_bwd.hip
extern "C" int snn_lif_tau_fwd(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta,
                               const float* v0, const float* i0, float* out, int64_t ldo, const float* addend,
                               int64_t ld_addend, float* vT, float* iT, float* vdec, int T, int64_t M, int C,
                               const snn_neuron_params* p, const float* c_mem, const float* c_syn, int flags, void* stream) {
    SNN_REQUIRE(neuron == SNN_NEURON_LIF && !(flags & SNN_SCAN_BF16_STORAGE), "snn_lif_tau_fwd: %s (neuron %d, flags 0x%x)",
                kTauCovers, neuron, flags);
    SNN_REQUIRE(c_mem && c_syn, "snn_lif_tau_fwd: null time constants");
    // (the forward scan addresses with 64-bit pointers whatever the flag says)
    return neuron_fwd(neuron, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld_addend, vT, iT, vdec, false, T, M, C, p,
                      flags & ~SNN_SCAN_WIDE_ADDRESSING, stream, c_mem, c_syn);
}
