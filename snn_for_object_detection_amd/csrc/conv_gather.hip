// Implicit-GEMM 2-D convolution on the gfx950 matrix cores, LDS-tiled, channels-last, all T*B frames of a layer
// in one launch.  Tensors are fp32 in HBM and accumulation is fp32; the PRODUCTS run on the 16-bit matrix pipe from
// pieces of the fp32 operands (split on the way into LDS), selected per call by the `precision` argument
// (include/snn_hip.h, SNN_PREC_*): fp16 x 3 (default forward: v_mfma_f32_32x32x16_f16, fp32-grade), bf16 x 6
// (fp32-grade for any range), bf16 x 3 (default backward: v_mfma_f32_32x32x16_bf16, rel 1e-5), or the exact fp32
// MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain).
//
// Replaces nn.Conv2d(bias=False, padding=int(k/2)) forward and ATen's conv backward
// (reference layer_gen.py:129-136) for the layer-major schedule.
//
//   forward / data-gradient ("gather conv", one kernel, two pixel mappings):
//       out[m][n] = sum_k A[m][k] * Wk[n][k]
//       m = output pixel (img, oy, ox); k = (tap, c); n = output channel
//       FWD  : A = x [img][oy*s-pad+kh][ox*s-pad+kw][c],             Wk = w  [Cout][taps][Cin]
//       DGRAD: A = dy[img][(oy+pad-kh)/s][(ox+pad-kw)/s][c] (exact), Wk = wt [Cin][taps][Cout]
//     block tile 128 pixels x BN channels x 32 k, 4 waves; LDS images of 16-bit pieces, [row][32+8] with an 80-byte
//     pitch read with ds_read_b128 (fp32 mode: [row][32+4] floats); software-pipelined main loop (convert tile k+1
//     in the MFMA shadow of tile k, loads of tile k+2 in flight); the data gradient of a strided conv is split
//     into stride x stride phase classes that only visit reachable taps; the epilogue can add up to two
//     same-shaped tensors (fused gradient accumulation).
//   weight gradient: conv_wgrad.hip; the event-frame layer (Cin = 2): conv_first.hip; what the three share: conv_common.h
//
// The split modes keep the 1e-4 parity target against the CPU reference: see DESIGN.md section 3 for the measured
// errors of each mode.
#include <stdlib.h>
#include <type_traits>
#include "conv_common.h"

#if defined(SNN_STAMP) || defined(SNN_CLOCK)
// tuning aid (scratch builds only).  -DSNN_CLOCK: shader-clock and 100 MHz wall-clock stamps at the begin and end of
// every block of k_conv_gather (the in-kernel clock under load, tools/clock_conv.py); -DSNN_STAMP additionally the
// per-phase cycle totals of wave 0 of the first 2048 blocks of the pipelined loop (tools/stamp_conv.py; costs ~10 %)
__device__ unsigned long long g_stamps[2048 * 8];
__device__ unsigned long long g_stamps2[2048 * 4];
extern "C" int snn_debug_stamps(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * n);
}
extern "C" int snn_debug_stamps2(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps2), sizeof(unsigned long long) * n);
}
#endif
#ifdef SNN_STAMP
#define STAMP(i) do { unsigned long long t_ = __builtin_readcyclecounter(); st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define STAMP(i) do {} while (0)
#endif

namespace {

constexpr int BM = 128;  // output pixels per block
constexpr int BK = 32;   // k elements per LDS stage
constexpr int LDK = BK + 4;
constexpr int LDB = BK + 8;  // bf16 row stride of the split-precision LDS images: 80 B keeps ds_read_b128 conflict-free
#ifndef SNN_GATHER_SB_WAVES
#define SNN_GATHER_SB_WAVES 3   // waves per SIMD the bf16-storage FORWARD instances of the pipelined kernel are compiled for
                                // (same-call A/B: 2 -> 3 waves 88 -> 79 us; 4 spills 13 registers, 80 us); the data-gradient
                                // instances (no statistics) fit 4 waves: 88 -> 81 us
#endif

struct ConvGeom {
    int64_t Mtot;      // GEMM rows: img * OH * OW (FWD) or img * OHc * OWc (DGRAD, one stride-phase class)
    int IH, IW, IC;    // gathered tensor
    int OH, OW, OC;    // produced tensor
    int KH, KW, stride, pad;
    int64_t ldi, ldo;
    int Ktot;          // k extent of this launch: KH*KW*IC (FWD) or nkh*nkw*IC (DGRAD class)
    int KtotFull;      // row length of the weight matrix: KH*KW*IC
    // DGRAD only.  Output pixels (hi, wi) with hi % stride == ph, wi % stride == pw form one class; only the
    // taps kh = kh0 + stride*jh (jh < nkh), kw = kw0 + stride*jw (jw < nkw) reach them, with source pixel
    // iy = (hi + pad - kh0)/stride - jh (exact).  For stride 1 there is a single class with every tap.
    int ph, pw, kh0, kw0, nkh, nkw, OHc, OWc;
    // ceil(2^32 / d) for d = IC and d = (DGRAD ? nkw : KW): q = umulhi(n, magic) == n / d for n * d < 2^32
    unsigned magic_ic, magic_kw;
    int out_vec;  // output (and addend) rows may be stored 16 bytes per lane
    int nimg;     // images in the gathered tensor (FAST loader: extent of its buffer resource)
    int mtiles, mtiles_per_xcd, ntiles;  // XCD-aware tile order (see k_conv_gather)
    // FWD only: statistics partials of the BatchNorm that follows (null: none), see stat_flush below
    double* bn_partial;
    int64_t bn_rows;   // output pixels per timestep (>= BM: a row tile meets at most two timesteps)
    int bn_chunks;     // chunk slots per timestep
    float x_th;        // XSP kernels: the gathered tensor holds saved LIF potentials, the operand is z = (v_dec > x_th)
};

// ---- BatchNorm statistics out of a forward epilogue.  The separate pass (snn_bn_stats) re-reads the whole layer
// output from HBM; the epilogue has every value in registers on its way to the store.  Layout of the partials is the
// one snn_bn_stats_finalize reads: partial[t][c][chunk][2] = (sum y, sum y^2) in fp64, a chunk being whatever set of
// pixels of timestep t one block (tile) owns.  The MFMA accumulator layout already is "one channel per lane": lane
// (r, h) of wave (wm, wn) holds channel (wn*TN + j)*32 + r of the 16 rows (wm*TM + i)*32 + (e&3) + 8*(e>>2) + 4*h,
// so a lane sums its own registers, the two half-waves are added by one shuffle and the WM waves through LDS, in
// that fixed order: deterministic, run to run.  (A convolution with statistics takes no addend: the sums are of the
// accumulators, which then are the stored values.)
//
// red: 4 * TN * 32 * 2 doubles of LDS, free to use; dst: the [C][2] slot of this block's chunk.  Block-uniform call.
template <int WM, int WN, int TN>
__device__ __forceinline__ void stat_flush(double (&s)[TN], double (&q)[TN], double* red, double* __restrict__ partial,
                                           int64_t step, int64_t chunk, int64_t chunks, int n0, int OC, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        s[j] += __shfl_xor(s[j], 32, 64);
        q[j] += __shfl_xor(q[j], 32, 64);
        if (lane < 32) {
            red[((wave * TN + j) * 32 + lane) * 2 + 0] = s[j];
            red[((wave * TN + j) * 32 + lane) * 2 + 1] = q[j];
        }
    }
    __syncthreads();
    if (tid < WN * TN * 32) {
        const int wn = tid / (TN * 32), jr = tid % (TN * 32);
        double ss = 0.0, qq = 0.0;
#pragma unroll
        for (int wm = 0; wm < WM; ++wm) {
            const double* src = red + (((wm * WN + wn) * TN) * 32 + jr) * 2;
            ss += src[0];
            qq += src[1];
        }
        if (n0 + tid < OC) {
            double* dst = partial + snn_bn_partial_index(step, chunk, n0 + tid, chunks, OC);
            dst[0] = ss;
            dst[1] = qq;
        }
    }
    __syncthreads();
}

// SPLIT = 0: exact fp32 MFMA (v_mfma_f32_32x32x2_f32): an fmaf chain, the reference arithmetic.
// SPLIT = 2: "bf16 x 3": every fp32 operand is split on the way into LDS into hi = bf16(x) and
//   lo = bf16(x - hi); the product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
//   (relative error ~2^-16 per product instead of 2^-24, at 16/3 of the fp32 matrix rate).  Default for the
//   data gradient, where a 1e-5 relative error is far inside the gradient tolerance.
// SPLIT = 4: "fp16 x 3": x = h + l with fp16 pieces (11 + 11 significant bits), products hh + hl + lh on
//   v_mfma_f32_32x32x16_f16: relative error 2^-22, fp32-grade like bf16 x 6 at HALF its matrix work and two LDS
//   images instead of three.  fp16 has the range for forward values (|x| < 65504; activations of a normalised
//   spiking net are O(1), weights are pre-scaled by 2^8), not for gradients - the backward kernels stay on bf16.
// SPLIT = 5: "bf16 x 1": the opt-in THROUGHPUT mode - every operand is rounded once to bf16 (8 significant bits) and
//   multiplied as it is: one product, fp32 accumulation and storage.  Not a parity mode (relative error 2^-9 per
//   product); tolerance stated in tests/test_gpu_bf16_mode.py.
// SPLIT = 3: "bf16 x 6": three-way split x = h + m + l (24 significant bits, i.e. the fp32 value itself) and the
//   six products hh + hm + mh + mm + hl + lh; the dropped terms are 2^-25 relative - fp32-grade accuracy at
//   16/6 of the fp32 matrix rate.
// FAST (host-checked: VEC, IC % 32 == 0, <= 31 taps, 4 images of the gathered tensor < 2 GiB): a k-step of 32 lies
// inside ONE filter tap, so the tap decode is scalar (SALU) and a row's address is "row offset + scalar tap
// offset".  Loads are raw buffer loads relative to the block's first image; padding / out-of-range rows get the
// offset 0xFFFFFFFF and the hardware range check returns zeros - no clamps, no value selects, no 64-bit address
// arithmetic in the loop (the generic loader spends more VALU cycles on addresses than the MFMAs take).
// PRESPLIT (FAST, SPLIT 2 or 4 only): `wk` is not the fp32 weight matrix but its pre-split image (snn_weight_presplit:
// per 4 consecutive k, 4 hi pieces then 4 lo pieces - the same 16 bytes at the same offsets), written once per optimiser
// step; the loader is unchanged and the per-block conversion of the weight tile (half of the conversion VALU of a
// k-step, repeated by every one of the ~1 400 blocks of a launch) disappears.  Same bits as converting on the fly.
// SB (FAST, SPLIT 5 only; SNN_PREC_BF16S, the bf16-STORAGE throughput mode): `in`, `out` and the addends are bf16 tensors
// (strides in elements).  The gathered rows arrive as 8-byte loads and go to LDS as they are - no conversion; the
// epilogue rounds the fp32 accumulators to bf16 on their way out.  Weights stay fp32 and are rounded in the loader.
// XSP (FAST, forward, SPLIT 4 only; snn_conv1x1_spikes_fwd): `in` holds the pre-reset potentials v_dec a LIF layer saved for
// its backward pass, NOT its output - that layer wrote no spike tensor at all (SNN_SCAN_SPIKES_FROM_VDEC) and the operand
// is formed here, z = (v_dec > x_th), on the way into LDS.  A spike is exact in ONE fp16 piece (16.0 or 0 after the 2^4
// pre-scale): no low image is written or read and the product low(x) * high(w) - identically zero - is not issued: two
// MFMA products per multiply-add, same bits as the three-product kernel fed the stored spikes.
// XM (XSP only; snn_conv1x1_mask_fwd, 1x1 / stride 1): `in` is the spike BIT MASK the scan wrote next to the potentials
// (SNN_SCAN_SPIKE_MASK): uint32 [pixel][ldi], bit c & 31 of word c >> 5.  A 32-channel k-step of a pixel is ONE dword: lane
// (r, h) loads the word of its own fragment row - one 4-byte load instruction per wave and 32 pixels, against four 16-byte
// ones - and expands byte 2 * ks + h of it into its 8 fp16 values (0x4C00 or 0) in registers.  No A image in LDS, nothing of
// A is written or read there; the MFMAs, their operands' bits and their order are those of XSP.
template <int BN, int WM, int WN, bool DGRAD, bool VEC, int SPLIT, bool FAST, bool PRESPLIT = false, bool SB = false,
          bool XSP = false, bool XM = false>
__global__ __launch_bounds__(kThreads, (FAST && SPLIT) ? (PRESPLIT ? 3 : (SB ? (DGRAD ? 4 : SNN_GATHER_SB_WAVES) : 2)) : SNN_CONV_MIN_WAVES) void k_conv_gather(const float* __restrict__ in, const float* __restrict__ wk,
                                                          float* __restrict__ out, ConvGeom g,
                                                          const float* __restrict__ addend, int64_t ld_add,
                                                          const float* __restrict__ addend2, int64_t ld_add2) {
    constexpr int TM = BM / WM / 32;
    constexpr int TN = BN / WN / 32;
    constexpr int BROWS = BN / 32;  // B rows loaded per thread
    static_assert(WM * WN == 4, "4 waves");
    static_assert(!SB || (FAST && SPLIT == 5 && !PRESPLIT), "bf16 storage: the pipelined one-product kernel");
    static_assert(!XSP || (FAST && SPLIT == 4 && !DGRAD && !PRESPLIT && !SB), "spikes from potentials: fp16 x 3 forward");
    static_assert(!XM || XSP, "spike bit mask: an instance of the spikes-from-potentials kernel");
    constexpr int ES = SB ? 2 : 4;   // bytes per activation element in HBM
    constexpr int NPIECE = SPLIT == 3 ? 3 : (SPLIT == 5 ? 1 : 2);  // 16-bit images per operand
    constexpr int A_BYTES = SPLIT ? NPIECE * BM * LDB * 2 : BM * LDK * 4;
    constexpr int B_BYTES = SPLIT ? NPIECE * BN * LDB * 2 : BN * LDK * 4;
    constexpr int STAGE_BYTES = 4 * 32 * (TN * 32 + 4) * 4;   // epilogue: 32 staged rows per wave (see below)
    constexpr int SMEM_BYTES = A_BYTES + B_BYTES > STAGE_BYTES ? A_BYTES + B_BYTES : STAGE_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES];
    float* As = reinterpret_cast<float*>(smem);
    float* Bs = reinterpret_cast<float*>(smem + A_BYTES);
    __bf16* Ah = reinterpret_cast<__bf16*>(smem);                 // [BM][LDB] high parts
    __bf16* Al = Ah + BM * LDB;                                   // [BM][LDB] low parts
    __bf16* Am = Al + BM * LDB;                                   // [BM][LDB] middle parts (SPLIT == 3)
    __bf16* Bh = reinterpret_cast<__bf16*>(smem + A_BYTES);
    __bf16* Bl = Bh + BN * LDB;
    __bf16* Bm = Bl + BN * LDB;

    const int tid = threadIdx.x;
#if defined(SNN_STAMP) || defined(SNN_CLOCK)
    const unsigned long long st_kernel_begin = __builtin_amdgcn_s_memtime();
    const unsigned long long st_real_begin = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane_id = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane_id & 31, h = lane_id >> 5;

    // XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs (each with its own 4 MiB L2): ids
    // L, L+8, L+16, ... run on one XCD.  XCD x gets the x-th CONTIGUOUS eighth of the pixel tiles (and all channel
    // tiles of a pixel tile back to back), so the blocks resident together on an XCD cover neighbouring image rows
    // and the 3x3 taps that reach into the rows above / below hit that XCD's L2.  With the plain order every XCD
    // held scattered 128-pixel segments and re-fetched the neighbouring rows from HBM (PMC: the 32-channel 3x3
    // data gradient read its input 5x).
    const int bid_xcd = blockIdx.x & 7, bid_q = blockIdx.x >> 3;
    const int bid_n = bid_q % g.ntiles;
    const int64_t bid_m = (int64_t)bid_xcd * g.mtiles_per_xcd + bid_q / g.ntiles;
    if (bid_m >= g.mtiles) return;  // padding block of the last XCD share (whole block, before any barrier)
    const int64_t m0 = bid_m * BM;
    const int n0 = bid_n * BN;

    // ---- per-thread loader geometry: rows lr + 32*j, k offset kq
    // Rows are permuted so that the two rows written by one 16-lane LDS store group lie 4 rows (320 B) apart: with
    // the 80-byte row pitch adjacent rows would overlap by 4 banks (measured: a third of all LDS cycles were
    // bank conflicts); 16 dwords apart modulo 32 banks they tile the banks exactly.
    const int lrr = tid >> 3;
    const int lr = ((lrr >> 1) & 3) + 4 * (lrr & 1) + 8 * (lrr >> 3), kq = (tid & 7) * 4;
    int a_y0[4], a_x0[4];
    int a_base[4];  // first pixel of the image (the host checks img * IH * IW < 2^31)
    bool a_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // 32-bit arithmetic (the host checks Mtot < 2^31): a 64-bit division costs ~10x a 32-bit one, and the
        // 13 of them per thread made the prologue 14 % of a block's lifetime (measured with s_memtime stamps)
        const unsigned m = (unsigned)m0 + lr + 32 * j;
        a_ok[j] = m < (unsigned)g.Mtot;
        const unsigned mm = a_ok[j] ? m : 0u;
        const unsigned ow_ = DGRAD ? g.OWc : g.OW, oh_ = DGRAD ? g.OHc : g.OH;
        const unsigned t = mm / ow_;
        const int ox = (int)(mm - t * ow_);
        const unsigned img = t / oh_;
        const int oy = (int)(t - img * oh_);
        a_base[j] = (int)(img * (unsigned)(g.IH * g.IW));
        if (!DGRAD) {
            a_y0[j] = oy * g.stride - g.pad;
            a_x0[j] = ox * g.stride - g.pad;
        } else if (g.stride == 1) {
            a_y0[j] = oy + g.pad;  // stride 1: ph = pw = kh0 = kw0 = 0
            a_x0[j] = ox + g.pad;
        } else {
            a_y0[j] = (int)((unsigned)(oy * g.stride + g.ph + g.pad - g.kh0) / (unsigned)g.stride);
            a_x0[j] = (int)((unsigned)(ox * g.stride + g.pw + g.pad - g.kw0) / (unsigned)g.stride);
        }
    }

    // k index -> (source pixel offset, weight column)
    auto decode_k = [&](int kk, int& dy, int& dx, int& c, int& wcol) {
        int tap = div_magic(kk, g.IC, g.magic_ic);
        c = kk - tap * g.IC;
        if (!DGRAD) {
            int kh = div_magic(tap, g.KW, g.magic_kw), kw = tap - kh * g.KW;
            dy = kh;
            dx = kw;
            wcol = kk;
        } else {
            int jh = div_magic(tap, g.nkw, g.magic_kw), jw = tap - jh * g.nkw;
            dy = -jh;
            dx = -jw;
            wcol = ((g.kh0 + g.stride * jh) * g.KW + (g.kw0 + g.stride * jw)) * g.IC + c;
        }
    };

    // A rows on their way to LDS: 4 fp32 values, or (SB) 4 bf16 values as two dwords.  (Integer-typed on purpose: carried
    // in float lanes and bit-cast back element by element, hipcc 7.2 narrows the 8-byte buffer load to 4 bytes.)
    // XM: one mask word per fragment row (TM of the 4 slots are used)
    using AReg = typename std::conditional<SB, u32x2, typename std::conditional<XM, unsigned, f32x4>::type>::type;
    AReg ra[4];
    f32x4 rb[BROWS];

    // ---- FAST loader state
    __amdgpu_buffer_rsrc_t rs_a, rs_b;
    int a_rel[4];            // byte offset of (row pixel origin, channel kq) from the block's first image
    unsigned a_mask[4];      // bit t: tap t of this row reads inside the image
    unsigned b_rel[BROWS];   // byte offset of (weight row, column kq); >= 2^31 for rows past OC
    [[maybe_unused]] int xm_rel[TM];   // XM: byte offset of the mask row of fragment row (wm * TM + i) * 32 + r; -1 past Mtot
    if constexpr (XM) {
        // the whole mask is one buffer (host-checked: Mtot * ldi * 4 < 2^31)
        rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, (int)(g.Mtot * g.ldi * 4), 0x00020000);
        rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wk), 0, g.OC * g.KtotFull * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int64_t m = m0 + (wm * TM + i) * 32 + r;
            xm_rel[i] = m < g.Mtot ? (int)(m * g.ldi * 4) : -1;
        }
#pragma unroll
        for (int j = 0; j < BROWS; ++j) {
            const int n = n0 + lr + 32 * j;
            b_rel[j] = n < g.OC ? (unsigned)(n * g.KtotFull + kq) * 4u : 0x80000000u;
        }
    } else if (FAST) {
        const int ow_ = DGRAD ? g.OWc : g.OW, oh_ = DGRAD ? g.OHc : g.OH;
        const int64_t img0 = (unsigned)m0 / (unsigned)(oh_ * ow_);
        const int64_t ipix = (int64_t)g.IH * g.IW;
        const int64_t bytes = ((((int64_t)g.nimg - img0) * ipix - 1) * g.ldi + g.IC) * ES;
        rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(in) + img0 * ipix * g.ldi * ES), 0,
                                                 bytes > 0xffffffffLL ? (int)0xffffffffu : (int)(unsigned)bytes,
                                                 0x00020000);
        rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wk), 0, g.OC * g.KtotFull * 4, 0x00020000);
        const int tw_n = DGRAD ? g.nkw : g.KW;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int relpix = (a_base[j] - (int)(img0 * ipix)) + a_y0[j] * g.IW + a_x0[j];
            a_rel[j] = (relpix * (int)g.ldi + kq) * ES;
            // bit (th * ntw + tw) = tap inside the image: row validity x column validity, branch-free (the taps of a
            // FAST launch are at most 5 x 5: ntaps <= 31)
            const int nth = DGRAD ? g.nkh : g.KH;
            unsigned xm = 0, mask = 0;
#pragma unroll
            for (int tw = 0; tw < 6; ++tw) {
                const int ix = DGRAD ? a_x0[j] - tw : a_x0[j] + tw;
                xm |= (tw < tw_n && (unsigned)ix < (unsigned)g.IW) ? 1u << tw : 0u;
            }
#pragma unroll
            for (int th = 0; th < 6; ++th) {
                const int iy = DGRAD ? a_y0[j] - th : a_y0[j] + th;
                mask |= (th < nth && (unsigned)iy < (unsigned)g.IH) ? xm << (th * tw_n) : 0u;
            }
            a_mask[j] = a_ok[j] ? mask : 0u;
        }
#pragma unroll
        for (int j = 0; j < BROWS; ++j) {
            const int n = n0 + lr + 32 * j;
            b_rel[j] = n < g.OC ? (unsigned)(n * g.KtotFull + kq) * 4u : 0x80000000u;
        }
    }
    const unsigned fast_tw_n = DGRAD ? g.nkw : g.KW;
    const unsigned fast_tw_one = fast_tw_n == 1 ? 1u : 0u;  // magic_u32(1) is 0: q = umulhi(n, 0) + n
    // which = 1: the A rows, 2: the B rows, 3: both
    auto load_tiles_fast = [&](int k0n, AReg (&ra)[4], f32x4 (&rb)[BROWS], int which = 3) {  // k0n is block-uniform: everything up to the per-row adds is scalar
        const bool kin = k0n < g.Ktot;
        const int tap = (int)__umulhi((unsigned)k0n, g.magic_ic);  // IC >= 32 here
        const int c0 = k0n - tap * g.IC;
        const int th = (int)(__umulhi((unsigned)tap, g.magic_kw) + (unsigned)tap * fast_tw_one);
        const int tw = tap - th * (int)fast_tw_n;
        int toff, wcol0;
        if (!DGRAD) {
            toff = ((th * g.IW + tw) * (int)g.ldi + c0) * ES;
            wcol0 = k0n;
        } else {
            toff = (c0 - (th * g.IW + tw) * (int)g.ldi) * ES;
            wcol0 = ((g.kh0 + g.stride * th) * g.KW + (g.kw0 + g.stride * tw)) * g.IC + c0;
        }
        const int tbit = kin ? tap : 31;  // bit 31 is never set: a prefetch past the last k-step loads zeros
        if constexpr (XM) {   // 1x1: k0n / 32 is the word of the row (a prefetch past the last k-step loads zeros)
            if (which & 1) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    ra[i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rs_a, (kin && xm_rel[i] >= 0) ? xm_rel[i] + (k0n >> 5) * 4 : -1, 0, 0);
            }
        } else if (which & 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int voff = ((a_mask[j] >> tbit) & 1u) ? a_rel[j] + toff : -1;
                if constexpr (SB) ra[j] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_a, voff, 0, 0));
                else ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, voff, 0, 0));
            }
        }
        if (which & 2) {
            const unsigned wb = (unsigned)wcol0 * 4u;
#pragma unroll
            for (int j = 0; j < BROWS; ++j)
                rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_b, (int)(b_rel[j] + wb), 0, 0));
        }
    };

    auto load_tiles = [&](int k0) {
        if (FAST) {
            load_tiles_fast(k0, ra, rb);
            return;
        }
        if constexpr (!SB && !XM) {   // (the generic loaders hold fp32 rows; SB / XM kernels are FAST by construction)
        const int kk = k0 + kq;
        if (VEC) {
            // Branch-free: every lane always loads from a clamped (valid) address and masks the value afterwards,
            // so the whole k-step stays one basic block and the scheduler can interleave these loads with MFMAs.
            const bool kin = kk < g.Ktot;
            int dy, dx, c, wcol;
            decode_k(kin ? kk : g.Ktot - 4, dy, dx, c, wcol);
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = a_y0[j] + dy, ix = a_x0[j] + dx;
                const bool ok = kin & a_ok[j] & ((unsigned)iy < (unsigned)g.IH) & ((unsigned)ix < (unsigned)g.IW);
                const int iyc = min(max(iy, 0), g.IH - 1), ixc = min(max(ix, 0), g.IW - 1);
                f32x4 v = *reinterpret_cast<const f32x4*>(in + (int64_t)(a_base[j] + iyc * g.IW + ixc) * g.ldi + c);
                ra[j] = ok ? v : zero;
            }
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                const int n = n0 + lr + 32 * j;
                const int nc = min(n, g.OC - 1);
                f32x4 v = *reinterpret_cast<const f32x4*>(wk + (int64_t)nc * g.KtotFull + wcol);
                rb[j] = (kin & (n < g.OC)) ? v : zero;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = kk + e;
                const bool kin = ke < g.Ktot;
                int dy, dx, c, wcol;
                decode_k(kin ? ke : 0, dy, dx, c, wcol);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int iy = a_y0[j] + dy, ix = a_x0[j] + dx;
                    float v = 0.f;
                    if (kin && a_ok[j] && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW)
                        v = in[(int64_t)(a_base[j] + iy * g.IW + ix) * g.ldi + c];
                    ra[j][e] = v;
                }
#pragma unroll
                for (int j = 0; j < BROWS; ++j) {
                    int n = n0 + lr + 32 * j;
                    rb[j][e] = (kin && n < g.OC) ? wk[(int64_t)n * g.KtotFull + wcol] : 0.f;
                }
            }
        }
        }
    };
    auto split_store = [&](const f32x4& v, __bf16* hi_img, __bf16* mid_img, __bf16* lo_img, int row) {
        bf16x4 hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {  // two elements per v_cvt_pk_bf16_f32; widening back is a shift / mask
            f32x2 rest = {v[e], v[e + 1]};
            bf16x2 p = __builtin_convertvector(rest, bf16x2);
            unsigned bits = __builtin_bit_cast(unsigned, p);
            hi[e] = p[0]; hi[e + 1] = p[1];
            rest[0] -= __builtin_bit_cast(float, bits << 16);
            rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
            if (SPLIT == 3) {
                p = __builtin_convertvector(rest, bf16x2);
                bits = __builtin_bit_cast(unsigned, p);
                mid[e] = p[0]; mid[e + 1] = p[1];
                rest[0] -= __builtin_bit_cast(float, bits << 16);
                rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
            }
            p = __builtin_convertvector(rest, bf16x2);
            lo[e] = p[0]; lo[e + 1] = p[1];
        }
        *reinterpret_cast<bf16x4*>(&hi_img[row * LDB + kq]) = hi;
        if (SPLIT == 3) *reinterpret_cast<bf16x4*>(&mid_img[row * LDB + kq]) = mid;
        *reinterpret_cast<bf16x4*>(&lo_img[row * LDB + kq]) = lo;
    };
    auto store_tiles = [&]() {
        if constexpr (SB || XM) return;
        else if (SPLIT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) split_store(ra[j], Ah, Am, Al, lr + 32 * j);
#pragma unroll
            for (int j = 0; j < BROWS; ++j) split_store(rb[j], Bh, Bm, Bl, lr + 32 * j);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(&As[(lr + 32 * j) * LDK + kq]) = ra[j];
#pragma unroll
            for (int j = 0; j < BROWS; ++j) *reinterpret_cast<f32x4*>(&Bs[(lr + 32 * j) * LDK + kq]) = rb[j];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if constexpr (FAST && SPLIT != 0) {
        // ---- software-pipelined main loop (2 waves / SIMD).  While the MFMAs of tile k run from LDS, the SAME wave
        // converts tile k+1 (raw fp32 in registers since the previous k-step) into its bf16 pieces in the MFMA
        // shadow - about 4 VALU per MFMA gap, which the matrix pipe hides - and then issues the loads of tile
        // k+2.  Between the two barriers only the LDS writes remain.  Measured without this (convert + write
        // between the barriers): MFMA pipe busy 36 % even with the global loads removed.
        constexpr int NP = NPIECE;                      // 16-bit images per operand
        constexpr int NPROD = SPLIT == 3 ? 6 : (SPLIT == 5 ? 1 : 3);   // MFMA products per accumulator and k16
        bf16x4 pa[4][NP], pb[BROWS][NP];                // [.][0] hi, [.][1] lo, [.][2] mid
        auto convert = [&](const f32x4& v, bf16x4* out, float scale) {
            if constexpr (SPLIT == 5) {  // one bf16 piece: round to nearest even
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const bf16x2 p = __builtin_convertvector(f32x2{v[e], v[e + 1]}, bf16x2);
                    out[0][e] = p[0]; out[0][e + 1] = p[1];
                }
                return;
            }
            if constexpr (SPLIT == 4) {  // fp16 pieces (v_cvt_pk_f16_f32); the residual x - hi is exact in fp32
                u32x2 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const float a = v[e] * scale, b = v[e + 1] * scale;
                    const f16x2 ph = __builtin_convertvector(f32x2{a, b}, f16x2);  // RNE: out of range -> inf (loud)
                    const f16x2 pl = __builtin_convertvector(f32x2{a - (float)ph[0], b - (float)ph[1]}, f16x2);
                    hi[e >> 1] = __builtin_bit_cast(unsigned, ph);
                    lo[e >> 1] = __builtin_bit_cast(unsigned, pl);
                }
                out[0] = __builtin_bit_cast(bf16x4, hi);
                out[1] = __builtin_bit_cast(bf16x4, lo);
                return;
            }
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                f32x2 rest = {v[e], v[e + 1]};
                bf16x2 p = __builtin_convertvector(rest, bf16x2);
                unsigned bits = __builtin_bit_cast(unsigned, p);
                out[0][e] = p[0]; out[0][e + 1] = p[1];
                rest[0] -= __builtin_bit_cast(float, bits << 16);
                rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
                if (SPLIT == 3) {
                    p = __builtin_convertvector(rest, bf16x2);
                    bits = __builtin_bit_cast(unsigned, p);
                    out[2][e] = p[0]; out[2][e + 1] = p[1];
                    rest[0] -= __builtin_bit_cast(float, bits << 16);
                    rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
                }
                p = __builtin_convertvector(rest, bf16x2);
                out[1][e] = p[0]; out[1][e + 1] = p[1];
            }
        };
        auto convert_a = [&](const AReg& v, bf16x4* out) {
            if constexpr (SB) out[0] = __builtin_bit_cast(bf16x4, v);   // already the bf16 values
            else if constexpr (XM) return;   // (expanded per fragment: mfma_group)
            else if constexpr (XSP) {   // z = (v_dec > th) as ONE fp16 piece of z * 2^4: 0x4C00 (16.0) or 0
                u32x2 hi;
#pragma unroll
                for (int e = 0; e < 4; e += 2)
                    hi[e >> 1] = (v[e] > g.x_th ? 0x4C00u : 0u) | (v[e + 1] > g.x_th ? 0x4C000000u : 0u);
                out[0] = __builtin_bit_cast(bf16x4, hi);
            } else convert(v, out, kF16ActScale);
        };
        auto convert_b = [&](const f32x4& v, bf16x4* out) {
            if constexpr (PRESPLIT) {   // the 16 bytes already are (4 hi, 4 lo)
                static_assert(!PRESPLIT || SPLIT == 2 || SPLIT == 4, "pre-split weights: two-piece modes only");
                out[0] = __builtin_bit_cast(bf16x4, f32x2{v[0], v[1]});
                out[1] = __builtin_bit_cast(bf16x4, f32x2{v[2], v[3]});
            } else {
                convert(v, out, kF16WeightScale);
            }
        };
        [[maybe_unused]] unsigned xm_cur[TM];   // XM: the mask words of the tile the MFMAs are working on
        // byte `sel` of a mask word as 8 fp16 values: bit b -> element b = 0x4C00 (16.0, the spike after the 2^4 pre-scale) or 0
        auto xm_expand = [&](unsigned word, int sel) {
            const unsigned b = (word >> (8 * sel)) & 0xffu;
            u32x4 d;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned v = (b >> (2 * q)) & 3u;
                d[q] = ((v | (v << 15)) & 0x00010001u) * 0x4C00u;
            }
            return __builtin_bit_cast(bf16x8, d);
        };
        auto write_tiles = [&]() {
#pragma unroll
            for (int j = 0; j < (XM ? 0 : 4); ++j) {
                const int o = (lr + 32 * j) * LDB + kq;
                *reinterpret_cast<bf16x4*>(&Ah[o]) = pa[j][0];
                if constexpr (NP >= 2 && !XSP) *reinterpret_cast<bf16x4*>(&Al[o]) = pa[j][1];
                if constexpr (NP >= 3) *reinterpret_cast<bf16x4*>(&Am[o]) = pa[j][2];
            }
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                const int o = (lr + 32 * j) * LDB + kq;
                *reinterpret_cast<bf16x4*>(&Bh[o]) = pb[j][0];
                if constexpr (NP >= 2) *reinterpret_cast<bf16x4*>(&Bl[o]) = pb[j][1];
                if constexpr (NP >= 3) *reinterpret_cast<bf16x4*>(&Bm[o]) = pb[j][2];
            }
        };
        auto mfma_group = [&](int ks) {  // lane (r, h) holds k = 16*ks + 8*h .. +7 of its row
            bf16x8 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int off = ((wm * TM + i) * 32 + r) * LDB + ks * 16 + 8 * h;
                if constexpr (XM) {
                    ah[i] = xm_expand(xm_cur[i], 2 * ks + h);
                    continue;
                }
                ah[i] = *reinterpret_cast<const bf16x8*>(&Ah[off]);
                if constexpr (NP >= 2 && !XSP) al[i] = *reinterpret_cast<const bf16x8*>(&Al[off]);
                if constexpr (NP >= 3) am[i] = *reinterpret_cast<const bf16x8*>(&Am[off]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int off = ((wn * TN + j) * 32 + r) * LDB + ks * 16 + 8 * h;
                bh[j] = *reinterpret_cast<const bf16x8*>(&Bh[off]);
                if constexpr (NP >= 2) bl[j] = *reinterpret_cast<const bf16x8*>(&Bl[off]);
                if constexpr (NP >= 3) bm[j] = *reinterpret_cast<const bf16x8*>(&Bm[off]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {  // small terms first
                    if constexpr (SPLIT == 5) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                        continue;
                    }
                    if constexpr (SPLIT == 4 && XSP) {   // the low image of a spike is zero: two products
                        const f16x8 xah = __builtin_bit_cast(f16x8, ah[i]);
                        const f16x8 xbh = __builtin_bit_cast(f16x8, bh[j]), xbl = __builtin_bit_cast(f16x8, bl[j]);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xah, xbl, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xah, xbh, acc[i][j], 0, 0, 0);
                        continue;
                    }
                    if constexpr (SPLIT == 4) {
                        const f16x8 xah = __builtin_bit_cast(f16x8, ah[i]), xal = __builtin_bit_cast(f16x8, al[i]);
                        const f16x8 xbh = __builtin_bit_cast(f16x8, bh[j]), xbl = __builtin_bit_cast(f16x8, bl[j]);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xal, xbh, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xah, xbl, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xah, xbh, acc[i][j], 0, 0, 0);
                        continue;
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    if (SPLIT == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        };
        constexpr int NM = TM * TN * (XSP ? 2 : NPROD);  // MFMAs per k16 group
        constexpr int NREAD = XM ? TN * NP : (XSP ? TM + TN * NP : (TM + TN) * NP);   // ds_read_b128 per k16 group
        constexpr int CONV_OPS = SPLIT == 3 ? 24 : (SPLIT == 5 ? 2 : 14);   // VALU per converted f32x4 (approx.)
        constexpr int VPG_A = ((XM ? TM * 18 : (XSP ? 4 * 8 : 4 * CONV_OPS)) + NM - 1) / NM;
        constexpr int VPG_B = PRESPLIT ? 1 : (BROWS * CONV_OPS + NM - 1) / NM;   // pre-split: only register moves
        if (g.Ktot > 0) {
            // both first tiles are requested back to back (the accumulators are not live yet, registers are free):
            // one exposed memory latency per block instead of two
            AReg ra0[4];
            f32x4 rb0[BROWS];
            load_tiles_fast(0, ra0, rb0);
            load_tiles_fast(BK, ra, rb);
            if constexpr (XM) {
#pragma unroll
                for (int i = 0; i < TM; ++i) xm_cur[i] = ra0[i];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) convert_a(ra0[j], pa[j]);
#pragma unroll
            for (int j = 0; j < BROWS; ++j) convert_b(rb0[j], pb[j]);
            write_tiles();
        }
        __syncthreads();
#ifdef SNN_STAMP
        unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long st_last = __builtin_readcyclecounter();
        const unsigned long long st_begin = st_last;
#endif
#pragma unroll 1
        for (int k0 = 0; k0 < g.Ktot; k0 += BK) {
            mfma_group(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) convert_a(ra[j], pa[j]);
            // shape the schedule: operand reads, then every MFMA followed by its share of the conversion VALU
            __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, VPG_A, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            STAMP(0);
            mfma_group(1);
#pragma unroll
            for (int j = 0; j < BROWS; ++j) convert_b(rb[j], pb[j]);
            __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, VPG_B, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            STAMP(1);
            if constexpr (XM) {   // the words of tile k + 1 (requested one k-step ago) become the current ones
#pragma unroll
                for (int i = 0; i < TM; ++i) xm_cur[i] = ra[i];
            }
            load_tiles_fast(k0 + 2 * BK, ra, rb);   // (requesting the A rows one MFMA group earlier: measured neutral)
            STAMP(2);
            __syncthreads();
            STAMP(3);
            write_tiles();
            STAMP(4);
            __syncthreads();
            STAMP(5);
        }
#ifdef SNN_STAMP
        if (tid == 0 && bid_n == 0 && blockIdx.x < 2048) {
            st_acc[6] = __builtin_readcyclecounter() - st_begin;
            st_acc[7] = st_begin;
            for (int i = 0; i < 8; ++i) g_stamps[blockIdx.x * 8 + i] = st_acc[i];
        }
#endif
    } else {
        if (g.Ktot > 0) {  // a dgrad stride-phase class may have no tap at all: its pixels are plain zeros
            load_tiles(0);
            store_tiles();
        }
        __syncthreads();

        // Branch-free steady state (a tile past Ktot loads zeros and is never read): keeping the MFMA chain in
        // one basic block lets the accumulators stay in their registers across iterations.
    #pragma unroll 1
        for (int k0 = 0; k0 < g.Ktot; k0 += BK) {
            load_tiles(k0 + BK);
            // keep the prefetch ahead of the MFMA chain: its latency must be covered by the whole k-step
            __builtin_amdgcn_sched_barrier(0);
            if (SPLIT) {
    #pragma unroll
                for (int ks = 0; ks < BK / 16; ++ks) {  // lane (r, h) holds k = 16*ks + 8*h .. +7 of its row
                    bf16x8 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
    #pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int off = ((wm * TM + i) * 32 + r) * LDB + ks * 16 + 8 * h;
                        ah[i] = *reinterpret_cast<const bf16x8*>(&Ah[off]);
                        al[i] = *reinterpret_cast<const bf16x8*>(&Al[off]);
                        if (SPLIT == 3) am[i] = *reinterpret_cast<const bf16x8*>(&Am[off]);
                    }
    #pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int off = ((wn * TN + j) * 32 + r) * LDB + ks * 16 + 8 * h;
                        bh[j] = *reinterpret_cast<const bf16x8*>(&Bh[off]);
                        bl[j] = *reinterpret_cast<const bf16x8*>(&Bl[off]);
                        if (SPLIT == 3) bm[j] = *reinterpret_cast<const bf16x8*>(&Bm[off]);
                    }
    #pragma unroll
                    for (int i = 0; i < TM; ++i)
    #pragma unroll
                        for (int j = 0; j < TN; ++j) {  // small terms first
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                            if (SPLIT == 3) {
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm[j], acc[i][j], 0, 0, 0);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
                            }
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                        }
                }
            }
            const float* Ac = As;
            const float* Bc = Bs;
    #pragma unroll
            for (int ks = 0; ks < (SPLIT ? 0 : BK / 8); ++ks) {
                f32x4 a[TM], b[TN];
    #pragma unroll
                for (int i = 0; i < TM; ++i)
                    a[i] = *reinterpret_cast<const f32x4*>(&Ac[((wm * TM + i) * 32 + r) * LDK + ks * 8 + 4 * h]);
    #pragma unroll
                for (int j = 0; j < TN; ++j)
                    b[j] = *reinterpret_cast<const f32x4*>(&Bc[((wn * TN + j) * 32 + r) * LDK + ks * 8 + 4 * h]);
    #pragma unroll
                for (int e = 0; e < 4; ++e)
    #pragma unroll
                    for (int i = 0; i < TM; ++i)
    #pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            store_tiles();
            __syncthreads();
        }
    }

    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5), i.e. a
    // lane holds ONE channel of 16 pixels.  Each wave transposes its accumulators through LDS (the operand tiles
    // are dead by now) so that a lane stores 16 contiguous bytes and a pixel row goes out as TN*128-byte runs:
    // 4x fewer, wider store instructions (the k-short 1x1 convolutions are store-issue bound otherwise).
    constexpr int EW = TN * 32 + 4;   // staged row length in floats
    constexpr int LPR = TN * 8;       // lanes per staged row (4 floats each)
    constexpr int RPP = 64 / LPR;     // rows per pass
    static_assert(4 * 32 * EW * 4 <= SMEM_BYTES, "epilogue staging does not fit the operand tiles");
    float* stage = reinterpret_cast<float*>(smem) + wave * 32 * EW;
    const bool ovec = g.out_vec != 0;
    if (!DGRAD && g.bn_partial != nullptr) {
        // BatchNorm partials: rows below `split` belong to timestep bn_t, the rest (up to Mtot) to bn_t + 1
        const int64_t bn_t = m0 / g.bn_rows;
        const int64_t split = (bn_t + 1) * g.bn_rows;
        const bool whole = split >= m0 + BM && m0 + BM <= g.Mtot;   // one timestep, no rows past the end
        double s_lo[TN], q_lo[TN], s_hi[TN], q_hi[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) s_lo[j] = q_lo[j] = s_hi[j] = q_hi[j] = 0.0;
        if (whole) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const double d = (double)(SPLIT == 4 ? acc[i][j][e] * kF16Unscale : acc[i][j][e]);
                        s_lo[j] += d;
                        q_lo[j] = fma(d, d, q_lo[j]);
                    }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int64_t m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                        const double d = (double)(SPLIT == 4 ? acc[i][j][e] * kF16Unscale : acc[i][j][e]);
                        const double lo = m < split ? d : 0.0, hi = (m >= split && m < g.Mtot) ? d : 0.0;
                        s_lo[j] += lo;
                        q_lo[j] = fma(lo, lo, q_lo[j]);
                        s_hi[j] += hi;
                        q_hi[j] = fma(hi, hi, q_hi[j]);
                    }
        }
        // the operand tiles are dead (the k loop ended with a barrier); the staging below starts after stat_flush's
        double* red = reinterpret_cast<double*>(smem);
        static_assert(4 * TN * 32 * 2 * 8 <= SMEM_BYTES, "statistics scratch does not fit");
        const int chunk = (int)(m0 / BM - (bn_t * g.bn_rows) / BM);
        stat_flush<WM, WN, TN>(s_lo, q_lo, red, g.bn_partial, bn_t, chunk, g.bn_chunks, n0, g.OC, tid);
        if (split < m0 + BM && split < g.Mtot)   // this tile is also the first one of the next timestep
            stat_flush<WM, WN, TN>(s_hi, q_hi, red, g.bn_partial, bn_t + 1, 0, g.bn_chunks, n0, g.OC, tid);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stage[((e & 3) + 8 * (e >> 2) + 4 * h) * EW + j * 32 + r] =
                    SPLIT == 4 ? acc[i][j][e] * kF16Unscale : acc[i][j][e];  // undo the operand pre-scales
        __syncthreads();
        // Address arithmetic: for the common case (output pixel = GEMM row) everything but a per-lane 32-bit offset
        // is wave-uniform: base pointers of the 32-row group live in SGPRs, the lane adds (its row) * ld + channel.
        // (The general form spent ~50 64-bit multiplies per wave here - a third of the epilogue.)
        const bool linear = !(DGRAD && g.stride > 1);
        const int64_t mrow0 = m0 + (wm * TM + i) * 32;   // wave-uniform
        const int lrow = lane_id / LPR;
        const int c4 = (lane_id % LPR) * 4;
        const int n = n0 + wn * TN * 32 + c4;
        typedef SnnStore<SB> St;   // fp32 tensors, or bf16 (rounded here) in the bf16-storage mode
        char* const out_b = reinterpret_cast<char*>(out);
        const char* const ad1_b = reinterpret_cast<const char*>(addend);
        const char* const ad2_b = reinterpret_cast<const char*>(addend2);
        char* out_g = out_b + mrow0 * g.ldo * ES;
        const char* ad1_g = addend ? ad1_b + mrow0 * ld_add * ES : nullptr;
        const char* ad2_g = addend2 ? ad2_b + mrow0 * ld_add2 * ES : nullptr;
        const int o_l = lrow * (int)g.ldo + n, a1_l = lrow * (int)ld_add + n, a2_l = lrow * (int)ld_add2 + n;
#pragma unroll
        for (int pass = 0; pass < 32 / RPP; ++pass) {
            const int row = pass * RPP + lrow;
            const int64_t m = mrow0 + row;
            if (m >= g.Mtot || n >= g.OC) continue;
            f32x4 v = *reinterpret_cast<const f32x4*>(&stage[row * EW + c4]);
            char* dst;
            const char *a1p, *a2p;
            if (linear) {
                dst = out_g + (o_l + pass * RPP * (int)g.ldo) * ES;
                a1p = ad1_g + (a1_l + pass * RPP * (int)ld_add) * ES;
                a2p = ad2_g + (a2_l + pass * RPP * (int)ld_add2) * ES;
            } else {
                const unsigned t = (unsigned)m / (unsigned)g.OWc;
                const int b = (int)((unsigned)m - t * (unsigned)g.OWc);
                const unsigned img = t / (unsigned)g.OHc;
                const int a = (int)(t - img * (unsigned)g.OHc);
                const int64_t pix = ((int64_t)img * g.OH + (a * g.stride + g.ph)) * g.OW + (b * g.stride + g.pw);
                dst = out_b + (pix * g.ldo + n) * ES;
                a1p = ad1_b + (pix * ld_add + n) * ES;
                a2p = ad2_b + (pix * ld_add2 + n) * ES;
            }
            if (ovec && n + 3 < g.OC) {
                if (addend) v += St::ld4_last(a1p, 0);  // fused accumulation (the addend's only reader)
                if (addend2) v += St::ld4_last(a2p, 0);
                St::st4(dst, 0, v);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (n + q < g.OC) {
                        float o = v[q];
                        if (addend) o += St::ld1(a1p, q);
                        if (addend2) o += St::ld1(a2p, q);
                        St::st1(dst, q, o);
                    }
            }
        }
        __syncthreads();
    }
#if defined(SNN_STAMP) || defined(SNN_CLOCK)
    if (tid == 0 && bid_n == 0 && blockIdx.x < 2048) {
        g_stamps2[blockIdx.x * 4 + 0] = st_kernel_begin;
        g_stamps2[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memtime();
        g_stamps2[blockIdx.x * 4 + 2] = st_real_begin;
        g_stamps2[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// The launch plan of k_conv_gather for one ConvGeom (the forward, or one stride phase of a data gradient), read by
// launch_gather and by snn_conv2d_gather_plan.  ok = 0: the launch refuses the call (why: the reason).
enum GatherLoader { kLoadScalar = 0, kLoadVec = 1, kLoadFast = 2, kLoadFastPresplit = 3, kLoadSB = 4, kLoadXSP = 5, kLoadXM = 6 };
enum GatherRefusal { kGatherOk = 0, kGatherTooManyPixels, kGatherNotFastSB, kGatherNotFastXSP, kGatherGridTooLarge };
struct GatherPlan {
    int ok, why;
    int loader;      // GatherLoader
    int bn;          // output channels per block: 32, 64, 128
    int out_vec;     // output (and addend) rows stored 16 bytes per lane
    int mtiles, mtiles_per_xcd, ntiles;
    int64_t blocks;  // mtiles_per_xcd * 8 * ntiles: the blocks past the last pixel tile of an XCD share return at once
};
// xm (with xsp): the gathered tensor is a spike bit mask (uint32 words, g.ldi words per pixel; kAlignIn16 then stands for
// its 4-byte alignment)
static GatherPlan gather_plan(const ConvGeom& g, bool dgrad, int split, bool sb, bool xsp, unsigned align, bool has_split,
                              bool has_add, bool has_add2, bool xm = false) {
    GatherPlan p = {};
    const bool vec = (g.IC % 4 == 0) && (xm || g.ldi % 4 == 0) && (align & (sb ? kAlignIn8 : kAlignIn16)) && (align & kAlignW16);
    const int64_t gm = snn_ceil_div(g.Mtot, BM);
    if (!(g.Mtot < 0x7fffffffLL && (int64_t)g.IH * g.IW < 0x7fffffffLL)) {
        p.why = kGatherTooManyPixels;
        return p;
    }
    const int nth = dgrad ? g.nkh : g.KH, ntw = dgrad ? g.nkw : g.KW;
    const int ntaps = nth * ntw;
    static const bool no_fast = snn_tuning_env("SNN_CONV_NO_FAST") != nullptr;  // tuning / bisecting aid
    const bool fast = vec && !no_fast && g.IC % BK == 0 && ntaps >= 1 && ntaps <= 31 && nth <= 6 && ntw <= 6 &&
                      (int64_t)g.IH * g.IW * g.ldi * 16 < 0x7fffffffLL && (int64_t)g.OC * g.KtotFull * 4 < 0x7fffffffLL &&
                      (!xm || (ntaps == 1 && g.stride == 1 && g.pad == 0 && g.ldi * 32 >= g.IC && g.Mtot * g.ldi * 4 < 0x7fffffffLL));
    p.out_vec = (g.ldo % 4 == 0) && (align & (sb ? kAlignOut8 : kAlignOut16)) &&
                (!has_add || (align & (sb ? kAlignAdd8 : kAlignAdd16))) &&
                (!has_add2 || (align & (sb ? kAlignAdd2_8 : kAlignAdd2_16)));
    if (sb && !fast) {
        p.why = kGatherNotFastSB;
        return p;
    }
    if (xsp && !fast) {
        p.why = kGatherNotFastXSP;
        return p;
    }
    // the pre-split weight image serves the pipelined kernel in its two-piece modes; every other path converts wk itself
    const bool presplit = has_split && (split == 2 || split == 4) && (align & kAlignSplit16);
    p.loader = sb ? kLoadSB : xm ? kLoadXM : xsp ? kLoadXSP : (fast && presplit) ? kLoadFastPresplit : fast ? kLoadFast : vec ? kLoadVec : kLoadScalar;
    p.bn = g.OC <= 32 ? 32 : (g.OC <= 64 ? 64 : 128);
    p.mtiles = (int)gm;
    p.mtiles_per_xcd = (int)snn_ceil_div(gm, 8);
    p.ntiles = (int)snn_ceil_div(g.OC, p.bn);
    p.blocks = (int64_t)p.mtiles_per_xcd * 8 * p.ntiles;
    if (p.blocks > 0x7fffffffLL) {
        p.why = kGatherGridTooLarge;
        return p;
    }
    p.ok = 1;
    return p;
}

static unsigned gather_align_bits(const void* in, const void* wk, const void* wk_split, const void* out, const void* addend,
                                  int64_t ld_add, const void* addend2, int64_t ld_add2) {
    unsigned a = 0;
    if (aligned(16, {in})) a |= kAlignIn16;
    if (aligned(8, {in})) a |= kAlignIn8;
    if (aligned(16, {wk})) a |= kAlignW16;
    if (aligned(16, {out})) a |= kAlignOut16;
    if (aligned(8, {out})) a |= kAlignOut8;
    if (addend && ld_add % 4 == 0 && aligned(16, {addend})) a |= kAlignAdd16;
    if (addend && ld_add % 4 == 0 && aligned(8, {addend})) a |= kAlignAdd8;
    if (addend2 && ld_add2 % 4 == 0 && aligned(16, {addend2})) a |= kAlignAdd2_16;
    if (addend2 && ld_add2 % 4 == 0 && aligned(8, {addend2})) a |= kAlignAdd2_8;
    if (wk_split && aligned(16, {wk_split})) a |= kAlignSplit16;
    return a;
}

constexpr int gather_wm(int bn) { return bn == 32 ? 4 : 2; }   // waves of a block over pixels / over its bn channels
constexpr int gather_wn(int bn) { return bn == 32 ? 1 : 2; }

// split: the SPLIT of k_conv_gather the precision asks for (snn_conv2d_fwd: 0, 3, 4, 5; snn_conv2d_dgrad: 0, 2, 5)
static int launch_gather(bool dgrad, int split, bool sb, bool xsp, const float* in, const float* wk, const void* wk_split,
                         float* out, const ConvGeom& g, const float* addend, int64_t ld_add, const float* addend2,
                         int64_t ld_add2, hipStream_t st, const char* name, bool xm = false) {
    unsigned align = gather_align_bits(in, wk, wk_split, out, addend, ld_add, addend2, ld_add2);
    if (xm) align = (align & ~(kAlignIn16 | kAlignIn8)) | (aligned(4, {in}) ? kAlignIn16 : 0u);
    const GatherPlan p = gather_plan(g, dgrad, split, sb, xsp, align, wk_split != nullptr, addend != nullptr,
                                     addend2 != nullptr, xm);
    SNN_REQUIRE(p.why != kGatherTooManyPixels, "%s: too many pixels", name);
    SNN_REQUIRE(p.why != kGatherNotFastSB, "%s: bf16 storage covers the pipelined implicit GEMM only (channels a multiple of 32, pixel "
                "stride a multiple of 4, 8-byte aligned tensors): %d channels, stride %lld", name, g.IC, (long long)g.ldi);
    SNN_REQUIRE(p.why != kGatherNotFastXSP, "%s: covers the pipelined implicit GEMM only (input channels a multiple of 32, pixel stride a "
                "multiple of 4, 16-byte aligned tensors): %d channels, stride %lld", name, g.IC, (long long)g.ldi);
    SNN_REQUIRE(p.why != kGatherGridTooLarge, "%s: grid too large", name);
    ConvGeom gg = g;
    gg.out_vec = p.out_vec;
    gg.mtiles = p.mtiles;
    gg.mtiles_per_xcd = p.mtiles_per_xcd;
    gg.ntiles = p.ntiles;
    const dim3 grid((unsigned)p.blocks);
    const float* wsrc = p.loader == kLoadFastPresplit ? static_cast<const float*>(wk_split) : wk;
    dispatch(
        [&](auto BN, auto L, auto DGRAD, auto SPLIT) {
            constexpr int l = L(), s = SPLIT();
            constexpr bool vec = l != kLoadScalar, fast = l >= kLoadFast, pre = l == kLoadFastPresplit, sbl = l == kLoadSB,
                           xml = l == kLoadXM, xspl = l == kLoadXSP || xml;
            // the vector loader has no two-piece fp16 and no one-product arithmetic (4 -> 3, 5 -> 2); the scalar one is fp32
            constexpr int ksplit = fast ? s : (vec ? (s == 4 ? 3 : (s == 5 ? 2 : s)) : 0);
            // SB is SPLIT 5, XSP the forward with SPLIT 4, the pre-split image serves SPLIT 2 and 4
            if constexpr ((DGRAD() ? s != 3 && s != 4 : s != 2) && (!sbl || s == 5) && (!xspl || (!DGRAD() && s == 4)) &&
                          (!pre || s == 2 || s == 4)) {
                hipLaunchKernelGGL((k_conv_gather<BN(), gather_wm(BN()), gather_wn(BN()), DGRAD(), vec, ksplit, fast, pre, sbl, xspl, xml>),
                                   grid, dim3(kThreads), 0, st, in, wsrc, out, gg, addend, ld_add, addend2, ld_add2);
                return true;
            }
            return false;
        },
        OneOf<32, 64, 128>{p.bn}, OneOf<0, 1, 2, 3, 4, 5, 6>{p.loader}, Flag{dgrad}, OneOf<0, 2, 3, 4, 5>{split});
    SNN_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

// ---- pre-split weight images (see PRESPLIT of k_conv_gather).  Elementwise over groups of 4 consecutive floats: the
// group's 16 bytes become (4 hi pieces, 4 lo pieces) with exactly the arithmetic of the in-kernel conversion - fp16
// pieces of w * 2^8 (forward, SNN_PREC_FP16X3) or bf16 pieces of w (data gradient, SNN_PREC_BF16X3; apply it to the
// transposed weights).  A weight row (KH*KW*Cin floats) must start on a group boundary.
namespace {
template <bool F16>
__global__ void k_weight_presplit(const f32x4* __restrict__ w, u32x4* __restrict__ out, int64_t groups) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = w[i];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
            if (F16) {
                const float a = v[e] * kF16WeightScale, b = v[e + 1] * kF16WeightScale;
                const f16x2 ph = __builtin_convertvector(f32x2{a, b}, f16x2);
                const f16x2 pl = __builtin_convertvector(f32x2{a - (float)ph[0], b - (float)ph[1]}, f16x2);
                o[e >> 1] = __builtin_bit_cast(unsigned, ph);
                o[2 + (e >> 1)] = __builtin_bit_cast(unsigned, pl);
            } else {
                f32x2 rest = {v[e], v[e + 1]};
                const bf16x2 ph = __builtin_convertvector(rest, bf16x2);
                const unsigned bits = __builtin_bit_cast(unsigned, ph);
                rest[0] -= __builtin_bit_cast(float, bits << 16);
                rest[1] -= __builtin_bit_cast(float, bits & 0xffff0000u);
                const bf16x2 pl = __builtin_convertvector(rest, bf16x2);
                o[e >> 1] = bits;
                o[2 + (e >> 1)] = __builtin_bit_cast(unsigned, pl);
            }
        }
        out[i] = o;
    }
}
}  // namespace

extern "C" int snn_weight_presplit(const float* w, void* out, int64_t n, int precision, void* stream) {
    SNN_REQUIRE(w && out && n > 0 && n % 4 == 0, "snn_weight_presplit: bad arguments (n = %lld must be a multiple of 4)",
                (long long)n);
    SNN_REQUIRE(aligned(16, {w, out}), "snn_weight_presplit: buffers must be 16-byte aligned");
    SNN_REQUIRE(precision == SNN_PREC_FP16X3 || precision == SNN_PREC_BF16X3,
                "snn_weight_presplit: precision must be SNN_PREC_FP16X3 (forward) or SNN_PREC_BF16X3 (data gradient)");
    const int64_t groups = n / 4;
    int64_t blocks = snn_ceil_div(groups, kThreads);
    if (blocks > 8 * snn_num_cu()) blocks = 8 * snn_num_cu();
    dispatch(
        [&](auto F16) {
            hipLaunchKernelGGL(k_weight_presplit<F16()>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                               reinterpret_cast<const f32x4*>(w), reinterpret_cast<u32x4*>(out), groups);
            return true;
        },
        Flag{precision == SNN_PREC_FP16X3});
    SNN_CHECK_LAUNCH("snn_weight_presplit");
    return 0;
}

// Chunk slots per timestep of the statistics partials (see stat_flush); 0: not produced.  The size covers the three
// forward kernels that leave them: the implicit GEMM, the first-layer row kernel and the halo-resident 3x3 kernel.
namespace {
static int64_t gather_bn_chunks(int64_t rows_per_step) { return (rows_per_step + BM - 1) / BM + 1; }

// chunk slots per timestep the epilogue of k_conv_gather fills (rows per chunk: BM); 0: this kernel leaves no partials
// (a timestep shorter than a row tile would meet more than two timesteps per tile) and the caller runs snn_bn_stats
static int gather_bn_plan(bool want, int64_t step_rows) {
    return want && step_rows >= BM && gather_bn_chunks(step_rows) <= 0x7fffffff ? (int)gather_bn_chunks(step_rows) : 0;
}

// geometry of a forward launch of k_conv_gather (no statistics, no threshold: the caller adds them)
static ConvGeom gather_fwd_geom(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                int pad, int64_t ldx, int64_t ldy) {
    ConvGeom g;
    g.Mtot = N * Ho * (int64_t)Wo;
    g.IH = H; g.IW = W; g.IC = Cin;
    g.OH = Ho; g.OW = Wo; g.OC = Cout;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.ldi = ldx; g.ldo = ldy;
    g.Ktot = g.KtotFull = KH * KW * Cin;
    g.nimg = (int)N;
    g.ph = g.pw = g.kh0 = g.kw0 = 0; g.nkh = KH; g.nkw = KW; g.OHc = Ho; g.OWc = Wo;
    g.magic_ic = magic_u32(Cin); g.magic_kw = magic_u32(KW);
    g.out_vec = 0; g.mtiles = g.mtiles_per_xcd = g.ntiles = 0;
    g.bn_partial = nullptr; g.bn_rows = 0; g.bn_chunks = 0; g.x_th = 0.0f;
    return g;
}

// geometry of a data gradient: what every stride phase shares ...
static ConvGeom gather_dgrad_geom(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                  int pad, int64_t lddy, int64_t lddx) {
    ConvGeom g;
    g.IH = Ho; g.IW = Wo; g.IC = Cout;  // gathered tensor is dy
    g.OH = H; g.OW = W; g.OC = Cin;     // one GEMM row per INPUT pixel
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.ldi = lddy; g.ldo = lddx;
    g.KtotFull = KH * KW * Cout;
    g.nimg = (int)N;
    g.out_vec = 0; g.mtiles = g.mtiles_per_xcd = g.ntiles = 0;
    g.bn_partial = nullptr; g.bn_rows = 0; g.bn_chunks = 0; g.x_th = 0.0f;
    g.Mtot = 0; g.Ktot = 0; g.ph = g.pw = g.kh0 = g.kw0 = g.nkh = g.nkw = g.OHc = g.OWc = 0; g.magic_ic = g.magic_kw = 0;
    return g;
}
// ... and one launch per stride phase (ph, pw), ph < min(stride, H), pw < min(stride, W): each class multiplies only the
// taps that can reach it (a class may have none: its pixels are the addends, or zeros)
static void gather_dgrad_phase(ConvGeom& g, int ph, int pw) {
    const int stride = g.stride, pad = g.pad, H = g.OH, W = g.OW;
    g.ph = ph; g.pw = pw;
    g.kh0 = (ph + pad) % stride; g.kw0 = (pw + pad) % stride;
    g.nkh = g.kh0 < g.KH ? (g.KH - g.kh0 + stride - 1) / stride : 0;
    g.nkw = g.kw0 < g.KW ? (g.KW - g.kw0 + stride - 1) / stride : 0;
    g.OHc = (H - ph + stride - 1) / stride;
    g.OWc = (W - pw + stride - 1) / stride;
    g.Mtot = (int64_t)g.nimg * g.OHc * (int64_t)g.OWc;
    g.Ktot = g.nkh * g.nkw * g.IC;
    g.magic_ic = magic_u32(g.IC); g.magic_kw = magic_u32(g.nkw);
}

// does the event-frame row kernel take this forward call (see snn_conv2d_fwd)?  align: the kAlign* facts of x and y
static bool fwd_takes_first(const FirstPlan& fp, bool has_addend, int64_t ldx, int64_t ldy, int W, int Wo, bool sbf,
                            unsigned align) {
    return fp.ok && !has_addend && ldx % 2 == 0 && (align & kAlignIn8) && ldy % 4 == 0 &&
           (align & (sbf ? kAlignOut8 : kAlignOut16)) && (int64_t)W * ldx < 0x7fffffffLL && (int64_t)Wo * ldy < 0x7fffffffLL;
}
}  // namespace

extern "C" size_t snn_conv2d_fwd_bn_partial_size(int64_t N, int frames_per_step, int Ho, int Wo, int Cout) {
    if (N <= 0 || frames_per_step <= 0 || N % frames_per_step != 0 || Ho <= 0 || Wo <= 0 || Cout <= 0) return 0;
    const int64_t T = N / frames_per_step, rows = (int64_t)frames_per_step * Ho * Wo;
    int64_t chunks = gather_bn_chunks(rows);
    if ((int64_t)frames_per_step * Ho > chunks) chunks = (int64_t)frames_per_step * Ho;   // first layer: <= one block per row
    const int64_t hc = snn_conv3x3_halo_bn_chunks(frames_per_step, Ho, Wo);                // halo-resident 3x3 (conv_halo.hip)
    if (hc > chunks) chunks = hc;
    return (size_t)(T * chunks * Cout * 2);
}

extern "C" int snn_conv2d_fwd(const float* x, int64_t ldx, const float* w, const void* w_split, float* y, int64_t ldy,
                              int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                              int pad, const float* addend, int64_t ld_addend, double* bn_partial, int frames_per_step,
                              int* bn_layout, int precision, void* stream) {
    SNN_REQUIRE(x && w && y, "snn_conv2d_fwd: null pointer");
    SNN_REQUIRE(!w_split || precision == SNN_PREC_FP16X3,
                "snn_conv2d_fwd: a pre-split weight image exists for SNN_PREC_FP16X3 only (precision %d)", precision);
    SNN_REQUIRE(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X6 || precision == SNN_PREC_FP16X3 ||
                    precision == SNN_PREC_BF16X1 || precision == SNN_PREC_BF16S,
                "snn_conv2d_fwd: precision must be SNN_PREC_FP32, _BF16X6, _FP16X3, _BF16X1 or _BF16S (got %d)", precision);
    const bool sbf = precision == SNN_PREC_BF16S;   // x (but for the fp32 event frames), y, addend are bf16
    if (check_conv_shape("snn_conv2d_fwd", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    SNN_REQUIRE(ldx >= Cin && ldy >= Cout, "snn_conv2d_fwd: pixel stride smaller than channel count");
    SNN_REQUIRE(!bn_partial || (bn_layout && frames_per_step > 0 && N % frames_per_step == 0),
                "snn_conv2d_fwd: statistics need bn_layout and a frames_per_step that divides N (%lld frames, %d per step)",
                (long long)N, frames_per_step);
    SNN_REQUIRE(!(bn_partial && addend), "snn_conv2d_fwd: statistics are of the convolution itself - no addend with bn_partial");
    if (bn_layout) bn_layout[0] = bn_layout[1] = 0;
    const int64_t step_rows = bn_partial ? (int64_t)frames_per_step * Ho * Wo : 0;
    ConvGeom g = gather_fwd_geom(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ldx, ldy);
    SNN_REQUIRE(N * (int64_t)H * W < 0x7fffffffLL && (int64_t)g.Ktot * Cin < 0xffffffffLL,
                "snn_conv2d_fwd: tensor too large for 32-bit pixel indexing");
    SNN_REQUIRE(!addend || ld_addend >= Cout, "snn_conv2d_fwd: addend pixel stride smaller than channel count");
    const FirstPlan fp = Cin == 2 && KH == 3 && KW == 3
                             ? snn_first_layer_plan(N, H, W, Ho, Wo, Cout, stride, pad, bn_partial ? frames_per_step : 0, false, 0)
                             : FirstPlan{};
    if (fwd_takes_first(fp, addend != nullptr, ldx, ldy, W, Wo, sbf,
                        gather_align_bits(x, w, nullptr, y, nullptr, 0, nullptr, 0))) {
        FirstGeom fg = {ldx, ldy, (int)(N * Ho), H, W, Ho, Wo, Cout, stride, pad, fp.group_rows, fp.group_blocks,
                        bn_partial, nullptr, 0, nullptr, 0, 1, fp.rs};
        if (bn_partial) bn_layout[0] = fp.group_blocks;
        return snn_launch_first(false, false, sbf, fp.blocks, fp.lds, x, w, nullptr, y, fg, stream, "snn_conv2d_fwd");
    }
    SNN_REQUIRE(!sbf || Cin % 32 == 0, "snn_conv2d_fwd: bf16 storage covers the event-frame layer (fp32 frames, Cin = 2, "
                "3x3) and layers with a multiple of 32 input channels (got %d)", Cin);
    if (const int chunks = gather_bn_plan(bn_partial != nullptr, step_rows)) {
        g.bn_partial = bn_partial;
        g.bn_rows = step_rows;
        g.bn_chunks = chunks;
        bn_layout[0] = g.bn_chunks;
        bn_layout[1] = BM;
    }
    return launch_gather(false, sbf ? 5 : precision, sbf, false, x, w, w_split, y, g, addend, ld_addend, nullptr, 0,
                         (hipStream_t)stream, "snn_conv2d_fwd");
}

extern "C" int snn_conv2d_dgrad(const float* dy, int64_t lddy, const float* wt, const void* wt_split, float* dx,
                                int64_t lddx, int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                                int stride, int pad, const float* addend, int64_t ld_addend, const float* addend2,
                                int64_t ld_addend2, int precision, void* stream) {
    SNN_REQUIRE(dy && wt && dx, "snn_conv2d_dgrad: null pointer");
    SNN_REQUIRE(!wt_split || precision == SNN_PREC_BF16X3,
                "snn_conv2d_dgrad: a pre-split weight image exists for SNN_PREC_BF16X3 only (precision %d)", precision);
    SNN_REQUIRE(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X3 || precision == SNN_PREC_BF16X1 ||
                    precision == SNN_PREC_BF16S,
                "snn_conv2d_dgrad: precision must be SNN_PREC_FP32, _BF16X3, _BF16X1 or _BF16S (got %d)", precision);
    const bool sbf = precision == SNN_PREC_BF16S;   // dy, dx and the addends are bf16
    const int bwd_split = (sbf || precision == SNN_PREC_BF16X1) ? 5 : (precision != SNN_PREC_FP32 ? 2 : 0);
    SNN_REQUIRE(!addend2 || ld_addend2 >= Cin, "snn_conv2d_dgrad: addend2 pixel stride smaller than channel count");
    if (check_conv_shape("snn_conv2d_dgrad", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    SNN_REQUIRE(lddy >= Cout && lddx >= Cin, "snn_conv2d_dgrad: pixel stride smaller than channel count");
    SNN_REQUIRE(!addend || ld_addend >= Cin, "snn_conv2d_dgrad: addend pixel stride smaller than channel count");
    ConvGeom g = gather_dgrad_geom(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, lddy, lddx);
    SNN_REQUIRE(N * (int64_t)Ho * Wo < 0x7fffffffLL && (int64_t)g.KtotFull * Cout < 0xffffffffLL,
                "snn_conv2d_dgrad: tensor too large for 32-bit pixel indexing");
    // one launch per stride phase: each class multiplies only the taps that can reach it
    for (int ph = 0; ph < stride && ph < H; ++ph)
        for (int pw = 0; pw < stride && pw < W; ++pw) {
            gather_dgrad_phase(g, ph, pw);
            const int rc = launch_gather(true, bwd_split, sbf, false, dy, wt, wt_split, dx, g, addend, ld_addend, addend2,
                                         ld_addend2, (hipStream_t)stream, "snn_conv2d_dgrad");
            if (rc) return rc;
        }
    return 0;
}

// Host-only: the plan of the k_conv_gather launch behind snn_conv2d_fwd (mode 0), one stride phase of snn_conv2d_dgrad
// (mode 1) or snn_conv2d_spikes_fwd (mode 2); see include/snn_hip.h.  It builds the geometry and reads the plan with the
// functions the launches use.
extern "C" int snn_conv2d_gather_plan(int mode, int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                                      int stride, int pad, int64_t ld_in, int64_t ld_out, int align_bits, int has_split_image,
                                      int has_addend, int has_addend2, int frames_per_step, int precision, int phase,
                                      int* out) {
    if (!out) return 1;
    for (int i = 0; i < 17; ++i) out[i] = 0;
    if (mode < 0 || mode > 2 || check_conv_shape("snn_conv2d_gather_plan", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad))
        return 1;
    const bool dgrad = mode == 1, xsp = mode == 2;
    const bool sbf = precision == SNN_PREC_BF16S;
    const unsigned align = (unsigned)align_bits;
    ConvGeom g;
    int split, nphases = 1, bn_chunks = 0;
    if (!dgrad) {
        if (xsp ? precision != SNN_PREC_FP16X3
                : !(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X6 || precision == SNN_PREC_FP16X3 ||
                    precision == SNN_PREC_BF16X1 || sbf))
            return 1;
        if ((has_split_image && precision != SNN_PREC_FP16X3) || ld_in < Cin || ld_out < Cout || has_addend2) return 1;
        if (frames_per_step > 0 && (N % frames_per_step != 0 || has_addend)) return 1;
        if (xsp && (has_addend || has_split_image ||
                    !spikes_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld_in)))
            return 1;
        g = gather_fwd_geom(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld_in, ld_out);
        if (!(N * (int64_t)H * W < 0x7fffffffLL && (int64_t)g.Ktot * Cin < 0xffffffffLL)) return 1;
        if (!xsp) {
            const FirstPlan fp = Cin == 2 && KH == 3 && KW == 3
                                     ? snn_first_layer_plan(N, H, W, Ho, Wo, Cout, stride, pad, frames_per_step > 0 ? frames_per_step : 0, false, 0)
                                     : FirstPlan{};
            if (fwd_takes_first(fp, has_addend != 0, ld_in, ld_out, W, Wo, sbf, align)) return 1;   // k_conv_first: snn_conv_first_plan
            if (sbf && Cin % 32 != 0) return 1;
        }
        bn_chunks = gather_bn_plan(frames_per_step > 0, frames_per_step > 0 ? (int64_t)frames_per_step * Ho * Wo : 0);
        split = sbf ? 5 : precision;
    } else {
        if (!(precision == SNN_PREC_FP32 || precision == SNN_PREC_BF16X3 || precision == SNN_PREC_BF16X1 || sbf)) return 1;
        if ((has_split_image && precision != SNN_PREC_BF16X3) || ld_in < Cout || ld_out < Cin || frames_per_step > 0) return 1;
        g = gather_dgrad_geom(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld_in, ld_out);
        if (!(N * (int64_t)Ho * Wo < 0x7fffffffLL && (int64_t)g.KtotFull * Cout < 0xffffffffLL)) return 1;
        const int nph = stride < H ? stride : H, npw = stride < W ? stride : W;
        nphases = nph * npw;
        if (phase < 0 || phase >= nphases) return 1;
        gather_dgrad_phase(g, phase / npw, phase % npw);
        split = sbf ? 5 : (precision == SNN_PREC_BF16X1 ? 5 : (precision != 0 ? 2 : 0));
    }
    const GatherPlan p = gather_plan(g, dgrad, split, sbf, xsp, align, has_split_image != 0, has_addend != 0, has_addend2 != 0);
    if (!p.ok) return 1;
    const int64_t idle = p.blocks - (int64_t)p.mtiles * p.ntiles;
    const int v[17] = {1, p.loader, p.bn, p.out_vec, p.mtiles, p.mtiles_per_xcd, p.ntiles, (int)p.blocks, (int)idle, g.nkh, g.nkw,
                       g.Ktot, g.OHc, g.OWc, nphases, bn_chunks, bn_chunks ? BM : 0};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
    return 0;
}

// ---- convolutions over spikes that were never stored (see k_conv_gather XSP, include/snn_hip.h)
extern "C" int snn_conv2d_spikes_supported(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                                           int stride, int pad, int64_t ld, int fwd_precision, int bwd_precision) {
    return (fwd_precision == SNN_PREC_FP16X3 && bwd_precision == SNN_PREC_BF16X3 &&
            spikes_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld)) ? 1 : 0;
}

extern "C" int snn_conv1x1_spikes_supported(int64_t N, int H, int W, int Cin, int Cout, int64_t ld, int fwd_precision,
                                            int bwd_precision) {
    return snn_conv2d_spikes_supported(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, ld, fwd_precision, bwd_precision);
}

extern "C" int snn_conv2d_spikes_fwd(const float* vdec, int64_t ld, float v_th, const float* w, float* y, int64_t ldy,
                                     int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                     int pad, double* bn_partial, int frames_per_step, int* bn_layout, void* stream) {
    SNN_REQUIRE(vdec && w && y, "snn_conv2d_spikes_fwd: null pointer");
    SNN_REQUIRE(v_th >= 0.0f, "snn_conv2d_spikes_fwd: a negative threshold would turn padding into spikes");
    if (check_conv_shape("snn_conv2d_spikes_fwd", N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad)) return 1;
    SNN_REQUIRE(spikes_shape_ok(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld) && ldy >= Cout,
                "snn_conv2d_spikes_fwd: shape not covered (ask snn_conv2d_spikes_supported)");
    SNN_REQUIRE(!bn_partial || (bn_layout && frames_per_step > 0 && N % frames_per_step == 0),
                "snn_conv2d_spikes_fwd: statistics need bn_layout and a frames_per_step that divides N");
    if (bn_layout) bn_layout[0] = bn_layout[1] = 0;
    ConvGeom g = gather_fwd_geom(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, ld, ldy);
    g.x_th = v_th;
    const int64_t step_rows = bn_partial ? (int64_t)frames_per_step * Ho * Wo : 0;
    if (const int chunks = gather_bn_plan(bn_partial != nullptr, step_rows)) {
        g.bn_partial = bn_partial;
        g.bn_rows = step_rows;
        g.bn_chunks = chunks;
        bn_layout[0] = g.bn_chunks;
        bn_layout[1] = BM;
    }
    return launch_gather(false, 4, false, true, vdec, w, nullptr, y, g, nullptr, 0, nullptr, 0, (hipStream_t)stream,
                         "snn_conv2d_spikes_fwd");
}

extern "C" int snn_conv1x1_spikes_fwd(const float* vdec, int64_t ld, float v_th, const float* w, float* y, int64_t ldy,
                                      int64_t N, int H, int W, int Cin, int Cout, void* stream) {
    return snn_conv2d_spikes_fwd(vdec, ld, v_th, w, y, ldy, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, nullptr, 0, nullptr, stream);
}

// ---- the 1x1 convolution over the spike bit mask of a scan with SNN_SCAN_SPIKE_MASK (see k_conv_gather XM, include/snn_hip.h)
namespace {
// the forward launch's own requirements, shared by the query and the call: shape, stride, plan and pointer alignment
static bool mask_fwd_ok(int64_t N, int H, int W, int Cin, int Cout, const uint32_t* mask, int64_t ld_mask, const float* w,
                        const float* y, int64_t ldy) {
    if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 32 == 0 && ld_mask >= Cin / 32 && ldy >= Cout &&
          N * (int64_t)H * W < 0x7fffffffLL && (int64_t)Cin * Cin < 0xffffffffLL && mask && w && y))
        return false;
    const ConvGeom g = gather_fwd_geom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, ld_mask, ldy);
    unsigned align = gather_align_bits(mask, w, nullptr, y, nullptr, 0, nullptr, 0) & ~(kAlignIn16 | kAlignIn8);
    if (aligned(4, {mask})) align |= kAlignIn16;
    const GatherPlan p = gather_plan(g, false, 4, false, true, align, false, false, false, true);
    return p.ok && p.loader == kLoadXM;
}
}  // namespace

extern "C" int snn_conv1x1_mask_supported(int64_t N, int H, int W, int Cin, int Cout, const uint32_t* mask, int64_t ld_mask,
                                          const float* w, const float* y, int64_t ldy, const float* dy, int64_t lddy,
                                          const float* dw, int fwd_precision, int bwd_precision) {
    if (fwd_precision != SNN_PREC_FP16X3 || bwd_precision != SNN_PREC_BF16X3 || !mask) return 0;
    if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 32 == 0 && ld_mask >= Cin / 32 && aligned(4, {mask}) &&
          N * (int64_t)H * W * ld_mask * 4 < 0x7fffffffLL))
        return 0;
    if ((w || y) && !mask_fwd_ok(N, H, W, Cin, Cout, mask, ld_mask, w, y, ldy)) return 0;
    if ((dy || dw) && !snn_wgrad_mask_ok(N, H, W, Cin, Cout, mask, ld_mask, dy, lddy, dw)) return 0;
    return 1;
}

extern "C" int snn_conv1x1_mask_fwd(const uint32_t* mask, int64_t ld_mask, const float* w, float* y, int64_t ldy, int64_t N,
                                    int H, int W, int Cin, int Cout, void* stream) {
    SNN_REQUIRE(mask && w && y, "snn_conv1x1_mask_fwd: null pointer");
    if (check_conv_shape("snn_conv1x1_mask_fwd", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0)) return 1;
    SNN_REQUIRE(mask_fwd_ok(N, H, W, Cin, Cout, mask, ld_mask, w, y, ldy),
                "snn_conv1x1_mask_fwd: call not covered (ask snn_conv1x1_mask_supported)");
    const ConvGeom g = gather_fwd_geom(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, ld_mask, ldy);
    return launch_gather(false, 4, false, true, reinterpret_cast<const float*>(mask), w, nullptr, y, g, nullptr, 0, nullptr, 0,
                         (hipStream_t)stream, "snn_conv1x1_mask_fwd", true);
}
