/*
 * snn_hip.h - C ABI of the MI355X (gfx950) spiking-CNN forward/backward step.
 *
 * This is the drop-in boundary below the reference's operator API
 * (models.generator {Conv, Norm, LIF, LI, Pool, ...}).  The reference has no
 * native code of its own: every entry point below replaces the ATen / norse
 * call sequence that one reference module issues per timestep, re-cut for a
 * layer-major / time-inner schedule (one call covers all T timesteps).
 * Citations are reference file:line (relative to the upstream tree).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (hipMalloc'ed by the caller, e.g. a
 *    torch storage); the library never allocates, frees or synchronises;
 *  - activations are channels-last: frame-major [N][H][W][C] with N = T*B
 *    frames ("T-major": frame index = t*B + b); `ld*` is the element stride
 *    between two pixels of a buffer (>= C; lets an op read / write a channel
 *    slice of a wider concat buffer, reference Dense merge generator.py:157-161);
 *  - conv weights are [Cout][KH][KW][Cin] (OHWI = torch channels_last memory
 *    of the reference's [Cout,Cin,KH,KW] parameter);
 *  - `stream` is a hipStream_t passed as void*;
 *  - return 0 on success, non-zero on error; snn_last_error() gives the text
 *    (thread-local).  Python wrappers turn non-zero into RuntimeError.
 *  - fp32 is the parity dtype (SNN_F32); per-(t,c) statistics are accumulated
 *    in fp64 like ATen's CPU batch-norm.
 */
#ifndef SNN_HIP_H
#define SNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNN_ABI_VERSION 20

/* neuron kinds for the fused affine+neuron temporal scan */
enum {
    SNN_NEURON_NONE = 0,   /* plain per-(t,c) affine (BatchNorm apply)            */
    SNN_NEURON_LIF = 1,    /* norse LIFCell step, layer_gen.py:232-235            */
    SNN_NEURON_LI = 2,     /* norse LICell step,  layer_gen.py:252-254            */
    SNN_NEURON_LI_TANH = 3,/* LICell followed by nn.Tanh, tiny_yolo.py:39-44      */
    SNN_NEURON_SLI = 4,    /* saturable leaky integrator, sli.py:110-126          */
    SNN_NEURON_SYNAPSE = 5 /* mediator-concentration synapse, synapse.py:73-103   */
};

/* Arithmetic of a convolution call (the `precision` argument of snn_conv2d_*).  Tensors in HBM and the accumulators
 * are fp32 in every mode; the modes differ in how the PRODUCTS are formed on the matrix cores:
 *   SNN_PREC_FP32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32): a k-ordered fmaf chain.               fwd, dgrad, wgrad
 *   SNN_PREC_BF16X3 operands split into bf16 hi + lo, product = hi*hi + hi*lo + lo*hi on the bf16 MFMA: relative
 *                   error ~2^-16 per product (measured 1e-5).  Default of the backward convolutions.   dgrad, wgrad
 *   SNN_PREC_BF16X6 three-way bf16 split of both operands (h + m + l = all 24 significant bits) and the six leading
 *                   products: fp32-grade (rel 5e-7 vs fp64) for any fp32 range.                                 fwd
 *   SNN_PREC_FP16X3 both operands split into two fp16 pieces (11 + 11 significant bits) after exact power-of-two
 *                   pre-scaling (weights x 2^8, activations x 2^4), products hh + hl + lh: relative error 2^-22
 *                   (measured 5e-7 vs fp64, equal to the fp32 MFMA's) at half the matrix work of BF16X6.  Range
 *                   contract: |x| < 4094 and |w| < 255 (beyond: inf/NaN in the output - visible, not silent);
 *                   values below |x| = 0.008 / |w| = 5e-4 keep an ABSOLUTE accuracy of 4e-9 / 2e-10 instead of 22
 *                   bits.  Default of the forward convolution (inputs are spikes / normalised activations).     fwd
 *   SNN_PREC_BF16X1 the opt-in THROUGHPUT mode ("bf16" of BASELINE configs[1]): every operand is rounded once to bf16
 *                   and multiplied as it is - one product, fp32 accumulation, fp32 tensors in HBM.  Relative error
 *                   2^-9 per product: NOT a parity mode (spike trains diverge from the fp32 reference within a few
 *                   layers; loss and gradients to ~1e-2).  Never a default.                     fwd, dgrad, wgrad
 *   SNN_PREC_BF16S  bf16 STORAGE (the opt-in throughput mode whose tensors are bf16 in HBM too): the activation
 *                   operands AND results of the call (x / y, dy / dx; every `float*` activation pointer of the
 *                   signature then addresses bf16 elements, pixel strides stay in ELEMENTS) are bf16, products are
 *                   single bf16 MFMA products (weights, fp32, are rounded to bf16 on the way in), accumulation and
 *                   BatchNorm statistics fp32 / fp64.  Weights, weight gradients, statistics, neuron state stay fp32.
 *                   Same tolerances class as SNN_PREC_BF16X1; never a default.  Covered shapes: the vectorised
 *                   (Cin % 32 == 0) implicit GEMM, the halo-resident 3x3 kernels, the event-frame kernels (input
 *                   frames fp32).                                                              fwd, dgrad, wgrad
 * The mode is an argument of every call - the library keeps no process-wide arithmetic state. */
enum { SNN_PREC_FP32 = 0, SNN_PREC_BF16X3 = 1, SNN_PREC_BF16X6 = 3, SNN_PREC_FP16X3 = 4, SNN_PREC_BF16X1 = 5,
       SNN_PREC_BF16S = 6 };

/* flags of snn_affine_neuron_fwd / _bwd */
enum { SNN_SCAN_WIDE_ADDRESSING = 1, /* bwd: use 64-bit pointer addressing even when one timestep of every tensor fits
                                        the 31-bit buffer offsets (the library switches by itself when it does not) */
       SNN_SCAN_LAST_STEP_ONLY = 2,  /* LIF / LI / LI+Tanh whose consumer keeps the last timestep only (the detection head,
                                        soda.py:141-144): fwd writes out[M][ldo] of step T-1 instead of [T][M][ldo];
                                        bwd takes g_out[M][ldg] (and, LI+Tanh, the saved output [M][C]) of that step,
                                        the output gradient of every earlier step being zero */
       SNN_SCAN_BF16_STORAGE = 4,    /* bf16-storage mode (see SNN_PREC_BF16S): the activation tensors of the call - fwd: y,
                                        out, addend, vdec; bwd: g_out, state, y, gx - are bf16 (pointers passed as float*,
                                        strides in elements); state (v, i), alpha / beta and the sums stay fp32.
                                        NONE / LIF / LI / LI+Tanh, C and strides multiples of 4 */
       SNN_SCAN_SPIKES_FROM_VDEC = 8,/* fwd, Norm -> LIF without a shortcut whose potentials are saved (vdec != NULL): write
                                        NO output tensor (out must be NULL) - the saved pre-reset potentials already hold
                                        the spikes, z = (v_dec > v_th), and the consumer forms them while it reads them
                                        (snn_conv1x1_spikes_fwd / _wgrad): 4 of the 12 bytes the scan moves per
                                        neuron-timestep never exist.  fp32 tensors, C and ldy multiples of 4 */
       SNN_SCAN_SUMS_FROM_STATE = 16,/* bwd, LIF from the initial state with `sums` wanted: y is NOT read (NULL allowed).
                                        The BatchNorm statistic the scan needs y for, sum(gx * y), is replaced by
                                        sum(gx * x) with the neuron's input x[t] = alpha*y[t] + beta rebuilt from the saved
                                        potentials (vd[t], vd[t-1], vd[t-2] and the reset rule determine x[t] to fp32
                                        rounding): 4 of the 16 bytes per neuron-timestep are never read.  The sums must
                                        then go through snn_bn_bwd_finalize_from_state.  Covered cases:
                                        snn_affine_neuron_bwd_sums_from_state().  The sequence must start from the
                                        initial state (v_leak, 0) - or carry the next flag */
       SNN_SCAN_STATE_LOOKBACK = 32, /* with SNN_SCAN_SUMS_FROM_STATE, for a SEGMENT [t0, t0 + T) of a longer saved
                                        sequence, t0 >= 2: `state` points at step t0 and state[-1], state[-2] (the two
                                        steps in front of it, same [M][C] layout) are read to rebuild the neuron state
                                        the segment starts from */
       SNN_SCAN_SPIKE_MASK = 32      /* fwd only (the value is shared with the bwd-only flag above; each direction refuses
                                        the other's meaning), together with SNN_SCAN_SPIKES_FROM_VDEC, through
                                        snn_affine_neuron_fwd_mask: the spikes also leave as ONE BIT per neuron,
                                        mask[T][M][ld_mask] of uint32 - bit (c & 31) of word (c >> 5) of a pixel's row is
                                        v_dec[t][m][c] > v_th (strict), taken from the value stored to vdec.  C % 32 == 0,
                                        ld_mask >= C / 32, mask 4-byte aligned; words c >> 5 >= C / 32 of a row are not
                                        written.  Read by the snn_conv1x1_mask_ entry points */ };

/* pooling kinds, layer_gen.py:139-173 / common.py:18-49 */
enum { SNN_POOL_AVG = 0, SNN_POOL_MAX = 1, SNN_POOL_SUM = 2 };

/* pointwise activations, layer_gen.py:257-284 */
enum { SNN_ACT_RELU = 0, SNN_ACT_SILU = 1, SNN_ACT_TANH = 2 };

/* Surrogate gradient dz/du of the LIF spike z = (u > 0), u = v_dec - v_th, a = alpha; every one has s(0) = 1:
 *   SNN_SURR_SUPER     1 / (a|u| + 1)^2        (SuperSpike; the default, and the only one that claims to restate norse)
 *   SNN_SURR_TRIANGLE  max(0, 1 - a|u|)
 *   SNN_SURR_SIGMOID   4 s(au) (1 - s(au)),  s(x) = 1 / (1 + exp(-x))
 *   SNN_SURR_ATAN      1 / (1 + (au)^2)
 * These definitions (normalisation and the meaning of alpha) are THIS project's own: like the rest of the LIF rule they
 * are "parity unpinned" - no norse source is at hand to compare them with. */
enum { SNN_SURR_SUPER = 0, SNN_SURR_TRIANGLE = 1, SNN_SURR_SIGMOID = 2, SNN_SURR_ATAN = 3 };

/* neuron constants exactly as norse rounds them in fp32 (oracle/neurons.py:neuron_constants) */
typedef struct snn_neuron_params {
    float c_mem;   /* dt * tau_mem_inv            (0.1)  */
    float c_syn;   /* -dt * tau_syn_inv           (-0.2) */
    float v_leak;  /* 0 */
    float v_th;    /* 1 */
    float v_reset; /* 0 */
    float alpha;   /* surrogate slope a (SuperSpike: 100) */
    float v_st;    /* SLI saturation potential, 1 (sli.py:38-39)                              */
    float tau_sec; /* synapse: mediator secretion rate 1/1e-3 (synapse.py:26-27)              */
    float tau_dis; /* synapse: mediator dissociation rate 1/5e-3 (synapse.py:29-30)           */
    float dt;      /* synapse integration step 1e-3 (synapse.py:77)                           */
    float sigma;   /* synapse inhibition, 0 = off (synapse.py:32-36)                          */
    /* ABI 20, LIF backward only (the forward is the same, bit for bit, whatever they hold).  Zero is the rule of every
     * earlier ABI, so a caller that zero-fills the tail of the struct computes what it always did. */
    int surrogate;      /* SNN_SURR_*                                                                              */
    int reset_detached; /* != 0: the spike inside the reset v = (1-z) v_dec + z v_reset is a constant of the backward
                           pass:  g_vd = g_v (1-z) + g_out s   instead of   g_v (1-z) + (g_out + g_v (v_reset - v_dec)) s */
} snn_neuron_params;

int snn_abi_version(void);
const char* snn_last_error(void);

/* ---------------------------------------------------------------- layout
 * [N][C][H][W] <-> [N][H][W][C].  Entry/exit adapters for callers that hold
 * the reference's NCHW event frames X[T,B,2,H,W] (soda.py:138-144). */
int snn_nchw_to_nhwc(const float* src, float* dst, int64_t N, int C, int H, int W, void* stream);
int snn_nhwc_to_nchw(const float* src, float* dst, int64_t N, int C, int H, int W, void* stream);
/* weights [Cout][KH][KW][Cin] -> [Cin][KH][KW][Cout] (operand of the data-gradient conv) */
int snn_weight_transpose(const float* w, float* wt, int Cout, int KH, int KW, int Cin, void* stream);
/* the same for every conv weight of a flat parameter buffer in ONE launch: table[l] = {element offset, Cout, KH*KW, Cin}
 * (device memory, int64); flat_wt mirrors the offsets of flat_w.  A layer is indexed in 32 bits: Cout*KH*KW*Cin < 2^31
 * (the table is device memory: the caller that builds it checks). */
int snn_weight_transpose_batched(const float* flat_w, float* flat_wt, const int64_t* table, int n_layers, void* stream);
/* Pre-split weight image for the convolution kernels: every group of 4 consecutive floats of `w` (n floats, n % 4 == 0,
 * both buffers 16-byte aligned, `out` as large as `w`) becomes 4 high + 4 low 16-bit pieces - fp16 pieces of w * 2^8 for
 * SNN_PREC_FP16X3 (forward, apply to the OHWI weights), bf16 pieces for SNN_PREC_BF16X3 (data gradient, apply to the
 * transposed weights) - exactly the pieces the kernels would derive themselves.  Elementwise, so ONE call over a flat
 * parameter buffer serves every layer whose weight rows start on a multiple of 4 floats; redo after an optimiser step. */
int snn_weight_presplit(const float* w, void* out, int64_t n, int precision, void* stream);

/* ---------------------------------------------------------------- convolution
 * Replaces nn.Conv2d(bias=False, padding=int(k/2), stride=s) of layer_gen.py:129-136
 * (forward) and its autograd (ATen conv backward) for all T*B frames at once.
 * Implicit GEMM on the matrix cores, LDS-tiled; `precision` = SNN_PREC_* (above).
 *
 * fwd  : y[n,ho,wo,co]   = sum_{kh,kw,ci} x[n, ho*s-pad+kh, wo*s-pad+kw, ci] * w[co,kh,kw,ci]
 * dgrad: dx[n,hi,wi,ci]  = sum_{kh,kw,co} dy[n,(hi+pad-kh)/s,(wi+pad-kw)/s,co] * wt[ci,kh,kw,co]
 *        (terms with a non-integral or out-of-range source pixel are 0; wt from snn_weight_transpose)
 * wgrad: dw[co,kh,kw,ci] = sum_{n,ho,wo} dy[n,ho,wo,co] * x[n, ho*s-pad+kh, wo*s-pad+kw, ci]
 *        partial sums over pixel ranges go to `workspace` ([splitk][Cout*KH*KW*Cin] floats, splitk from
 *        snn_conv2d_wgrad_splitk), then reduced in fixed order (bitwise reproducible).  3x3 / pad 1 / stride 1|2
 *        layers with Cin, Cout multiples of 32 take the halo-resident kernel (csrc/wgrad_halo.hip), the rest the
 *        implicit-GEMM kernel.
 * fwd / dgrad `addend` (may be NULL): a tensor of the result's shape with pixel stride ld_addend that is added
 *   in the epilogue (result = conv + addend); passing the destination itself accumulates in place.  This
 *   fuses the gradient sum of a tensor consumed by several branches (generator.py:181-187) into the dgrad.
 * wgrad accumulate != 0 : the result is added to dw instead of overwriting it.
 * fwd `bn_partial` (may be NULL): the convolution is followed by a train-mode BatchNorm (layer_gen.py:211-214 after
 *   :129-136) whose per-timestep statistics are then taken from the values on their way to the store instead of a
 *   second pass over y.  The N frames are T = N / frames_per_step timesteps of frames_per_step frames; bn_partial
 *   holds snn_conv2d_fwd_bn_partial_size() doubles; on return (host side, no synchronisation) bn_layout[0] =
 *   chunks per timestep and bn_layout[1] = rows per chunk, the two layout arguments of snn_bn_stats_finalize /
 *   snn_bn_stats_reduce.  bn_layout[0] == 0: this shape's kernel did not produce them - run snn_bn_stats.
 * fwd `w_split` / dgrad `wt_split` (may be NULL): the pre-split image of the same weights (snn_weight_presplit below),
 *   valid for SNN_PREC_FP16X3 (fwd) / SNN_PREC_BF16X3 (dgrad) only.  With it the kernels stop converting the weight
 *   tile in every block; the results are bit-identical to the conversion on the fly.  Shapes whose kernel cannot use
 *   it read `w` / `wt` as before, so both pointers are always passed. */
/* Weight gradient with the BatchNorm-backward affine applied while dy is READ (no materialised dy): the gradient that
 * reaches the convolution through a train-mode BatchNorm (layer_gen.py:211-214) is dy = A[t][c]*gx + B[t][c]*y + C[t][c]
 * (snn_bn_bwd_apply); when nothing else consumes dy - the event-frame layer, whose input needs no gradient - the
 * weight-gradient kernel forms it on the fly from gx (the scan's output, pixel stride ldgx), the saved convolution
 * output y (ldy) and coef = [3][T][Cout] (A, B, C planes), t = frame / frames_per_step.  Same statement, same
 * roundings as snn_bn_bwd_apply + snn_conv2d_wgrad.  snn_conv2d_wgrad_bn_supported: 1 for the shapes covered (the
 * event-frame row kernel: Cin = 2, 3x3); workspace / splitk as for snn_conv2d_wgrad. */
int snn_conv2d_wgrad_bn_supported(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                  int pad);
int snn_conv2d_wgrad_bn(const float* x, int64_t ldx, const float* gx, int64_t ldgx, const float* y, int64_t ldy,
                        const float* coef, int T, int frames_per_step, float* dw, int64_t N, int H, int W, int Cin, int Ho,
                        int Wo, int Cout, int KH, int KW, int stride, int pad, int accumulate, float* workspace, int splitk,
                        void* stream);
/* ---- Halo-resident 3x3 / stride 1 / pad 1 convolution (csrc/conv_halo.hip): forward AND data gradient of the 32-, 64- and
 * 128-channel layers (reference models/modules/layer_gen.py:129-136, nn.Conv2d(C, C', 3, padding=1, bias=False)).
 * The activation halo of a tile is fetched and split into its 16-bit pieces once per 32-channel chunk (the implicit
 * GEMM does both once per tap); the weights arrive by LDS-DMA from an image in MFMA-fragment order.
 *   snn_conv3x3_halo_supported : 1 when the kernel covers the shape (Cin % 32 == 0; Cout = 32 or a multiple of 64; rows of
 *                                up to 78 pixels as padded strips, longer rows as 4 x 32 rectangles); otherwise use
 *                                snn_conv2d_fwd / snn_conv2d_dgrad.
 *   snn_weight_frag_image_batched : builds the weight images of n layers in ONE launch.  table (device, int64) rows
 *       {float offset of the layer's [O][3][3][I] matrix in flat_src, BYTE offset of its image in flat_dst, O, I}; an
 *       image takes snn_weight_frag_image_bytes(O, I) = 9*O*I*4 bytes (as many as the weights); max_threads = the
 *       largest 9 * (I/32) * (O/32) * 128 of the table.  Forward: src = the OHWI weights, flip = 0, SNN_PREC_FP16X3.
 *       Data gradient: src = the transposed weights [Cin][KH][KW][Cout] (snn_weight_transpose), flip = 1 (mirrored
 *       taps), SNN_PREC_BF16X3.  Redo after every optimiser step.
 *   snn_conv3x3_halo : y[N][H][W][ldy] = conv3x3(x[N][H][W][ldx], image) (+ addend + addend2), Cin input and Cout output
 *       channels (for a data gradient: x = dy, "Cin" = the layer's Cout and vice versa).  precision = the image's.
 *       bn_partial / frames_per_step / bn_layout as for snn_conv2d_fwd (forward arithmetic only, no addend); the partials
 *       hold snn_conv2d_fwd_bn_partial_size() doubles, bn_layout[0] = snn_conv3x3_halo_bn_chunks(), bn_layout[1] = 0. */
/* Data gradient of a 3x3 / stride 2 / pad 1 convolution in ONE pass over dy (csrc/conv_halo.hip, k_conv_s2dgrad3): the
 * four stride-phase classes of dx are produced from one staged dy halo instead of four launches that each gather dy
 * again.  wt_image = the layer's data-gradient image (snn_weight_frag_image_batched of the transposed weights, flip = 1,
 * SNN_PREC_BF16X3 - the image the stride-1 data gradient uses).  dx[N][H][W][lddx] (Cin channels) from dy[N][Ho][Wo][lddy]
 * (Cout channels), Ho = (H-1)/2 + 1; addend / addend2 as for snn_conv2d_dgrad.  bf16 x 3 arithmetic, or bf16 storage.
 * Covers Cout % 32 == 0, Cin % 64 == 0, any width (dy rows of up to 157 cells as padded strips, longer ones as rectangles). */
int snn_conv3x3_s2_dgrad_supported(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout);
/* Host-only plan queries of the halo-resident kernels: they read the plan function the launch reads.
 *   snn_conv3x3_halo_plan : the grid snn_conv3x3_halo launches for the shape (frames_per_step > 0: with statistics
 *       partials, tiles never straddle two timesteps; <= 0: without).  snn_conv3x3_s2_dgrad_plan : the same for
 *       snn_conv3x3_s2_dgrad (arguments as snn_conv3x3_s2_dgrad_supported).  out[7] = { mode (1 padded-strip tiles of
 *       128 cells, 2 rectangles of 4 x 32 pixels), output channels per block (32, 64, 128), tiles, tiles per group (=
 *       per timestep with statistics), tiles per XCD share, channel tiles, blocks (whole groups of 8: the blocks past the
 *       last tile return at once) }.  Return 0, or 1 (out[0] = 0) for a shape the launch would refuse.
 *   snn_conv2d_wgrad_halo_plan : the halo-resident weight-gradient plan snn_conv2d_wgrad runs for a 3x3 / pad 1 layer on a
 *       device with num_cu compute units (0: the current device's; 256 without one).  out[16] = { ok (0: the implicit
 *       GEMM takes the shape), R, CW (patch rows / columns), wco, wk (waves over output channels / over K-steps), nks
 *       (16-pixel K-steps per patch), npr, npc (patches per image column / row), patches, splits, pps (patches per
 *       split), HR, HC (halo rows / columns), HWD (LDS row pitch in pixels), tiles_co, tiles_ci }.  Returns 0. */
int snn_conv3x3_s2_dgrad_plan(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int* out);
int snn_conv3x3_halo_plan(int64_t N, int H, int W, int Cin, int Cout, int frames_per_step, int* out);
int snn_conv2d_wgrad_halo_plan(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int stride, int num_cu, int* out);
/* Host-only plan query of the event-frame row kernel (k_conv_first: Cin = 2, 3x3, Cout = 4 * 2^k <= 256, W + 2 pad <= 1408):
 * the plan snn_conv2d_fwd (frames_per_step > 0: with statistics partials; <= 0: without), snn_conv2d_wgrad and
 * snn_conv2d_wgrad_bn (wgrad = 1) launch for the shape on a device with num_cu compute units (0: the current device's;
 * 256 without one).  It reads the plan function the launches read.  out[10] = { ok (0: another kernel takes the shape),
 * rs (output rows staged per barrier pair, 1..4), LW (padded input row width W + 2 pad), cgs (channel groups Cout / 4),
 * PP (pixel lanes 256 / cgs), blocks (the grid; weight gradient: = snn_conv2d_wgrad_splitk, one workspace slab each),
 * group_rows, group_blocks (rows of a group - a timestep with statistics, else all N * Ho - and the blocks that walk
 * them; = bn_layout[0] with statistics), the most rows a block walks, the rows of that block's last stage }.
 * Returns 0, or 1 (out[0] = 0) for a shape the kernel does not take.  Pointer alignment and strides are the call's. */
int snn_conv_first_plan(int64_t N, int H, int W, int Ho, int Wo, int Cout, int stride, int pad, int frames_per_step,
                        int wgrad, int num_cu, int* out);
int snn_conv3x3_s2_dgrad(const float* dy, int64_t lddy, const void* wt_image, float* dx, int64_t lddx, int64_t N, int H, int W,
                         int Cin, int Ho, int Wo, int Cout, const float* addend, int64_t ld_addend, const float* addend2,
                         int64_t ld_addend2, int precision /* SNN_PREC_BF16X3 | SNN_PREC_BF16S */, void* stream);
int snn_conv3x3_halo_supported(int64_t N, int H, int W, int Cin, int Cout);
int64_t snn_conv3x3_halo_bn_chunks(int frames_per_step, int H, int W);
size_t snn_weight_frag_image_bytes(int O, int I);
int snn_weight_frag_image_batched(const float* flat_src, void* flat_dst, const int64_t* table, int n, int max_threads,
                                  int flip, int precision, void* stream);
int snn_conv3x3_halo(const float* x, int64_t ldx, const void* w_image, float* y, int64_t ldy, int64_t N, int H, int W,
                     int Cin, int Cout, const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2,
                     double* bn_partial, int frames_per_step, int* bn_layout, int precision, void* stream);
size_t snn_conv2d_fwd_bn_partial_size(int64_t N, int frames_per_step, int Ho, int Wo, int Cout);
int snn_conv2d_fwd(const float* x, int64_t ldx, const float* w, const void* w_split, float* y, int64_t ldy,
                   int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                   int KH, int KW, int stride, int pad, const float* addend, int64_t ld_addend,
                   double* bn_partial, int frames_per_step, int* bn_layout, int precision, void* stream);
/* dgrad takes TWO optional addends (dx = conv^T(dy) + addend + addend2): a tensor consumed by a convolution, a
 * residual shortcut and a Dense pass-through (the YOLO bottleneck inside a C2f block) gets its whole gradient in one
 * epilogue instead of two extra add passes. */
int snn_conv2d_dgrad(const float* dy, int64_t lddy, const float* wt, const void* wt_split, float* dx, int64_t lddx,
                     int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                     int KH, int KW, int stride, int pad, const float* addend, int64_t ld_addend,
                     const float* addend2, int64_t ld_addend2, int precision, void* stream);
int snn_conv2d_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw,
                     int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                     int KH, int KW, int stride, int pad, int accumulate,
                     float* workspace, int splitk, int precision, void* stream);
/* number of workspace slabs snn_conv2d_wgrad wants for this shape and precision (workspace = splitk*Cout*KH*KW*Cin
 * floats); same geometry arguments as snn_conv2d_wgrad; host-only, callable without a device */
int snn_conv2d_wgrad_splitk(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                            int stride, int pad, int precision);
/* which kernel snn_conv2d_wgrad takes for this shape: 0 implicit GEMM (k_conv_wgrad_pipe), 1 halo-resident
 * (k_conv_wgrad_halo), 2 event-frame row kernel (k_conv_first); host-only - labels of the measurement tools */
int snn_conv2d_wgrad_kernel(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                            int precision);
/* Host-only plan queries of the implicit-GEMM kernels (k_conv_gather; k_conv_wgrad_pipe / k_conv_wgrad and the slab
 * reducers): they read the plan functions the launches read and are callable without a device.  `align_bits` carries what a
 * launch derives from its pointers: 1 / 2 the gathered tensor (x; dy of a data gradient) is 16- / 8-byte aligned, 4 the
 * weight matrix is 16-byte aligned, 8 / 16 the produced tensor (y, dx; for snn_conv2d_wgrad_plan: dy) is 16- / 8-byte
 * aligned, 32 / 64 the first addend is 16- / 8-byte aligned AND its pixel stride a multiple of 4 (snn_conv2d_wgrad_plan: 32 =
 * dw and the workspace are 16-byte aligned), 128 / 256 the same for the second addend, 512 the pre-split weight image is
 * 16-byte aligned; 1023 = everything aligned.  The 8-byte bits matter for SNN_PREC_BF16S only.
 *   snn_conv2d_gather_plan : mode 0 snn_conv2d_fwd, 1 one stride phase of snn_conv2d_dgrad (phase = ph * min(stride, W) + pw,
 *       the launch order), 2 snn_conv2d_spikes_fwd; geometry arguments as for those calls, ld_in / ld_out the pixel strides
 *       of the gathered / produced tensor; frames_per_step > 0: a forward with statistics partials.  out[17] = { ok, loader
 *       (0 scalar, 1 16-byte vectors, 2 pipelined buffer loads, 3 the same with the pre-split weight image, 4 bf16 storage,
 *       5 spike operand), output channels per block (32, 64, 128), out_vec (16-byte stores), pixel tiles of 128, pixel
 *       tiles per XCD share, channel tiles, blocks (= 8 * tiles per share * channel tiles), idle blocks past the last
 *       tile, nkh, nkw (taps of this phase; KH, KW forward), k extent of this phase, OHc, OWc (pixel rows / columns of this
 *       phase), phases of the call, statistics chunks per timestep, rows per chunk (0, 0: no partials from this kernel) }.
 *       Returns 0, or 1 (out[0] = 0) for a call the entry point refuses or hands to another kernel (the event-frame
 *       layer: snn_conv_first_plan).
 *   snn_conv2d_wgrad_plan : snn_conv2d_wgrad (spikes = 1: snn_conv2d_spikes_wgrad) on a device with num_cu compute units
 *       (0: the current device's; 256 without one) with splitk = snn_conv2d_wgrad_splitk.  out[18] = { ok, kernel (0
 *       pipelined k_conv_wgrad_pipe, 1 vectorised k_conv_wgrad, 2 scalar k_conv_wgrad, 3 halo-resident, 4 event-frame row
 *       kernel), tile id, bm, bn (block tile over Cout x (tap, ci)), tiles over Cout, tiles over (tap, ci), pixels per LDS
 *       stage (32 / 64), splitk, pixels per split, pixels of the last split that owns any, splits that own none (zero
 *       slabs), reducer (0 k_wgrad_reduce, 1 k_wgrad_reduce_once, 2 k_wgrad_reduce4 in two passes, 3 in one pass), KG
 *       (thread groups sharing an element's slabs), non-empty row groups, slab rows per group, reducer blocks, grid of the
 *       convolution kernel }.  For kernels 3 / 4 only splitk and the reducer fields are filled (snn_conv2d_wgrad_halo_plan /
 *       snn_conv_first_plan describe the rest; whether the halo-resident kernel can address the buffers is the launch's
 *       check - if not, the implicit GEMM runs with the same splitk).  Returns 0, or 1 (out[0] = 0) for a refused call. */
int snn_conv2d_gather_plan(int mode, int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                           int pad, int64_t ld_in, int64_t ld_out, int align_bits, int has_split_image, int has_addend,
                           int has_addend2, int frames_per_step, int precision, int phase, int* out);
int snn_conv2d_wgrad_plan(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                          int64_t ldx, int64_t lddy, int align_bits, int precision, int spikes, int num_cu, int* out);
/* ---- 1x1 convolutions over spikes that were never stored.  The stage-entry layers of the generated nets are
 * Conv -> Norm -> LIF feeding only 1x1 convolutions (reference models/tiny_yolo.py:76-85 behind :16-21); their LIF
 * (models/modules/layer_gen.py:232-235) saves v_dec for its backward pass anyway, so the spike tensor z = (v_dec > v_th)
 * is not written (SNN_SCAN_SPIKES_FROM_VDEC) and these entry points take the POTENTIALS as their input tensor:
 *   snn_conv1x1_spikes_fwd   : y[N][H][W][ldy] (Cout channels) = conv1x1(z, w[Cout][Cin]), fp16 x 3 arithmetic - a spike
 *                              is exact in one fp16 piece, so two of the three products are issued; same bits as
 *                              snn_conv2d_fwd(z, ...)
 *   snn_conv1x1_spikes_wgrad : dw[Cout][Cin] (+)= sum_pixels dy z^T, bf16 x 3 arithmetic (two products); workspace / splitk
 *                              as for snn_conv2d_wgrad with KH = KW = 1 (snn_conv2d_wgrad_splitk); same bits as
 *                              snn_conv2d_wgrad(z, ...)
 *   snn_conv1x1_spikes_supported : 1 for the shapes covered (Cin % 32 == 0, Cout % 4 == 0, ld % 4 == 0, the two default
 *                              arithmetics); otherwise the layer must write its spikes.
 * v_th >= 0 (padding rows read as potential 0 and must not spike).  The data gradient needs no input tensor. */
int snn_conv1x1_spikes_supported(int64_t N, int H, int W, int Cin, int Cout, int64_t ld, int fwd_precision,
                                 int bwd_precision);
int snn_conv1x1_spikes_fwd(const float* vdec, int64_t ld, float v_th, const float* w, float* y, int64_t ldy, int64_t N, int H,
                           int W, int Cin, int Cout, void* stream);
int snn_conv1x1_spikes_wgrad(const float* vdec, int64_t ld, float v_th, const float* dy, int64_t lddy, float* dw, int64_t N,
                             int H, int W, int Cin, int Cout, int accumulate, float* workspace, int splitk, void* stream);

/* The same for ANY convolution the pipelined implicit GEMM covers (KH, KW <= 5, Cin % 32 == 0, Cout % 4 == 0) - a plain
 * `Conv -> Norm -> LIF -> Conv` stack (models/modules/layer_gen.py:106-136 / 211-235: the deep backbones of BASELINE
 * configs[4]) writes no spike tensor between its layers:
 *   snn_conv2d_spikes_fwd   : as snn_conv2d_fwd on z = (vdec > v_th), fp16 x 3 arithmetic with two products; bn_partial /
 *                             frames_per_step / bn_layout as there
 *   snn_conv2d_spikes_wgrad : as snn_conv2d_wgrad (workspace / splitk from snn_conv2d_wgrad_splitk, SNN_PREC_BF16X3); 3x3
 *                             layers the halo-resident weight gradient covers take it (two products)
 *   snn_conv3x3_halo_spikes : the halo-resident 3x3 / stride 1 / pad 1 forward (snn_conv3x3_halo, fp16 x 3 image) on the
 *                             potentials; shapes: snn_conv3x3_halo_supported
 * The *_supported queries see shapes and strides only.  The implicit-GEMM kernels behind snn_conv2d_spikes_fwd /
 * snn_conv1x1_spikes_fwd also need 16-byte aligned potentials and weight, the weight gradients 16-byte aligned potentials
 * and dy with lddy % 4 == 0; a call outside that is refused on the host (error, nothing launched) - the caller writes
 * the spikes and takes snn_conv2d_fwd / snn_conv2d_wgrad instead (functional._spikes_fwd_ok / _spikes_wgrad_ok). */
int snn_conv2d_spikes_supported(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                int pad, int64_t ld, int fwd_precision, int bwd_precision);
int snn_conv2d_spikes_fwd(const float* vdec, int64_t ld, float v_th, const float* w, float* y, int64_t ldy, int64_t N, int H,
                          int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, double* bn_partial,
                          int frames_per_step, int* bn_layout, void* stream);
int snn_conv2d_spikes_wgrad(const float* vdec, int64_t ld, float v_th, const float* dy, int64_t lddy, float* dw, int64_t N,
                            int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                            int accumulate, float* workspace, int splitk, void* stream);
int snn_conv3x3_halo_spikes(const float* vdec, int64_t ld, float v_th, const void* w_image, float* y, int64_t ldy, int64_t N,
                            int H, int W, int Cin, int Cout, double* bn_partial, int frames_per_step, int* bn_layout,
                            void* stream);

/* ---- ... and over the spike BIT MASK a scan with SNN_SCAN_SPIKE_MASK wrote: mask[N * H * W][ld_mask] of uint32, bit
 * (c & 31) of word (c >> 5) of a pixel's row = spike of channel c.  The three calls mirror the snn_conv1x1_spikes_ ones with
 * (mask, ld_mask) in place of (vdec, ld, v_th); they move 1 bit instead of 32 per input element - one 4-byte load per pixel
 * and 32-channel chunk, expanded to the matrix-core operand in registers - and run the arithmetic of the potentials-fed
 * calls in their order: y and dw are bit-identical to theirs (same tile plans, split-K and ordered slab reduction).
 *   snn_conv1x1_mask_supported : 1 when BOTH launches the non-NULL pointers describe are covered: it checks everything
 *                              they hard-require - the two default arithmetics, Cin % 32 == 0, ld_mask >= Cin / 32, the mask
 *                              4-byte aligned and below 2 GiB; forward (w and y given): w 16-byte aligned, ldy >= Cout;
 *                              weight gradient (dy and dw given): Cout % 4 == 0, lddy % 4 == 0, lddy >= Cout, dy 16-byte
 *                              aligned, the pixels of a split below 2 GiB of dy.  A NULL w / y (dy / dw) leaves that launch
 *                              unchecked.  After a 1 the corresponding launch does not refuse; after a 0 the caller takes
 *                              the potentials (snn_conv1x1_spikes_fwd / _wgrad), which the scan wrote all the same. */
int snn_conv1x1_mask_supported(int64_t N, int H, int W, int Cin, int Cout, const uint32_t* mask, int64_t ld_mask,
                               const float* w, const float* y, int64_t ldy, const float* dy, int64_t lddy, const float* dw,
                               int fwd_precision, int bwd_precision);
int snn_conv1x1_mask_fwd(const uint32_t* mask, int64_t ld_mask, const float* w, float* y, int64_t ldy, int64_t N, int H, int W,
                         int Cin, int Cout, void* stream);
int snn_conv1x1_mask_wgrad(const uint32_t* mask, int64_t ld_mask, const float* dy, int64_t lddy, float* dw, int64_t N, int H,
                           int W, int Cin, int Cout, int accumulate, float* workspace, int splitk, void* stream);

/* ---- BOTH gradients of a 1x1 / stride 1 / pad 0 convolution from one pass over dy.  The weight-gradient kernel
 * has every stage of dy in LDS; where one block owns all output channels (Cout <= 128) it also forms the data gradient of
 * the stage, dx = dy wt^T + addend + addend2, from the same LDS images.  SNN_PREC_BF16X3 on fp32 tensors only.  Results
 * are bit-identical to the separate calls given the same splitk: dx to snn_conv2d_dgrad(dy, wt, NULL, ...), dw to
 * snn_conv2d_wgrad (snn_conv1x1_mask_wgrad for the mask form).
 *   snn_conv1x1_bwd       : x fp32 [N*H*W][ldx]; the arguments of snn_conv2d_dgrad and snn_conv2d_wgrad merged.  wt is the
 *                           transposed weight [Cin][Cout]; workspace = splitk * Cout * Cin floats, splitk from
 *                           snn_conv2d_wgrad_splitk.  dw == NULL: the slabs stay in the workspace and
 *                           snn_conv2d_wgrad_reduce sums them later - on another stream if the caller orders the two.
 *   snn_conv1x1_mask_bwd  : the same over the spike bit mask of the scan in front (snn_conv1x1_mask_wgrad's operand).
 *   snn_conv1x1_bwd_supported : host-only; 1 when the launch the arguments describe is taken AND its layer class measured
 *                           faster fused.  It returns 0 for everything the launch refuses: Cout > 128 (or a weight-gradient
 *                           tile that does not own all output channels), Cin or Cout no multiple of 4 (mask: Cin % 32),
 *                           pixel strides below the channel counts or no multiples of 4, x / dy / wt / dx / addends not
 *                           16-byte aligned (mask: 4), a pixel split of dy or x (the whole mask) beyond 2 GiB, any
 *                           precision but SNN_PREC_BF16X3 (bf16 storage, exact fp32, bf16 x 1).  is_mask: x is the bit mask
 *                           and ldx its words per pixel.  dw may be NULL (unchecked).  splitk 0: snn_conv2d_wgrad_splitk's.
 *   snn_conv2d_wgrad_reduce : dw[n] (+)= the splitk slabs of `workspace` in slab order - the reduction every weight
 *                           gradient ends with. */
int snn_conv1x1_bwd_supported(int64_t N, int H, int W, int Cin, int Cout, const void* x, int64_t ldx, int is_mask,
                              const float* dy, int64_t lddy, const float* wt, const float* dx, int64_t lddx,
                              const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2,
                              const float* dw, int splitk, int precision);
int snn_conv1x1_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* wt, float* dx, int64_t lddx,
                    const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2, float* dw, int64_t N,
                    int H, int W, int Cin, int Cout, int accumulate, float* workspace, int splitk, int precision,
                    void* stream);
int snn_conv1x1_mask_bwd(const uint32_t* mask, int64_t ld_mask, const float* dy, int64_t lddy, const float* wt, float* dx,
                         int64_t lddx, const float* addend, int64_t ld_addend, const float* addend2, int64_t ld_addend2,
                         float* dw, int64_t N, int H, int W, int Cin, int Cout, int accumulate, float* workspace, int splitk,
                         int precision, void* stream);
int snn_conv2d_wgrad_reduce(float* workspace, float* dw, int64_t n, int splitk, int accumulate, void* stream);

/* ---------------------------------------------------------------- batch-norm statistics
 * Train-mode nn.BatchNorm2d (layer_gen.py:211-214) applied per TIMESTEP: for every (t,c)
 * the biased mean/var over the M = B*h*w pixels of timestep t (generator.py:190-195 calls the
 * module once per timestep).  `partial` is scratch of snn_bn_stats_partial_size() doubles.
 * snn_bn_stats_finalize also performs the T sequential running-stat updates of one reference
 * forward (momentum 0.1, unbiased variance) when running_mean/var are non-NULL, and emits the
 * per-(t,c) affine  alpha = gamma*invstd, beta = bias - mean*alpha  that the scan consumes.
 * use_running != 0 (eval mode): alpha/beta come from the running statistics for every t.
 * chunks / rows_per_chunk describe the layout of `partial`: 0, 0 for the one snn_bn_stats writes, the two values
 * snn_conv2d_fwd returned in bn_layout for partials that came out of a convolution epilogue. */
size_t snn_bn_stats_partial_size(int T, int64_t M, int C);
int snn_bn_stats(const float* y, int64_t ldy, int T, int64_t M, int C, double* partial, void* stream);
int snn_bn_stats_finalize(const double* partial, int chunks, int rows_per_chunk, int T, int64_t M, int C,
                          const float* gamma, const float* bias, float eps, float momentum,
                          float* running_mean, float* running_var, int use_running,
                          float* mean, float* invstd, float* alpha, float* beta, void* stream);

/* SyncBatchNorm form (config.yaml:76) of the two steps above: reduce the chunk partials to sums[T][C][2]
 * (sum y, sum y^2), let the caller all-reduce that small tensor over the ranks, then finish from the global
 * sums over M_total = world * M pixels.  var_scratch: T*C doubles. */
int snn_bn_stats_reduce(const double* partial, int chunks, int rows_per_chunk, int T, int64_t M, int C, double* sums,
                        void* stream);
int snn_bn_stats_from_sums(const double* sums, int T, int64_t M_total, int C,
                           const float* gamma, const float* bias, float eps, float momentum,
                           float* running_mean, float* running_var,
                           float* mean, float* invstd, float* alpha, float* beta,
                           double* var_scratch, void* stream);

/* ---------------------------------------------------------------- fused affine + neuron scan
 * One kernel = BatchNorm apply + T-step neuron recurrence with the membrane state held in
 * registers.  Replaces, per layer, T x {BatchNorm2d apply, ~12 elementwise norse ops}
 * (layer_gen.py:211-235, norse lif_feed_forward_step / li_feed_forward_step).
 *
 *   x[t]   = y[t]*alpha[t,c] + beta[t,c]                 (alpha/beta NULL -> identity)
 *   LIF    : i' = i + x; vd = v + c_mem*((v_leak - v) + i'); i = i' + c_syn*i';
 *            z = (vd - v_th > 0); v = (1-z)*vd + z*v_reset; out[t] = z
 *   LI     : i' = i + x; v = v + c_mem*((v_leak - v) + i'); i = i' + c_syn*i'; out[t] = v (or tanh(v))
 *   SLI    : as LI with the input gated: i' = i + x*sigmoid(v_st - |v|)
 *   SYNAPSE: p = p + ((x - p)*(x > 0 ? tau_sec : tau_dis))*dt; g = sigma ? 4*sigma*(p - sigma*p^2) : p;
 *            out[t] = max(g, 0); the state is p alone (held in the v slot, i unused)
 *   v0/i0 NULL -> initial state (v = v_leak, i = 0); vT/iT NULL -> final state not written.
 *   vdec (training) receives what the backward scan needs per step: LIF the pre-reset potential vd[t],
 *   SLI the potential BEFORE the step, SYNAPSE the new concentration p[t].
 *   addend (may be NULL; [T][M][C-slice], pixel stride ld_addend): out[t] = neuron output + addend[t] - the residual
 *   shortcut (generator.py:145-146, stack + sum) folded into the store; not allowed with LI_TANH, whose backward
 *   scan reads its own output.
 * Layout: y/out/vdec are [T][M][C-slice] with pixel strides ldy/ldo (vdec dense, ld = C). */
int snn_affine_neuron_fwd(int neuron, const float* y, int64_t ldy,
                          const float* alpha, const float* beta,
                          const float* v0, const float* i0,
                          float* out, int64_t ldo, const float* addend, int64_t ld_addend,
                          float* vT, float* iT, float* vdec,
                          int T, int64_t M, int C, const snn_neuron_params* p, int flags, void* stream);
/* The same call with a spike bit mask as a further output: with SNN_SCAN_SPIKE_MASK | SNN_SCAN_SPIKES_FROM_VDEC in flags it
 * writes vdec, the final state AND mask[T][M][ld_mask] (layout: see the flag); vdec and the state are the bits of the call
 * without the flag.  Without the flag mask must be NULL and the call is snn_affine_neuron_fwd. */
int snn_affine_neuron_fwd_mask(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta,
                               const float* v0, const float* i0, float* out, int64_t ldo, const float* addend,
                               int64_t ld_addend, float* vT, float* iT, float* vdec, int T, int64_t M, int C,
                               const snn_neuron_params* p, int flags, void* stream, uint32_t* mask, int64_t ld_mask);

/* Reverse-time scan (BPTT through the neuron).  LIF: the surrogate dz/du is p->surrogate (default SuperSpike,
 * 1/(alpha|u|+1)^2) and the reset path is differentiated through the spike unless p->reset_detached (default: NOT
 * detached); a non-default rule takes a second instance of the same kernel on the same launch plan, on fp32 tensors (with
 * SNN_SCAN_BF16_STORAGE it is refused), an unknown surrogate code is refused, and so is a non-default rule with a neuron
 * other than LIF.  g_out is dL/d out[t]; g_vT/g_iT (may be NULL = 0) are the
 * gradients of the final state; writes gx = dL/dx[t] (dense [T][M][C]), g_v0/g_i0 (may be NULL)
 * and, when `sums` != NULL, per-block partial sums of gx and gx*y per (t,c) for the BatchNorm
 * backward (`sums` scratch of snn_affine_neuron_bwd_sums_size() doubles, y must be given).
 * `state` is the forward's vdec buffer for LIF / SLI / SYNAPSE, out (tanh output) for LI_TANH, unused otherwise.
 * alpha/beta (may be NULL = identity): the forward's affine, needed to rebuild x[t] for SLI / SYNAPSE.
 * apply_scale != 0: gx is multiplied by alpha[t,c] before it is written (eval-mode BN: dy = alpha*gx).
 * flags: any of SNN_SCAN_WIDE_ADDRESSING, SNN_SCAN_LAST_STEP_ONLY (LIF / LI / LI+Tanh), SNN_SCAN_BF16_STORAGE,
 * SNN_SCAN_SUMS_FROM_STATE [| SNN_SCAN_STATE_LOOKBACK] (see the enum; what a combination does not cover is refused). */
size_t snn_affine_neuron_bwd_sums_size(int T, int64_t M, int C);
/* 1 when snn_affine_neuron_bwd(flags | SNN_SCAN_SUMS_FROM_STATE) covers the call (LIF, the ordered-sums plan of the shape,
 * 32-bit buffer addressing, fp32 tensors, all T gradients, c_mem in [1/64, 1]) */
int snn_affine_neuron_bwd_sums_from_state(int neuron, int T, int64_t M, int C, int64_t ldg, const snn_neuron_params* p,
                                          int flags);
/* host-only: the instance snn_affine_neuron_bwd(neuron, ..., ldg, ..., ldy, ..., sums != NULL iff with_sums, ..., p, flags)
 * launches, into out[10] = { vec (channels per thread), mode (0 no sums, 1 ordered per-wave slabs, 2 LDS atomics), BUF
 * (1: buffer-resource addressing), NP (pixel rows per thread), cvb (channel groups per block), gy (channel blocks), gx
 * (pixel blocks), rpb (pixel rows of P = 256 / cvb pixels per block), 1 if the last pixel row is partial, LDS bytes }.
 * The launch and this query read one plan function.  0, or 1 (with the launch's message) for a call the scan refuses by
 * its shape or flags alone: a bad shape or neuron code, unknown flag bits, a flag the neuron or the channel count does not
 * cover, an SNN_SCAN_SUMS_FROM_STATE request that is not covered.  Pointer alignment is the launch's own check. */
int snn_affine_neuron_bwd_plan(int neuron, int T, int64_t M, int C, int64_t ldg, int64_t ldy, int with_sums,
                               const snn_neuron_params* p, int flags, int64_t* out);
int snn_affine_neuron_bwd(int neuron, const float* g_out, int64_t ldg, const float* state,
                          const float* y, int64_t ldy, const float* g_vT, const float* g_iT,
                          const float* alpha, const float* beta, int apply_scale,
                          float* gx, float* g_v0, float* g_i0, double* sums,
                          int T, int64_t M, int C, const snn_neuron_params* p, int flags, void* stream);

/* LIF with PER-CHANNEL time constants, and their gradients (additions of ABI 20; `neuron` must be SNN_NEURON_LIF - the
 * argument is there so that anything else is refused by name).  The forward step is the one above with the struct's
 * scalars c_mem, c_syn replaced by c_mem[c], c_syn[c] (fp32 [C]; the struct's own two are not read):
 *   i' = i + x; vd = v + c_mem[c]*((v_leak - v) + i'); i = i' + c_syn[c]*i'; z = (vd - v_th > 0); v = (1-z)*vd + z*v_reset
 * and the reverse scan is snn_affine_neuron_bwd's with the same replacement, every gradient rule of the struct included.
 * When tau_partial != NULL it also forms, per pixel block and channel, the partial sums of
 *   dL/dc_mem[c] = sum_{t,m} g_vd[t] (vd[t] - v[t-1]) / c_mem[c]
 *   dL/dc_syn[c] = sum_{t,m} g_i[t] i'[t],   i'[t] = (vd[t] - v[t-1]) / c_mem[c] - (v_leak - v[t-1])
 * (g_i[t]: the gradient arriving at the current after step t; v[t-1] = z[t-1] ? v_reset : vd[t-1], and for t = 0 the
 * forward's initial potential v0, NULL = v_leak) from the saved potentials alone: nothing else is saved or re-read.
 * tau_partial: snn_lif_tau_bwd_partial_size(T, M, C, sums != NULL) doubles.  Fixed summation order (bitwise reproducible)
 * except on the LDS-atomics plan of the shape (mode 2 of snn_affine_neuron_bwd_plan), which adds with LDS float atomics.
 * The scan reads y for the BatchNorm statistic (`sums`): SNN_SCAN_SUMS_FROM_STATE / _STATE_LOOKBACK are refused, and so are
 * SNN_SCAN_BF16_STORAGE, a neuron other than LIF, and SNN_SCAN_LAST_STEP_ONLY together with tau_partial.  A sequence is
 * scanned in one launch (no segment look-back for the two sums).
 *
 * snn_lif_tau_param: the parametrisation c_mem = sigmoid(w_mem), 1 + c_syn = sigmoid(w_syn) (so c_mem in (0, 1), c_syn in
 * (-1, 0)) from n = 1 (per layer) or n = C (per channel) raw values, into c_mem[C], c_syn[C].
 * snn_lif_tau_finalize: the partials in block order, times c_mem (1 - c_mem) and s (1 - s), s = 1 + c_syn; per_layer: summed
 * over the channels in order into ONE value each; stored, or added when accumulate != 0 (as dgamma / dbias).  T, M, C and
 * with_sums are those of the scan that wrote the partials.
 * snn_lif_tau_bwd_plan (host-only): out[12] = the ten values of snn_affine_neuron_bwd_plan for the instance snn_lif_tau_bwd
 * launches, then 1 when the two sums are combined in fixed order (0: LDS float atomics) and the LDS bytes of the launch;
 * returns 1 with the launch's message for what snn_lif_tau_bwd refuses by shape, neuron or flags alone. */
int snn_lif_tau_param(const float* w_mem, const float* w_syn, int n, int C, float* c_mem, float* c_syn, void* stream);
int snn_lif_tau_fwd(int neuron, const float* y, int64_t ldy, const float* alpha, const float* beta,
                    const float* v0, const float* i0, float* out, int64_t ldo,
                    const float* addend, int64_t ld_addend, float* vT, float* iT, float* vdec,
                    int T, int64_t M, int C, const snn_neuron_params* p,
                    const float* c_mem, const float* c_syn, int flags, void* stream);
size_t snn_lif_tau_bwd_partial_size(int T, int64_t M, int C, int with_sums);
int snn_lif_tau_bwd_plan(int neuron, int T, int64_t M, int C, int64_t ldg, int64_t ldy, int with_sums, int with_tau_sums,
                         const snn_neuron_params* p, int flags, int64_t* out);
int snn_lif_tau_bwd(int neuron, const float* g_out, int64_t ldg, const float* state, const float* y, int64_t ldy,
                    const float* g_vT, const float* g_iT, const float* alpha, const float* beta, int apply_scale,
                    float* gx, float* g_v0, float* g_i0, double* sums,
                    int T, int64_t M, int C, const snn_neuron_params* p,
                    const float* c_mem, const float* c_syn, const float* v0, double* tau_partial, int flags, void* stream);
int snn_lif_tau_finalize(const double* tau_partial, int T, int64_t M, int C, int with_sums,
                         const float* c_mem, const float* c_syn, int per_layer,
                         float* d_wmem, float* d_wsyn, int accumulate, void* stream);

/* Memory-saving LIF pair (same results, bit for bit, as the two calls above with neuron = SNN_NEURON_LIF).  Instead
 * of vd[t] for every step, the forward stores the state (v, i) BEFORE every K-th step, K = snn_lif_ckpt_interval():
 *   ckpt[ceil(T/K)][2][M][C]   (2*ceil(T/K)/T of the per-step buffer: half at K = 4)
 * and the backward scan re-runs the K forward steps of a chunk from its checkpoint (it needs y and alpha/beta for
 * that) before walking the chunk in reverse.  An opt-in memory lever for 1280x720-class inputs
 * (functional.LIF_CHECKPOINT_BYTES); speed-neutral.  Default gradient rule only: snn_lif_bwd_ckpt refuses a struct with
 * surrogate != SNN_SURR_SUPER or reset_detached != 0 before it launches anything. */
int snn_lif_ckpt_interval(void);
int snn_lif_fwd_ckpt(const float* y, int64_t ldy, const float* alpha, const float* beta,
                     const float* v0, const float* i0, float* out, int64_t ldo,
                     const float* addend, int64_t ld_addend, float* vT, float* iT, float* ckpt,
                     int T, int64_t M, int C, const snn_neuron_params* p, void* stream);
int snn_lif_bwd_ckpt(const float* g_out, int64_t ldg, const float* ckpt, const float* y, int64_t ldy,
                     const float* g_vT, const float* g_iT, const float* alpha, const float* beta, int apply_scale,
                     float* gx, float* g_v0, float* g_i0, double* sums,
                     int T, int64_t M, int C, const snn_neuron_params* p, void* stream);

/* BatchNorm backward, second phase.  From the partial sums: per-(t,c)
 *   dy = A*gx + Bc*y + Cc,  A = alpha, Bc = -alpha*invstd*s2, Cc = -alpha*s1 + alpha*invstd*mean*s2,
 *   s1 = mean_pix(gx), s2 = mean_pix(gx*xhat);  dgamma[c] = sum_t sum_pix gx*xhat, dbias[c] = sum_t sum_pix gx.
 * dgamma/dbias are accumulated (+=) when accumulate != 0.  `sums` is reduced in place. */
int snn_bn_bwd_finalize(double* sums, int T, int64_t M, int C,
                        const float* gamma, const float* mean, const float* invstd,
                        float* coefA, float* coefB, float* coefC,
                        float* dgamma, float* dbias, int accumulate, void* stream);
/* The same for sums of a scan that ran with SNN_SCAN_SUMS_FROM_STATE: sum(gx*y) = mean*sum(gx) + (sum(gx*x) - bias*sum(gx))
 * / (gamma*invstd) (bias NULL = 0, gamma NULL = 1), then as above.  A channel whose gamma is exactly 0 has no xhat left in x: its sum(gx*y) is formed
 * from gx[T][M][C] and y[T][M][ldy] inside this call (one block per such channel: slow, exact, rare). */
int snn_bn_bwd_finalize_from_state(double* sums, int T, int64_t M, int C,
                                   const float* gamma, const float* bias, const float* mean, const float* invstd,
                                   const float* gx, const float* y, int64_t ldy,
                                   float* coefA, float* coefB, float* coefC,
                                   float* dgamma, float* dbias, int accumulate, void* stream);
/* The same in two steps for SyncBatchNorm: raw[T][C][2] = (sum gx, sum gx*y) of this rank; the caller
 * all-reduces a copy; coefficients come from the global sums over M_total pixels while dgamma / dbias use
 * the rank-local sums (DDP averages them afterwards).  param_sums: T*C*2 doubles of scratch. */
int snn_bn_bwd_reduce(const double* sums, int T, int64_t M, int C, double* raw, void* stream);
/* ... for sums of a scan that ran with SNN_SCAN_SUMS_FROM_STATE: raw receives (sum gx, sum gx*y) all the same (converted
 * with this rank's view of gamma / bias / mean / invstd, which SyncBatchNorm keeps equal on every rank) */
int snn_bn_bwd_reduce_from_state(const double* sums, int T, int64_t M, int C, const float* gamma, const float* bias,
                                 const float* mean, const float* invstd, const float* gx, const float* y, int64_t ldy,
                                 double* raw, void* stream);
int snn_bn_bwd_coef(const double* raw, const double* raw_local, double* param_sums, int T, int64_t M_total, int C,
                    const float* gamma, const float* mean, const float* invstd,
                    float* coefA, float* coefB, float* coefC,
                    float* dgamma, float* dbias, int accumulate, void* stream);
int snn_bn_bwd_apply(const float* gx, const float* y, int64_t ldy,
                     const float* coefA, const float* coefB, const float* coefC,
                     float* dy, int64_t lddy, int T, int64_t M, int C, int accumulate, void* stream);
/* the same two passes on bf16 tensors (bf16-storage mode, see SNN_PREC_BF16S: gx / y / dy are bf16, coefficients and
 * partials as above; C and the strides multiples of 4) */
int snn_bn_bwd_apply_bf16(const float* gx, const float* y, int64_t ldy, const float* coefA, const float* coefB,
                          const float* coefC, float* dy, int64_t lddy, int T, int64_t M, int C, int accumulate, void* stream);
int snn_bn_stats_bf16(const float* y, int64_t ldy, int T, int64_t M, int C, double* partial, void* stream);

/* ---------------------------------------------------------------- merges and pointwise
 * Residual merge = torch.stack(out).sum(0) (generator.py:145-146); Dense merge = torch.cat(out,1)
 * (generator.py:157-158).  A channel-slice copy / add over M pixels covers both and their backward. */
int snn_copy_channels(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream);
int snn_add_channels(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream);
/* dst = a + b over M pixels x C channels, each operand with its own pixel stride */
int snn_add(const float* a, int64_t lda, const float* b, int64_t ldb, float* dst, int64_t ldd,
            int64_t M, int C, void* stream);
/* the same merges on bf16 tensors (bf16-storage mode, see SNN_PREC_BF16S; pointers typed float*, strides in elements; the sum
 * is formed in fp32 and rounded once), and the conversion at the boundary of the bf16 domain (dense, n elements;
 * to_bf16 != 0: fp32 -> bf16 round to nearest even, else bf16 -> fp32) */
int snn_copy_channels_bf16(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream);
int snn_add_bf16(const float* a, int64_t lda, const float* b, int64_t ldb, float* dst, int64_t ldd, int64_t M, int C,
                 void* stream);
int snn_convert_bf16(const void* src, void* dst, int64_t n, int to_bf16, void* stream);
int snn_act_fwd(int act, const float* x, float* y, int64_t n, void* stream);
int snn_act_bwd(int act, const float* x, const float* y, const float* gy, float* gx, int64_t n, void* stream);

/* C (+)= op(A) x op(B), row-major fp32, op = transpose when the flag is set: A is [M][K] ([K][M] transposed), B is [K][N]
 * ([N][K] transposed), C is [M][N]; every element is an fmaf chain in k order.  For weight-sized matrices: two 1x1
 * convolutions with nothing between them (the C2f entry, models/tiny_yolo.py:76-82) are composed into one, and
 * their weight gradients are products of the composed gradient with the other factor.
 * Ct (may be NULL; accumulate must be 0): the transposed result [N][M] from the same launch - the composed weight and
 * the operand of its data gradient. */
int snn_small_gemm(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                  int64_t ldc, int M, int N, int K, int accumulate, float* Ct, int64_t ldct, void* stream);
/* n products C_i = A_i B_i of dense row-major matrices (A_i [M,K], B_i [K,N], C_i [M,N]; Ct_i [N,M] = the transposed copy,
 * base_ct may be NULL) in ONE launch: the composed 1x1 weights w2 w1 of every C2f entry (reference models/tiny_yolo.py:76-82)
 * once per optimiser step.  `table` (device): n rows {A offset, B offset, C offset, Ct offset, M, N, K, ldct} as int64 (ABI
 * v9: 8 columns), offsets in floats relative to the four base pointers; ldct = row length of the transposed copy (0 = M):
 * several products may write column blocks of ONE [N][sum M] matrix - the row-stacked weight of sibling 1x1 convolutions
 * (models/tiny_yolo.py:84-85) and its transpose; max_tiles >= ceil(M/32) * ceil(N/32) of every row.  Same fmaf chains
 * (k order) as snn_small_gemm. */
int snn_small_gemm_batched(const float* base_a, const float* base_b, float* base_c, float* base_ct, const int64_t* table,
                           int n, int max_tiles, void* stream);

/* ConvLSTM cell (conv_lstm.py:51-78), pointwise part after the 1x1 gate convolution.  gates is dense
 * [M][4C] = (input, forget, output, candidate); c_prev NULL = zero state.
 *   c = sigmoid(f)*c_prev + sigmoid(i)*tanh(g);  h = sigmoid(o)*tanh(c) */
int snn_lstm_cell_fwd(const float* gates, const float* c_prev, float* h, float* c, int64_t M, int C, void* stream);
int snn_lstm_cell_bwd(const float* gates, const float* c_prev, const float* c, const float* gh, const float* gc,
                      float* g_gates, float* g_c_prev, int64_t M, int C, void* stream);

/* ConvLSTM with 1x1 gates over a whole sequence (conv_lstm.py:51-78) as a per-pixel temporal scan: a workgroup keeps a
 * tile of pixels for all T steps, the gate product [x_t ; h_{t-1}] . w^T runs on the fp32 MFMA (exact fp32 products, fp32
 * accumulation: no operand split, no range contract), c stays in registers and h in LDS.  Channels-last, time outermost:
 * x [T][M][ldx >= Cin], w [4Ch][Cin + Ch] = conv.weight in OHWI, gate rows (input, forget, output, candidate).
 * No atomics and a fixed summation order: the same inputs give the same bits.
 *
 * snn_convlstm_seq_supported: host-only (no device needed); the launchers check the same function.  Covered:
 * Ch % 16 == 0, 16 <= Ch <= 256, 1 <= Cin <= 256, ldx >= Cin; any T, M >= 1.
 * snn_convlstm_seq_tile: host-only; pixels per workgroup (16 or 32) both kernels use for M pixels, 0 if unsupported.
 *
 * fwd: h0 / c0 [M][Ch], NULL = zeros.  Writes hs [T][M][Ch] and cT [M][Ch]; save_gates [T][M][4Ch] (the gate values AFTER
 * their non-linearity) and save_c [T][M][Ch] (c_t) only when given (both or neither): what the backward reads.
 *
 * bwd, t = T-1 .. 0: dh = gh_t + carried dh; the cell backward on the saved gates gives dgates_t (pre-activation
 * gradients, written to dgates [T][M][4Ch]); d[x ; h] = dgates_t . w: the first Cin columns go to dx_t (pixel stride
 * lddx; dx NULL = not wanted), the last Ch are the carried dh.  gh [T][M][Ch] may be NULL (loss on the final state
 * only); ghT / gcT [M][Ch] (NULL = zero) are the gradients of the returned final state (h_T, c_T), added to the carries
 * before step T-1; c0 as given to the forward.  dh0 / dc0 [M][Ch] receive the carries after step 0 when given.  The
 * weight gradient is NOT formed here: it is one snn_conv2d_wgrad over the T*B frames of [x ; h_prev] with dy = dgates. */
int snn_convlstm_seq_supported(int Cin, int Ch, int64_t ldx);
int snn_convlstm_seq_tile(int Cin, int Ch, int64_t M);
int snn_convlstm_seq_fwd(const float* x, int64_t ldx, const float* w, const float* h0, const float* c0, float* hs,
                         float* cT, float* save_gates, float* save_c, int T, int64_t M, int Cin, int Ch, void* stream);
int snn_convlstm_seq_bwd(const float* w, const float* save_gates, const float* save_c, const float* c0, const float* gh,
                         const float* ghT, const float* gcT, float* dgates, float* dx, int64_t lddx, float* dh0,
                         float* dc0, int T, int64_t M, int Cin, int Ch, void* stream);

/* ---------------------------------------------------------------- depthwise convolution (csrc/conv_depthwise.hip)
 * Conv2d(C, C, K, stride, padding = K / 2, groups = C, bias = False) over channels-last frames [N][H][W][ld >= C]; the
 * output is [N][Ho][Wo], Ho = (H + 2 pad - K) / stride + 1 (Wo alike).  fp32 storage, exact fp32 products, fp32
 * accumulation in kh-major tap order; memory-bound stencils, no MFMA and no arithmetic mode.
 *
 * snn_dwconv_supported: host-only; the ONE statement of what the kernels run - K in {3, 5}, stride in {1, 2},
 * pad = K / 2, C >= 1, N * H * W < 2^31.  Every launcher checks the same function and refuses the rest by name.
 *
 * wt: the TAP-MAJOR weight image [K*K][C], wt[kh*K + kw][c] = weight[c][0][kh][kw] (snn_weight_transpose with I = 1).
 * Any float alignment; every operand may be a channel slice (pixel stride > C) at any channel offset.
 *
 * dgrad: dx [N][H][W][lddx] from dy [N][Ho][Wo][lddy]; every dx element is written exactly once.
 *
 * wgrad: dw [C][K*K] = the parameter's storage order, stored (accumulate 0) or added to (1).  workspace: what
 * snn_dwconv_wgrad_workspace_size returns for the same arguments (fp64 slab rows, 8-byte aligned).  chunks: pixel chunks
 * the sum is split into, 0 = the kernel's own plan (a function of the shape only).  Within a chunk at most 32 products
 * are added in fp32 before the sum continues in fp64; no atomics - the same call gives the same bits. */
int snn_dwconv_supported(int64_t N, int H, int W, int C, int K, int stride, int pad);
int snn_dwconv_fwd(const float* x, int64_t ldx, const float* wt, float* y, int64_t ldy, int64_t N, int H, int W, int C,
                   int K, int stride, int pad, void* stream);
int snn_dwconv_dgrad(const float* dy, int64_t lddy, const float* wt, float* dx, int64_t lddx, int64_t N, int H, int W,
                     int C, int K, int stride, int pad, void* stream);
size_t snn_dwconv_wgrad_workspace_size(int64_t N, int H, int W, int C, int K, int stride, int pad, int chunks);
int snn_dwconv_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dw, int64_t N, int H, int W, int C,
                     int K, int stride, int pad, int accumulate, void* workspace, int chunks, void* stream);

/* Pool("A"/"M"/"S", k, stride) (layer_gen.py:146-173, common.py:18-49), no padding, floor mode.  Both calls refuse
 * k > H, k > W and any Ho, Wo other than (H - k) / stride + 1, (W - k) / stride + 1 before they launch. */
int snn_pool_fwd(int kind, const float* x, float* y, int64_t N, int H, int W, int C,
                 int Ho, int Wo, int k, int stride, void* stream);
int snn_pool_bwd(int kind, const float* x, const float* gy, float* gx, int64_t N, int H, int W, int C,
                 int Ho, int Wo, int k, int stride, void* stream);

/* ---------------------------------------------------------------- pooling with padding, SPP (csrc/pool.hip)
 * Avg / Max / SumPool2d(k, stride, pad), floor mode, over channels-last frames [N][H][W][ld >= C], fp32; the output is
 * [N][Ho][Wo], Ho = (H + 2 pad - k) / stride + 1 (Wo alike).  Every operand may be a channel slice (pixel stride > C) at
 * any channel offset; 16-byte accesses where pointers and strides allow, guarded scalar ones elsewhere, same arithmetic.
 *
 * snn_pool2d_supported: host-only; the ONE statement of what the kernels run - 2 <= k <= 7, 1 <= stride <= k,
 * 0 <= pad <= k / 2, H + 2 pad >= k, W + 2 pad >= k, C >= 1, N * H * W < 2^31.  The launchers refuse the rest by name.
 *
 * fwd: MAX pads with -inf and compares `v > acc || v != v` in window row-major order (ATen: first maximum, a NaN wins).
 * AVG divides by k * k (count_include_pad); in-image taps are added one by one in window row-major order.  At pad = 0
 * all three kinds give the bits of snn_pool_fwd.
 *
 * bwd: a gather - gx = addend (NULL: 0) + the covering windows' terms in ascending (ho, wo), added one by one; every gx
 * element is written exactly once.  MAX routes a window's gradient to its first maximal in-image tap (NaN rule above)
 * and is the only kind that reads x.  addend must not alias gx.  At pad = 0 without addend: the bits of snn_pool_bwd.
 *
 * snn_spp_fwd: y [N][H][W][ldy >= (levels + 1) * C] = x beside `levels` chained MaxPool(k, 1, k / 2) of it (slice j =
 * j pools), in one pass over x; bit-identical to `levels` calls of snn_pool2d_fwd.  snn_spp_supported: k in {3, 5},
 * levels in {1, 2, 3}, C >= 1, N * H * W < 2^31.  The backward is `levels` calls of snn_pool2d_bwd on slices of y. */
int snn_pool2d_supported(int64_t N, int H, int W, int C, int k, int stride, int pad);
int snn_pool2d_fwd(int kind, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t N, int H, int W, int C, int k,
                   int stride, int pad, void* stream);
int snn_pool2d_bwd(int kind, const float* x, int64_t ldx, const float* gy, int64_t ldgy, const float* addend, int64_t ldadd,
                   float* gx, int64_t ldgx, int64_t N, int H, int W, int C, int k, int stride, int pad, void* stream);
int snn_spp_supported(int64_t N, int H, int W, int C, int k, int levels);
int snn_spp_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t N, int H, int W, int C, int k, int levels,
                void* stream);

/* nn.Upsample(scale_factor=s, mode="nearest") (layer_gen.py:176-194) */
int snn_upsample_fwd(const float* x, float* y, int64_t N, int H, int W, int C, int scale, void* stream);
int snn_upsample_bwd(const float* gy, float* gx, int64_t N, int H, int W, int C, int scale, void* stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adamax(lr, betas=(0.9,0.999), eps=1e-8, weight_decay=0) single-tensor step
 * (soda.py:135-136) over a flat parameter / gradient buffer; grad is multiplied by grad_scale first
 * (1/world_size after the data-parallel SUM all-reduce, DDP's gradient averaging). */
int snn_adamax_step(float* param, const float* grad, float* exp_avg, float* exp_inf,
                    int64_t n, float lr, float beta1, float beta2, float eps, int step,
                    float grad_scale, void* stream);

/* Control record of one optimiser step, in DEVICE memory (16 bytes, 4-byte aligned): written by snn_grad_norm, read on
 * the device by every snn_adamax_step_ctl launch of that step - the host never has to look at it to issue the step.
 * The caller zeroes it once; `skipped` then counts for as long as the same record is used. */
typedef struct snn_step_control {
    float   norm;     /* 2-norm of grad*grad_scale over the n elements (pre-clip)            */
    float   scale;    /* extra multiplier: min(1, max_norm / (norm + 1e-6f)), or 1            */
    int32_t finite;   /* 1 if every element is finite                                         */
    int32_t skipped;  /* running count of non-finite steps seen through this record           */
} snn_step_control;

/* 2-norm of a flat gradient and the step's control record (Lightning's gradient_clip_val with
 * gradient_clip_algorithm="norm" = torch.nn.utils.clip_grad_norm_, norm type 2; detect_anomaly's job for the
 * gradient).  Squares and sums are formed in fp64.  Block b sums the 8192 elements [8192 b, 8192 b + 8192) of the
 * buffer counted from the 16-byte boundary at or below `grad`; threads, waves, blocks and block partials are combined
 * in a fixed order without atomics, so the record is bitwise reproducible and the same on every device.  `grad` needs
 * 4-byte alignment only (full groups are read as aligned 16-byte loads, the two ragged ends element by element).
 * Two launches.  Writes  norm = (float)(grad_scale * sqrt(sum g^2)),  scale = min(1, max_norm / (norm + 1e-6f)) in
 * fp32 (exactly 1.0f when max_norm <= 0: norm only),  finite = isfinite(sum g^2),  skipped += !finite.
 * ws: snn_grad_norm_workspace_size(n) bytes, 8-byte aligned (host-only helper, callable without a GPU). */
size_t snn_grad_norm_workspace_size(int64_t n);
int snn_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, void* ws,
                  snn_step_control* ctl, void* stream);

/* snn_adamax_step with, per element and in this order (clip_grad_norm_ / clip_grad_value_ followed by
 * torch.optim.Adamax(weight_decay)):  g = grad*grad_scale;  g *= ctl->scale (ctl given);
 * g = clamp(g, -clip_value, +clip_value) (clip_value > 0);  g += weight_decay * param.
 * With a ctl whose `finite` is 0 the launch stores nothing: parameters and both moments keep their bits.
 * ctl NULL, weight_decay 0 and clip_value <= 0 launch snn_adamax_step's kernel: the same bits. */
int snn_adamax_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_inf,
                        int64_t n, float lr, float beta1, float beta2, float eps, int step,
                        float grad_scale, float weight_decay, float clip_value,
                        const snn_step_control* ctl, void* stream);

/* Weight average (EMA) inside the step.  snn_adamax_step_ema is snn_adamax_step_ctl plus, per element and after the
 * parameter update,  ema = ema + ema_weight * (param_new - ema)  in fp32, unfused.  ema_weight = 1 - decay is formed by
 * the caller (in double, then rounded once): the kernel never subtracts a decay close to 1 from 1 in fp32.  param,
 * exp_avg and exp_inf come out bit for bit as from snn_adamax_step_ctl with the same arguments (also where that call
 * launches snn_adamax_step's kernel).  With a ctl whose `finite` is 0 the launch stores nothing, ema included.
 * Pointer alignment as snn_adamax_step_ctl (4 bytes).  36 bytes moved per element instead of 28.
 * snn_ema_update applies the same update from any `src` under the same ctl rule: parameters that took no Adamax step,
 * BatchNorm buffers.  ema and src must not overlap.
 * Both return non-zero before any launch, with a snn_last_error() that names the argument, for a NULL pointer (ctl may
 * be NULL), n <= 0 or an ema_weight outside (0, 1] (a NaN included). */
int snn_adamax_step_ema(float* param, const float* grad, float* exp_avg, float* exp_inf, float* ema,
                        int64_t n, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                        float weight_decay, float clip_value, float ema_weight,
                        const snn_step_control* ctl, void* stream);
int snn_ema_update(float* ema, const float* src, int64_t n, float ema_weight,
                   const snn_step_control* ctl, void* stream);

/* ---------------------------------------------------------------- event voxelisation
 * utils/datasets.py:378-435: scatter events (t_bin, p, y, x) into binary frames [T][H][W][2]
 * (channels-last image of the reference's [T,2,H,W]); x is clipped to W-1; value 1 (not a count). */
int snn_events_to_frames(const int32_t* t_bin, const int32_t* x, const int32_t* y, const int32_t* p,
                         int64_t n_events, float* frames, int T, int H, int W, void* stream);

/* Augmented event feed: the scatter with the binning of the raw timestamps and a per-sample horizontal flip, zoom,
 * shift and random event drop inside it.  aug is int32 [B][8] in device memory, one row per sample:
 *   {flip (0 | 1), a_q16 (zoom s = a_q16 / 65536; 65536 = identity; callers keep it in [2^14, 2^18]), ox, oy (pixel
 *    shift after the zoom), drop_bits (a uint32 threshold floor(p_drop 2^32); 0 = keep all), seed_bits (uint32), 0, 0}.
 * The events of sample b are offsets[b] .. offsets[b+1] (offsets int64 [B+1], offsets[0] = 0), t0 int64 [B] its window
 * start, frames [T][B][H][W][2] (zero-filled here).  Event e of sample b, j = e - offsets[b]:
 *   1. t_bin = floor((t_us - t0[b]) / step_us) (a true floor); skipped unless 0 <= t_bin < T;
 *   2. skipped unless 0 <= y < H and p in {0, 1}; x clipped into [0, W-1] (the contract of snn_events_to_frames);
 *   3. skipped if fmix32((uint32)j ^ fmix32(seed + 0x9E3779B9 * (uint32)(j >> 32))) < drop (fmix32: the murmur3
 *      finaliser) - a function of the event's index inside its sample, not of what else the batch holds;
 *   4. flip: x = W - 1 - x;   5. x' = (((2x + 1) a_q16) >> 17) + ox = floor((x + 0.5) s) + ox, y' likewise with oy;
 *   6. skipped unless (x', y') is inside the frame (dropped, not clipped: for ANY table contents nothing is written
 *      outside the buffer);   7. frames[t_bin][b][y'][x'][p] = 1.
 * Zooming in does not interpolate: a factor above 1 leaves the gaps sparse events leave.  n_events = 0 and empty
 * samples are fine.  Refused: null pointers, step_us <= 0, a frame buffer of 2^31 elements or more. */
int snn_events_to_frames_aug(const int64_t* t_us, const int32_t* x, const int32_t* y, const int32_t* p,
                             const int64_t* offsets, const int64_t* t0, const int32_t* aug, int64_t n_events,
                             float* frames, int T, int B, int H, int W, int64_t step_us, void* stream);

/* The same feed from the 8-byte records of a Prophesee DAT recording, unpacked in the kernel: words is uint32 [n][2] in
 * device memory, 8-byte aligned (sample slices may start at any event), event e = {ts_us, data}:
 *   t_us = words[2e] zero-extended to 64 bits;  d = words[2e+1]:  x = d & 0x3FFF, y = (d >> 14) & 0x3FFF,
 *   p = (d >> 28) & 1; bits 29-31 are ignored.
 * Everything else - offsets, t0, the table, binning, x clipped to [0, W-1], y >= H dropped, the drop hash on the index
 * inside the sample, flip, zoom, shift, the frame test, zero-fill, the refusals - is snn_events_to_frames_aug's.  aug NULL
 * is the identity and reads no table.  For ANY word contents and ANY table contents nothing is written outside frames.
 * n_events = 0 zero-fills and launches nothing.  Timestamps do not wrap inside a recording (2^32 us = 71 minutes). */
int snn_events_to_frames_packed(const uint32_t* words, const int64_t* offsets, const int64_t* t0, const int32_t* aug,
                                int64_t n_events, float* frames, int T, int B, int H, int W, int64_t step_us,
                                void* stream);

/* Event representations: the same two feeds with another rule 7.  Rules 1-6 of snn_events_to_frames_aug pick the event
 * and its cell exactly as above; frames stays [T][B][H][W][2] fp32, polarity the channel.  A cell holds a uint32
 * accumulator from zero (the zero fill: zero bits are +0.0f), updated with integer atomics - add and max are order
 * independent, so the result is bit-identical from run to run and under any permutation of a sample's events - and one
 * in-place finalize pass turns accumulators into values, every operation a single fp32 round-to-nearest (fl):
 *   SNN_EVREP_BINARY  the idempotent 1.0f store of the entries above, bit for bit; clip = 0 and scale = 1 only, no
 *                     finalize pass.
 *   SNN_EVREP_COUNT   n += 1 per event;  v = fl(fl(min(n, clip)) scale);  0 <= clip <= 2^24, clip = 0: no clip.
 *   SNN_EVREP_TIME    m = max over the events of r + 1, r = d - t_bin step_us the offset inside the bin (d = t_us -
 *                     t0[b], 0 <= r < step_us): the latest event of the bin;  v = fl(fl(fl(m) / fl(step_us)) scale), in
 *                     (0, 1] scale;  clip must be 0, step_us <= 2^32 - 1.
 *   SNN_EVREP_VOXEL   bilinear in time around the bin centres, in Q16.  Rule 1 keeps its window test (0 <= d < T
 *                     step_us) and its bin is replaced:  u = 2d - step_us,  k = floor(u / (2 step_us)) in -1 .. T-1,
 *                     rem = u - 2 k step_us,  q = floor(rem 2^16 / (2 step_us)) in 64-bit integers;  the event adds
 *                     65536 - q to bin k if k >= 0 and q to bin k + 1 if k + 1 <= T - 1 and q > 0 (weight that falls
 *                     outside the window is lost);  v = fl(fl(fl(min(acc, clip 65536)) 2^-16) scale);  0 <= clip <=
 *                     65535 (0: no clip), step_us < 2^40.  A cell that collects more than 2^16 - 1 events' weight in
 *                     one bin wraps modulo 2^32: outside the contract, and still nothing is written outside frames.
 * Empty cells stay +0.0f.  scale must be finite and > 0.  The finalize pass asks frames 4-byte alignment only (16-byte
 * accesses between a scalar head and tail).  n_events = 0 zero-fills and launches nothing.
 * snn_events_rep_supported (host only) answers 1 / 0 for (rep, step_us, clip) by the ranges above (step_us > 0).
 * snn_events_to_frames_aug_rep is snn_events_to_frames_aug, snn_events_to_frames_packed_rep
 * snn_events_to_frames_packed - arguments, checks and refusals under their own names - except that aug may be NULL for
 * both (the identity, no table read).  On top they refuse, naming the argument: an unknown rep, a clip out of range for
 * the rep, a scale that is not finite or <= 0 (or not 1 for binary), a step_us too large for time / voxel, and for the
 * non-binary representations n_events >= 2^32. */
#define SNN_EVREP_BINARY 0
#define SNN_EVREP_COUNT 1
#define SNN_EVREP_TIME 2
#define SNN_EVREP_VOXEL 3
int snn_events_rep_supported(int rep, int64_t step_us, int clip);
int snn_events_to_frames_aug_rep(const int64_t* t_us, const int32_t* x, const int32_t* y, const int32_t* p,
                                 const int64_t* offsets, const int64_t* t0, const int32_t* aug, int64_t n_events,
                                 float* frames, int T, int B, int H, int W, int64_t step_us, int rep, int clip,
                                 float scale, void* stream);
int snn_events_to_frames_packed_rep(const uint32_t* words, const int64_t* offsets, const int64_t* t0, const int32_t* aug,
                                    int64_t n_events, float* frames, int T, int B, int H, int W, int64_t step_us,
                                    int rep, int clip, float scale, void* stream);

/* The boxes of the same transform.  labels_in / labels_out: fp32 [B][N][width], width 5 (class, x1, y1, x2, y2) or 6
 * (ts in front, copied untouched), boxes normalised to [0, 1]; a row whose class is below 0 is padding and stays
 * padding.  A valid row, s = a_q16 2^-16:  flip (x1, x2) = (1 - x2, 1 - x1);  x' = x s + ox / W, y' = y s + oy / H;
 * A0 = area of that box, A1 = area of it clipped to [0, 1]; the row is kept, with the CLIPPED box, when
 * A1 >= min_visible A0 and the clipped extents are at least min_size_px pixels wide and high; otherwise it becomes all
 * -1.  Kept rows are written to the front of their sample in their order, the -1 rows behind them (the layout a collate
 * that pads at the end produces); N never changes.  One block per sample.  labels_out must not be labels_in. */
int snn_labels_augment(const float* labels_in, float* labels_out, const int32_t* aug, int B, int N, int width, int W,
                       int H, float min_visible, float min_size_px, void* stream);

/* ---------------------------------------------------------------- carried state
 * Training on consecutive windows of a recording carries the detector state (fp32 tensors [B, ...], the sample
 * outermost, each sample's block dense) from one step to the next.  snn_state_reset puts the samples that start a new
 * recording back to rest in all n tensors with ONE launch: table (device, int64) has n rows {address of the tensor,
 * elements per sample, rest value as fp32 bits in the low 32 bits}; sample b of tensor l is the `elements` floats at
 * address + 4 * b * elements.  first[B] (device, int32): != 0 fills the sample's block of every tensor with the row's
 * rest value, 0 leaves every byte of it alone - a block of the grid (16 chunks x B x n) then returns after reading
 * first[b], so the usual step costs one near-empty launch and the host never reads first.  Addresses need 4-byte
 * alignment only (16-byte stores between scalar head and tail); n, B <= 65535. */
int snn_state_reset(const int64_t* table, int n, int B, const int32_t* first, void* stream);

/* ---------------------------------------------------------------- detection decode
 * Tail of SODa.predict (models/soda.py:202-233): per anchor conf = max_k prob[k], class = argmax - 1 (background -1),
 * box = offset_inverse(anchor, offsets) (utils/box.py:72-79, 102-119).  prob [A][K], offsets / anchors / boxes [A][4].
 * Contract of the probabilities: every entry lies in [0, 1] or is NaN.  The argmax starts from column 0 and moves on
 * prob[k] > best only, so the first maximum wins, a NaN never replaces a finite best and a NaN in column 0 stays: a row
 * whose column 0 is NaN (an all-NaN row among them) decodes to class -1 with confidence NaN whatever its other columns
 * hold, and a NaN in a later column is passed over (torch.max of the host path would return that NaN and its column:
 * the one place where the two paths differ).  A class -1 row is never an NMS candidate; snn_detect_assemble writes it
 * as a not-kept row in anchor order with class -1, its confidence as it is (NaN < pos_threshold is false) and its
 * decoded box.  The caller's ordering between decode and NMS (box.py: detection_order) must keep such a row inside the
 * background band for seg to count it there; rows of one class and equal confidence are ordered by anchor, ascending,
 * so of identical boxes with equal confidence the lowest anchor is kept.
 * snn_detect_decode[_batched] read and write scalars: no pointer needs more than its type's 4-byte alignment (boxes
 * included, unlike in the NMS and assemble entry points below), and K has no upper bound (K > 1, A > 0; batched:
 * N * A < 2^31 - 256). */
int snn_detect_decode(const float* cls_prob, const float* offsets, const float* anchors, int A, int K,
                      float* conf, int* cls, float* boxes, void* stream);
/* Per-class greedy NMS (utils/box.py:82-99).  order[A]: anchor ids sorted by (class ascending, confidence descending);
 * seg[num_classes + 1]: members of class c are order[seg[c] .. seg[c+1]).  kept[seg[c] ..) receives the kept ids of
 * class c in keep order, nkept[c] their number; kept_flag[id] = 1 and kept_rank[id] = rank inside its class for kept
 * anchors (both arrays must be zeroed by the caller).  One block per class; a candidate survives
 * only while IoU <= iou_threshold against every kept box (so a NaN IoU suppresses, as utils/box.py:95-97 does). */
int snn_nms_sorted(const float* boxes, const int* order, const int* seg, int num_classes, float iou_threshold,
                   int* kept, int* nkept, unsigned char* kept_flag, int* kept_rank, void* stream);
/* The same for N frames at once (every timestep of a clip, every sample of a validation batch), rows = N * A.
 * snn_detect_decode_batched: prob [N][A][K], offsets [N][A][4], anchors [A][4] (the anchor of a row is row % A);
 *   conf / cls [N][A], boxes [N][A][4].
 * snn_nms_sorted_batched: one block per (class, frame).  order[N][A]: ROW ids (n * A + anchor) sorted by (frame, class
 *   ascending, confidence descending, anchor ascending); seg[N][num_classes + 1] counts inside the frame: the members of
 *   frame n's class c are order[n * A + seg[n][c] .. n * A + seg[n][c + 1]).  kept[N][A] (row ids, frame n's class c from
 *   n * A + seg[n][c]), nkept[N][num_classes], kept_flag / kept_rank [N][A] as above, zeroed by the caller.
 * snn_detect_assemble: the output rows (utils/box.py:121-153), one block per frame: out[N][A][6] rows (class, conf, x1,
 *   y1, x2, y2); kept rows first at class_off[class] + rank (class_off = exclusive sum of nkept[n]), the others behind
 *   them in anchor order; conf < pos_threshold gives class -1 and confidence 1 - conf, a row that was not kept class -1.
 *   num_classes <= 1024.  boxes 16-byte, out 8-byte aligned; N * A < 2^31 - 256 in all three. */
int snn_detect_decode_batched(const float* cls_prob, const float* offsets, const float* anchors, int N, int A, int K,
                              float* conf, int* cls, float* boxes, void* stream);
int snn_nms_sorted_batched(const float* boxes, const int* order, const int* seg, int N, int A, int num_classes,
                           float iou_threshold, int* kept, int* nkept, unsigned char* kept_flag, int* kept_rank,
                           void* stream);
int snn_detect_assemble(const float* conf, const int* cls, const float* boxes, const int* nkept,
                        const unsigned char* kept_flag, const int* kept_rank, int N, int A, int num_classes,
                        float pos_threshold, float* out, void* stream);

/* ---------------------------------------------------------------- training targets and loss
 * snn_roi_assign: RoI.__call__ (utils/roi.py:18-109) for a whole batch, one block per sample.  anchors [A][4] corner
 * boxes, labels [B][N][5] rows (class, x1, y1, x2, y2) with -1 padding rows (which, as upstream, still claim an anchor
 * in the greedy phase).  An anchor takes the ground truth of highest IoU when that IoU >= iou_threshold, then every
 * label row claims the globally best remaining anchor (first maximum on ties).  Outputs: bbox_offset [B][A][4] =
 * offset_boxes(anchor, assigned box) * mask (utils/box.py:62-69), bbox_mask [B][A][4] (0 / 1), class_labels [B][A]
 * int64 (0 = background, label + 1 otherwise).  workspace: snn_roi_workspace_size(B, A, N) bytes.
 * The claimed anchor of a round is trunc((float)flat / (float)N) of the flat argmax index, as upstream forms it
 * (utils/roi.py:105).  With A * N > 2^24 the fp32 quotient differs from flat / N for some indices; those assignments are
 * upstream's and are reproduced.  For an index in the last anchor's row it can round up to A, where upstream raises
 * IndexError; the kernel then takes anchor A - 1 and writes nothing outside the sample's rows.  A * N must stay below
 * 2^31 - 1024 (refused otherwise). */
size_t snn_roi_workspace_size(int B, int A, int N);
int snn_roi_assign(const float* anchors, const float* labels, int B, int A, int N, float iou_threshold,
                   void* workspace, float* bbox_offset, float* bbox_mask, int64_t* class_labels, void* stream);
/* SODa._loss (models/soda.py:259-281) over rows = B*A anchors with K = classes + 1 logits each:
 *   loss = loss_ratio * mean(CE[label > 0]) + (1 - loss_ratio) * mean(CE[label == 0]) + mean |bbox*mask - offset*mask|
 * fwd writes the scalar loss and stats[5] = {sum CE pos, #pos, sum CE neg, #neg, sum L1} (fp64, kept for bwd);
 * bwd writes d loss / d logits [rows][K] and d loss / d bbox [rows][4], scaled by the device scalar *g_loss.
 * The kernels are those of snn_det_loss_ext_* below with SNN_LOSS_CLS_CE, SNN_LOSS_BOX_L1, box_weight 1, A = 1 and no
 * steps, except that the two means divide by #pos / #neg as they are: an empty class gives NaN, as the reference's
 * ce[pos].mean().  workspace: snn_det_loss_workspace_size(rows) bytes (= snn_det_loss_ext_workspace_size(rows)). */
size_t snn_det_loss_workspace_size(int64_t rows);
int snn_det_loss_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset, const float* bbox_mask,
                     const int64_t* class_labels, int64_t rows, int K, float loss_ratio, void* workspace, double* stats,
                     float* loss, void* stream);
int snn_det_loss_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset, const float* bbox_mask,
                     const int64_t* class_labels, int64_t rows, int K, float loss_ratio, const double* stats,
                     const float* g_loss, float* g_logits, float* g_bbox, void* stream);

/* ---- Every labelled timestep of a sequence (multi-target labels; new symbols under ABI v20).  labels [B][N][6] rows
 * (ts, class, x1, y1, x2, y2): ts the integer-valued timestep of the uncut sequence, -1 in every column = padding row.
 * The training step drops a prefix of t0 frames; a row belongs to step ts - t0 of the cut sequence of T steps and is
 * ignored outside [0, T).  K (1 .. 32, <= T) is the number of frame slots per sample.  Nothing here synchronises with
 * the host or allocates.
 * snn_label_steps: one block per sample.  steps [K][B] int32: the latest K distinct steps of the sample's real rows
 * (class >= 0) in ascending order from slot 0, -1 in the unused slots. */
int snn_label_steps(const float* labels, int B, int N, int T, int K, int t0, int* steps, void* stream);
/* Channels-last frames [T][B][M pixels][C] with pixel strides ld >= C on both sides (float4 when C, both strides and the
 * pointers allow, scalar otherwise).  fwd: dst[k][b] = src[steps[k][b]][b], zeros for an empty slot (a step outside
 * [0, T)).  bwd: writes the C channels of EVERY frame of g_src [T][B] in one pass - the gradient of the slot that
 * selected the frame (the sum in slot order when several slots of a sample name one step), exact zeros elsewhere; no
 * memset, no atomics. */
int snn_gather_steps_fwd(const float* src, int64_t ld_src, const int* steps, float* dst, int64_t ld_dst, int T, int B,
                         int K, int64_t M, int C, void* stream);
int snn_gather_steps_bwd(const float* g_dst, int64_t ld_dst, const int* steps, float* g_src, int64_t ld_src, int T, int B,
                         int K, int64_t M, int C, void* stream);
/* snn_roi_assign_steps: one block per slot (k, b).  The slot's assignment is snn_roi_assign's for one sample whose label
 * tensor [n][5] holds, in their order, the real rows of sample b with ts - t0 == steps[k][b] and its padding rows
 * (which, as there, claim an anchor in the greedy phase; the fp32 quotient of the claimed anchor uses n).  Rows of other
 * timesteps take no part.  An empty slot gets zero targets.  Outputs bbox_offset [K][B][A][4], bbox_mask [K][B][A][4],
 * class_labels [K][B][A] int64.  steps is trusted as snn_label_steps writes it (the call carries no T to check it
 * against): a step >= 0 that no real row of the sample lies on, in a sample without padding rows, leaves n = 0 rows -
 * the slot then gets zero targets as an empty one does (nothing is read or written out of bounds), but being >= 0 it
 * still counts as valid in snn_det_loss_steps_*.  workspace: snn_roi_steps_workspace_size(K, B, A, N) bytes, 16-byte
 * aligned as the anchors and the box outputs; A * N below 2^31 - 1024. */
size_t snn_roi_steps_workspace_size(int K, int B, int A, int N);
int snn_roi_assign_steps(const float* anchors, const float* labels, const int* steps, int K, int B, int A, int N,
                         int t0, float iou_threshold, void* workspace, float* bbox_offset, float* bbox_mask,
                         int64_t* class_labels, void* stream);
/* ---- Task-aligned anchor assignment (DESIGN section 5 "Anchor assignment"; new symbols under ABI v20): the positives
 * are chosen from the predictions, which are read as constants.  One entry for both label forms:
 *   steps == NULL: labels [B][N][5] rows (class, x1, y1, x2, y2), predictions [B][A][C] / [B][A][4], S = B slots, K = 1;
 *   otherwise:     labels [B][N][6] rows (ts, class, x1, y1, x2, y2), steps [K][B] as snn_label_steps writes them,
 *                  predictions [K][B][A][C] / [K][B][A][4], S = K * B slots, K in 1 .. 32.
 * C = classes + 1 logits per anchor, column 0 the background.  A row takes part when 0 <= class, class + 1 < C,
 * x2 > x1, y2 > y1 and, with steps, ts - t0 == steps[k][b]; padding rows and rows of a class the logits have no column
 * for take no part (the class is never used as an index).  Per slot:
 *   p_a    = offset_inverse(anchor_a, bbox_preds_a), the exponent argument o / 5 replaced by log(1000 / 16) where it
 *            is not <= that (NaN included), as decode_box of det_loss.hip;
 *   s[a,j] = softmax(cls_logits_a)[class_j + 1], u[a,j] = I / (U + 1e-7) of p_a and box j; what is not > 0 counts as 0;
 *   anchor a is a candidate of row j when its centre lies strictly inside box j; t[a,j] = s^alpha * u^beta (0 when not
 *   > 0); every row selects up to topk candidates in (t descending, anchor ascending) order, t = 0 included;
 *   an anchor selected by several rows goes to the row of largest u[a,j] (the lower row on ties); then, in row order,
 *   a row left without an anchor claims the still unassigned anchor of highest box_iou(anchor, box) (first maximum).
 * Outputs as snn_roi_assign / snn_roi_assign_steps write them: bbox_offset [S][A][4] = offset_boxes(anchor, assigned
 * box) * mask, bbox_mask [S][A][4], class_labels [S][A] int64 (class + 1, 0 = background); assigned_row [S][A] int32
 * (may be NULL): the label-row index, -1 for background.  An empty slot (steps < 0) and a slot without a row that takes
 * part get exact zeros (assigned_row -1).  Three launches, no host synchronisation, no allocation, no atomics.
 * workspace: snn_tal_workspace_size(S, A, N, topk) bytes.  Refused before any launch: null pointers (steps and
 * assigned_row may be NULL), topk outside 1 .. 64, C outside 2 .. 64, alpha or beta negative or not finite, A * N at or
 * above 2^31 - 1024, anchors / bbox_preds / bbox_offset / bbox_mask / workspace not 16-byte aligned. */
size_t snn_tal_workspace_size(int S, int A, int N, int topk);
int snn_tal_assign(const float* anchors, const float* labels, const int* steps, const float* cls_logits,
                   const float* bbox_preds, int K, int B, int A, int N, int C, int t0, int topk, float alpha, float beta,
                   void* workspace, float* bbox_offset, float* bbox_mask, int64_t* class_labels, int* assigned_row,
                   void* stream);
/* The loss above over the anchors of the V valid slots (steps[k][b] >= 0) of predictions [K][B][A][C] / [K][B][A][4]:
 *   loss = loss_ratio * mean(CE[pos]) + (1 - loss_ratio) * mean(CE[neg]) + sum |bbox*mask - offset*mask| / (4 A V)
 * stats[6] = the five sums of snn_det_loss_fwd and V, counted on the device.  V = 0: loss 0 and zero gradients; V > 0
 * without positives (or negatives): NaN, as snn_det_loss_fwd.  bwd writes all K*B*A rows, exact zeros for empty slots.
 * The kernels of snn_det_loss_ext_* with the same fixed modes, this A and steps, and the same means as they are.
 * workspace: snn_det_loss_steps_workspace_size(K, B, A) bytes (= snn_det_loss_ext_workspace_size(K * B * A)). */
size_t snn_det_loss_steps_workspace_size(int K, int B, int A);
int snn_det_loss_steps_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                           const float* bbox_mask, const int64_t* class_labels, const int* steps, int K, int B, int A,
                           int C, float loss_ratio, void* workspace, double* stats, float* loss, void* stream);
int snn_det_loss_steps_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                           const float* bbox_mask, const int64_t* class_labels, const int* steps, int K, int B, int A,
                           int C, float loss_ratio, const double* stats, const float* g_loss, float* g_logits,
                           float* g_bbox, void* stream);

/* ---- Selectable detection loss (new symbols under ABI v20; one kernel family serves these and snn_det_loss_* above,
 * whose signatures and conventions are unchanged).  The same rows, with
 * anchors [A][4] corner boxes (row r uses anchor r % A; rows is a multiple of A) and steps [rows / A] int32 or NULL:
 * with steps, the rows of a frame with steps[frame] < 0 are left out of every sum and get exact zeros as gradients, and
 * V counts the other frames on the device; without, V = rows / A.
 *   cls  = loss_ratio * sum_pos f / max(n_pos, 1) + (1 - loss_ratio) * sum_neg f / max(n_neg, 1)
 *          f = ce = -log softmax(x)[y] (SNN_LOSS_CLS_CE) or (1 - p_y)^gamma * ce (SNN_LOSS_CLS_FOCAL); pos: label > 0
 *   box  = box_weight * sum |bbox*mask - offset*mask| / (4 A V)                              (SNN_LOSS_BOX_L1)
 *        = box_weight * sum over box rows of (1 - IoU + penalty) / max(n_pos, 1)             (GIOU, DIOU, CIOU)
 *   loss = cls + box; without any positive row the means over them are 0 (not NaN); V = 0: loss 0, zero gradients.
 * Box rows have label > 0 and all four mask entries equal to 1.  Their boxes are offset_inverse (utils/box.py:72-79) of
 * the anchor with bbox_preds and with bbox_offset, the exponent argument o / 5 clamped above at log(1000 / 16) (zero
 * gradient past the clamp).  IoU = I / (U + eps); GIoU penalty (C - U) / (C + eps) of the enclosing box's area C;
 * DIoU rho^2 / (c^2 + eps), squared centre distance over squared enclosing diagonal; CIoU adds alpha * v with
 * v = 4 / pi^2 (atan(wg / (hg + eps)) - atan(w / (h + eps)))^2 and alpha = v / (1 - IoU + v + eps) held constant in the
 * gradient; eps = 1e-7.  Rows that are no box rows get exact zeros in g_bbox under the IoU modes.
 * stats[9] = {sum f pos, n_pos, sum f neg, n_neg, box sum, V, pos term, neg term, box term}: the last three are the fp32
 * terms of the loss, loss = (pos term + neg term) + box term.  Refused before any launch: null pointers (steps may be
 * NULL), K outside 1 .. 64, rows not a positive multiple of A, unknown modes, gamma < 0, bbox_preds / bbox_offset /
 * bbox_mask / anchors / g_bbox not 16-byte aligned.  workspace: snn_det_loss_ext_workspace_size(rows) bytes. */
enum { SNN_LOSS_CLS_CE = 0, SNN_LOSS_CLS_FOCAL = 1 };
enum { SNN_LOSS_BOX_L1 = 0, SNN_LOSS_BOX_GIOU = 1, SNN_LOSS_BOX_DIOU = 2, SNN_LOSS_BOX_CIOU = 3 };
size_t snn_det_loss_ext_workspace_size(int64_t rows);
int snn_det_loss_ext_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                         const float* bbox_mask, const int64_t* class_labels, const float* anchors, const int* steps,
                         int64_t rows, int A, int K, float loss_ratio, int cls_mode, float gamma, int box_mode,
                         float box_weight, void* workspace, double* stats, float* loss, void* stream);
int snn_det_loss_ext_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                         const float* bbox_mask, const int64_t* class_labels, const float* anchors, const int* steps,
                         int64_t rows, int A, int K, float loss_ratio, int cls_mode, float gamma, int box_mode,
                         float box_weight, const double* stats, const float* g_loss, float* g_logits, float* g_bbox,
                         void* stream);

/* ---------------------------------------------------------------- detection mAP (ABI v12)
 * COCO bounding-box mAP as the reference computes it in validation_step / test_step (models/soda.py:160-182, 283-321:
 * torchmetrics MeanAveragePrecision, iou_type "bbox", area range "all", no crowd boxes).
 * snn_map_match: one block per (image, class).  dets [B][A][6] rows (class, score, x1, y1, x2, y2), labels [B][G][5] rows
 * (class, x1, y1, x2, y2), class < 0 = padding; order [B][A] int32 row ids sorted by (class ascending, score descending),
 * stably; seg [B][num_classes + 1] int32: the rows of class c are order[b][seg[b][c] .. seg[b][c+1]).  The first `slots`
 * of them (= the largest maxDet, <= 1024) are matched greedily at each of the num_iou (<= 31) thresholds (device fp64
 * table) against the image's ground truth of the class (G <= 2048 rows per image).  Records [B][num_classes][slots]:
 * score (-inf for an empty slot) and match_mask (bit 31: slot used, bit t: matched at threshold t); npig[c] += the
 * image's ground-truth count of class c (one integer atomic per block, zeroed by the caller once per evaluation).
 * snn_map_accumulate: order [num_classes][records] int32: positions (image * slots + slot) of each class's records
 * sorted by score descending, stably; match_mask [num_classes][records] in position order; max_dets [num_max_dets] int32
 * ascending (device), rec_thresholds [num_rec] fp64 ascending (device, <= 1024); t50 / t75: index of IoU 0.5 / 0.75 in
 * the threshold table or -1.  out[3 + num_max_dets] fp32 = map, map_50, map_75, mar at each max_dets entry; -1 where no
 * class has ground truth.  workspace: snn_map_workspace_size(num_classes, num_max_dets, num_iou) bytes. */
int snn_map_match(const float* dets, const float* labels, const int* order, const int* seg, int B, int A, int G,
                  int num_classes, int slots, const double* iou_thresholds, int num_iou, float* score,
                  unsigned* match_mask, int* npig, void* stream);
size_t snn_map_workspace_size(int num_classes, int num_max_dets, int num_iou);
int snn_map_accumulate(const int* order, const unsigned* match_mask, const int* npig, int num_classes, int records,
                       int slots, const int* max_dets, int num_max_dets, const double* rec_thresholds, int num_rec,
                       int num_iou, int t50, int t75, void* workspace, float* out, void* stream);

/* ---------------------------------------------------------------- mAP area ranges, per-class AP, size filter (ABI v20,
 * symbols added).  COCOeval's area ranges on pixel sizes: a row's pixel width is (double)fl32(x2 - x1) * img_w, its
 * height (double)fl32(y2 - y1) * img_h, its area their fp64 product; small [0, 32^2], medium [32^2, 96^2], large
 * [96^2, 1e10], both ends inclusive.  Per range a ground-truth row outside it is ignored; a detection takes the free
 * non-ignored row of largest IoU >= the threshold (ties to the later row) and only when none qualifies the free ignored
 * row chosen by the same rule; a detection matched to an ignored row, or unmatched with its own area outside the range,
 * is ignored: neither true nor false positive, though it keeps its slot among the first maxDet.  The "all" outputs of
 * these entry points carry the bits of the three above.  Every refusal names its entry point and launches nothing.
 * snn_map_filter_rows: one thread per row.  det_key [B][A] int32: the class id, num_classes for an id out of range,
 * num_classes + 1 for padding; label_cls [B][G]: the labels' class column.  A row (either kind) with
 * wp^2 + hp^2 < min_box_diag^2, wp < min_box_side or hp < min_box_side (pixels; each test active only when its limit
 * is > 0) becomes padding (key num_classes + 1, class -1).  *bad (device int64) += rows left with an id >= num_classes.
 * snn_map_match_areas: snn_map_match with the labels' class column read from label_cls and, with num_ranges == 3 (0: the
 * "all" pass alone, the area pointers may be null), per slot and range area_matched / area_ignored
 * [B][num_classes][3][slots] (bit t: at threshold t) and npig_area [3][num_classes] += the non-ignored rows.
 * snn_map_accumulate_areas: snn_map_accumulate over masks laid out [num_classes][3][records] beside match_mask;
 * out[3 + num_max_dets + 2 * num_ranges]: the values of snn_map_accumulate, then (map, mar) at the largest maxDet for
 * small, medium, large; out_class (may be null) [2][num_classes]: each class's AP and AR at the largest maxDet for
 * "all", -1 without ground truth.  workspace: snn_map_areas_workspace_size bytes. */
int snn_map_filter_rows(const float* dets, const float* labels, int B, int A, int G, int num_classes, double img_h,
                        double img_w, double min_box_diag, double min_box_side, int* det_key, float* label_cls,
                        int64_t* bad, void* stream);
int snn_map_match_areas(const float* dets, const float* labels, const float* label_cls, const int* order, const int* seg,
                        int B, int A, int G, int num_classes, int slots, const double* iou_thresholds, int num_iou,
                        double img_h, double img_w, int num_ranges, float* score, unsigned* match_mask,
                        unsigned* area_matched, unsigned* area_ignored, int* npig, int* npig_area, void* stream);
size_t snn_map_areas_workspace_size(int num_classes, int num_max_dets, int num_iou, int num_ranges);
int snn_map_accumulate_areas(const int* order, const unsigned* match_mask, const unsigned* area_matched,
                             const unsigned* area_ignored, const int* npig, const int* npig_area, int num_classes,
                             int records, int slots, const int* max_dets, int num_max_dets, const double* rec_thresholds,
                             int num_rec, int num_iou, int t50, int t75, int num_ranges, void* workspace, float* out,
                             float* out_class, void* stream);

/* ---------------------------------------------------------------- activity counts (ABI v20, symbols added)
 * Per-channel counts of the elements of a channels-last tensor src[T][M][ld] that satisfy a predicate: the spikes of a
 * LIF layer from whatever its forward scan left (spike tensor, saved potentials, bit mask) and the non-zero operands of
 * a convolution.  Counts are exact integers: per-lane 32-bit counters, one 64-bit integer atomic add per (block,
 * timestep, channel); nothing is accumulated in floating point. */
enum { SNN_ACT_NONZERO_F32 = 0, SNN_ACT_NONZERO_BF16 = 1,   /* x != 0 (-0.0 is zero; NaN and denormals are non-zero) */
       SNN_ACT_ABOVE_F32 = 2,   SNN_ACT_ABOVE_BF16 = 3,     /* x > threshold, strict - the comparison of the scans and of
                                                               the snn_conv*_spikes_* consumers; NaN is not above */
       SNN_ACT_MASK = 4 };                                  /* uint32 words, layout of SNN_SCAN_SPIKE_MASK; C % 32 == 0 */
/* ld: pixel stride of src in elements (SNN_ACT_MASK: in words), ld >= C (mask: >= C / 32); any C >= 1, any ld and any
 * pointer alignment are taken: 4 channels per access where C % 4 == 0, ld % 4 == 0 and src is 16-byte (bf16: 8-byte)
 * aligned, one channel per access otherwise; the mask is read one word per lane.  Channels >= C of a row - the bits of
 * mask words past C / 32 included - never reach a count.  counts: int64 [T][C] with per_step != 0, else [C] (summed over
 * the timesteps); accumulate == 0 overwrites the buffer, != 0 adds to it.  Refused by name (nothing launched): an
 * unknown kind, a non-positive shape, ld too small, a mask with C % 32 != 0, a null pointer. */
int snn_activity_count(const void* src, int kind, int64_t ld, float threshold, int T, int64_t M, int C,
                       int per_step, int64_t* counts, int accumulate, void* stream);
/* Host only: out[4] = {channels per access (4 / 1; mask: 32), pixel rows per block, grid x, grid y} of exactly the
 * instance snn_activity_count launches for these arguments; `aligned` != 0: src is 16-byte (bf16: 8-byte) aligned. */
int snn_activity_count_plan(int kind, int T, int64_t M, int C, int64_t ld, int aligned, int64_t* out /*[4]*/);

#ifdef __cplusplus
}
#endif
#endif /* SNN_HIP_H */
