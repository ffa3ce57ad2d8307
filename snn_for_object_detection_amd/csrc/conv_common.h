// What the implicit-GEMM convolution family shares (gfx950):
//
//   conv_gather.hip   forward / data gradient k_conv_gather, the pre-split weight images, the spike-operand forward
//   conv_wgrad.hip    weight gradient k_conv_wgrad / k_conv_wgrad_pipe, the slab reducers, the spike-operand weight gradient
//   conv_first.hip    the event-frame layer k_conv_first (forward and weight gradient)
//
// and what the halo-resident 3x3 kernels (conv_halo.hip, wgrad_halo.hip) spell the same way: kThreads, the 16-bit and
// 32-bit vector types, the fp16 x 3 pre-scales, div_magic.  Only what two or more sources use lives here, and no kernels.
// Everything has internal linkage but the event-frame layer's geometry, plan and launch at the end: the forward
// (conv_gather.hip) and the weight gradient (conv_wgrad.hip) both launch the kernel conv_first.hip holds.
#pragma once
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;
// 3 waves / SIMD (<= 168 VGPRs): measured +5..+25 % over 2 waves / SIMD with a second LDS stage
#define SNN_CONV_MIN_WAVES 3

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// fp16 x 3 ("SPLIT = 4"): operands are pre-scaled by powers of two (exact) so that the LOW pieces stay in fp16's normal
// range: weights x 2^8 (|w| < 255), activations x 2^4 (|x| < 4094; full 22-bit precision down to |x| = 0.008, graceful
// below: absolute error 4e-9).  The accumulators are scaled back by 2^-12 in the epilogue.
constexpr float kF16WeightScale = 256.0f;
constexpr float kF16ActScale = 16.0f;
constexpr float kF16Unscale = 1.0f / (kF16WeightScale * kF16ActScale);

__device__ __forceinline__ int div_magic(int n, int d, unsigned magic) { return d == 1 ? n : (int)__umulhi((unsigned)n, magic); }

// Alignment facts a launch derives from its pointers and strides (the `align_bits` of the host-only plan queries): a
// tensor counts as vectorisable when its pointer is 16-byte (fp32) / 8-byte (bf16 storage) aligned; for an addend the bit
// also requires a pixel stride that is a multiple of 4 elements.
enum : unsigned {
    kAlignIn16 = 1u, kAlignIn8 = 2u, kAlignW16 = 4u, kAlignOut16 = 8u, kAlignOut8 = 16u, kAlignAdd16 = 32u, kAlignAdd8 = 64u,
    kAlignAdd2_16 = 128u, kAlignAdd2_8 = 256u, kAlignSplit16 = 512u, kAlignAll = 1023u
};

static int check_conv_shape(const char* name, int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH,
                            int KW, int stride, int pad) {
    SNN_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0,
                "%s: bad shape", name);
    SNN_REQUIRE(Ho == (H + 2 * pad - KH) / stride + 1 && Wo == (W + 2 * pad - KW) / stride + 1 && Ho > 0 && Wo > 0,
                "%s: output size %dx%d does not match input %dx%d k=%dx%d s=%d p=%d", name, Ho, Wo, H, W, KH, KW,
                stride, pad);
    return 0;
}

// the shapes the convolutions over spikes that were never stored cover (see k_conv_gather XSP, include/snn_hip.h)
static bool spikes_shape_ok(int64_t N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                            int64_t ld) {
    // the pipelined implicit GEMM (forward FAST path, pipelined weight gradient); 3x3 / stride 1 layers the halo-resident
    // kernels cover take those instead (snn_conv3x3_halo_spikes, k_conv_wgrad_halo NPROD 2)
    return N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH >= 1 && KW >= 1 && KH <= 5 && KW <= 5 && stride >= 1 &&
           Ho == (H + 2 * pad - KH) / stride + 1 && Wo == (W + 2 * pad - KW) / stride + 1 && Ho > 0 && Wo > 0 &&
           Cin % 32 == 0 && Cout % 4 == 0 && ld % 4 == 0 && ld >= Cin && N * (int64_t)H * W < 0x7fffffffLL &&
           N * (int64_t)Ho * Wo < 0x7fffffffLL && (int64_t)H * W * ld * 16 < 0x7fffffffLL;
}

}  // namespace

// ---- the event-frame layer (conv_first.hip), launched by snn_conv2d_fwd, snn_conv2d_wgrad and snn_conv2d_wgrad_bn
struct FirstGeom {
    int64_t ldx, ldy;
    int rows;  // N * Ho output rows
    int H, W, Ho, Wo, Cout, stride, pad;
    // Rows are dealt to the blocks in groups: group q = blockIdx / group_blocks owns rows [q, q+1) * group_rows and
    // its group_blocks blocks walk them with that stride.  One group (all rows) unless the forward pass also emits
    // BatchNorm partials: then a group is a TIMESTEP and block j of it writes chunk j of partial[t][c][chunk][2].
    int group_rows, group_blocks;
    double* bn_partial;
    // weight gradient with the BatchNorm-backward affine applied on the fly (BNAPPLY): the `dy` operand is gx and
    // dy = A[t][c] * gx + B[t][c] * y + C[t][c], t = image / frames_per_step; coef = [3][T][C]
    const float* bn_y;
    int64_t bn_ldy;
    const float* bn_coef;
    int bn_tc;   // T * C: distance between the three coefficient planes
    int bn_fps;  // frames per timestep
    int rs;      // output rows a block stages (input rows -> LDS) and computes between two barriers: first_layer_rs()
};

// The launch plan of k_conv_first, read by the three launches and by snn_conv_first_plan.  ok = 0: the shape is not
// covered (the caller checks its pointers and strides on top).  frames_per_step > 0: the forward with statistics
// partials.  num_cu: 0 the current device's.
struct FirstPlan {
    int ok;
    int rs, LW, cgs, PP;            // rows per stage, padded input row width, channel groups, pixel lanes
    int blocks;                     // grid (weight gradient: = snn_conv2d_wgrad_splitk, the slabs)
    int group_rows, group_blocks;   // see FirstGeom
    int max_rows, last_stage_rows;  // the most rows a block walks, and the rows of that block's last stage
    size_t lds;                     // dynamic LDS bytes: rs staged output rows of 3 padded input rows
};
FirstPlan snn_first_layer_plan(int64_t N, int H, int W, int Ho, int Wo, int Cout, int stride, int pad,
                               int frames_per_step, bool wgrad, int num_cu);
// the shapes k_conv_first takes: the caller checks alignment of its buffers on top
bool snn_first_layer_shape(int Cin, int Cout, int KH, int KW);
// grid of its weight gradient = the workspace slabs (num_cu <= 0: the current device's)
int snn_first_layer_blocks(int64_t rows, int num_cu);
// the one launch of k_conv_first (see conv_first.hip)
int snn_launch_first(bool wgrad, bool bnapply, bool sb, int blocks, size_t lds, const float* x, const float* w,
                     const float* dy, float* out, const FirstGeom& fg, void* stream, const char* name);

// what snn_conv1x1_mask_wgrad hard-requires of a call (conv_wgrad.hip), for snn_conv1x1_mask_supported (conv_gather.hip)
bool snn_wgrad_mask_ok(int64_t N, int H, int W, int Cin, int Cout, const uint32_t* mask, int64_t ld_mask, const float* dy,
                       int64_t lddy, const float* dw);
