// The optimiser step for gfx950: the fused Adamax family (plain, with the step control record, with the weight average
// folded in), the stand-alone average update, and the bitwise reproducible gradient-norm reduction that fills the control
// record.  All HBM-bound grid-stride loops over flat fp32 buffers; include/snn_hip.h states the rules of each entry point.
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------ Adamax
// One body, four kernels in front of it.  CTL = false is the plain step; CTL = true adds, in the order of clip_grad_* followed
// by torch.optim.Adamax: the control record's clip factor, the value clamp, the weight decay - and stores NOTHING when the
// record says the gradient was not finite (the moments would stay non-finite for ever: u = max(b2 * inf, ...) = inf).
// EMA = true moves the weight average towards the parameter it has just written, ema += ew * (p_new - ema) with
// ew = 1 - decay formed by the caller: 8 more bytes per element in the pass that holds p_new in a register anyway.  The
// parameter and both moments are computed by the same expressions in the same order whatever EMA is: the same bits.
template <bool CTL, bool EMA>
__device__ __forceinline__ void adamax_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr,
                                            float gscale, float wd, float clip, const snn_step_control* __restrict__ ctl,
                                            float* __restrict__ ema, float ew) {
    float cscale = 1.0f;
    if constexpr (CTL) {
        if (ctl) {
            if (!ctl->finite) return;
            cscale = ctl->scale;
        }
    }
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        float ge = g[e] * gscale;  // gscale = 1/world_size after a SUM all-reduce (exact for powers of two)
        if constexpr (CTL) {
            ge *= cscale;                                                      // clip_grad_norm_: grad.mul_(clip_coef)
            if (clip > 0.0f) ge = ge < -clip ? -clip : (ge > clip ? clip : ge);  // clip_grad_value_ (a NaN stays a NaN)
            if (wd != 0.0f) ge += wd * p[e];                                   // grad.add(param, alpha=weight_decay)
        }
        // torch.optim.Adamax single-tensor: exp_avg.lerp_(grad, 1-beta1); exp_inf = max(exp_inf*beta2, |g|+eps)
        float me = m[e] + w1 * (ge - m[e]);
        float ue = fmaxf(u[e] * b2, fabsf(ge) + eps);
        m[e] = me;
        u[e] = ue;
        const float pe = p[e] - clr * (me / ue);
        p[e] = pe;
        if constexpr (EMA) {
            const float a = ema[e];
            ema[e] = a + ew * (pe - a);
        }
    }
}
__global__ void k_adamax(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                         float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr, float gscale) {
    adamax_body<false, false>(p, g, m, u, n, w1, b2, eps, clr, gscale, 0.0f, 0.0f, nullptr, nullptr, 0.0f);
}
__global__ void k_adamax_ctl(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ u, int64_t n, float w1, float b2, float eps, float clr, float gscale,
                             float wd, float clip, const snn_step_control* __restrict__ ctl) {
    adamax_body<true, false>(p, g, m, u, n, w1, b2, eps, clr, gscale, wd, clip, ctl, nullptr, 0.0f);
}
// CTL mirrors snn_adamax_step_ctl's choice between the two kernels above, so the parameter and the moments come out of the
// same instantiation of the arithmetic in either case.
template <bool CTL>
__global__ void k_adamax_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ u, float* __restrict__ ema, int64_t n, float w1, float b2, float eps,
                             float clr, float gscale, float wd, float clip, float ew,
                             const snn_step_control* __restrict__ ctl) {
    adamax_body<CTL, true>(p, g, m, u, n, w1, b2, eps, clr, gscale, wd, clip, ctl, ema, ew);
}
// The same update from an arbitrary source: parameters that received no gradient in a step (Adamax leaves them alone, the
// average does not) and the BatchNorm buffers.  A record that says "not finite" stores nothing here either.
__global__ void k_ema_update(float* __restrict__ ema, const float* __restrict__ src, int64_t n, float ew,
                             const snn_step_control* __restrict__ ctl) {
    if (ctl && !ctl->finite) return;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const float a = ema[e];
        ema[e] = a + ew * (src[e] - a);
    }
}

// ------------------------------------------------------------------------------------------ gradient norm
// sum g^2 over a flat gradient, bitwise reproducible: block b owns the kNormRun elements [b * kNormRun, (b + 1) * kNormRun)
// of the buffer counted from the 16-byte boundary at or below its first element (`shift` = 0..3 floats in front of it), so
// every full group of four is one aligned 16-byte load whatever the base pointer is; the groups cut by either end of the
// buffer (at most two in the whole launch) are read element by element.  A thread adds its squares in index order, the wave
// and the block combine in a fixed butterfly, and the second kernel adds the block partials in index order: no atomics,
// and nothing that depends on the device - the run length is a constant, not a function of the CU count.
constexpr int kNormRun = 8192;
constexpr int kNormGroups = kNormRun / (4 * kThreads);   // 16-byte groups per thread

__device__ __forceinline__ double block_sum_ordered(double acc) {
    __shared__ double wave_sum[kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += wave_sum[w];
    return s;   // the same value in every thread
}

__global__ void k_grad_norm_partial(const float* __restrict__ g, int64_t n, int shift, double* __restrict__ partial) {
    const int64_t end = n + shift;   // the buffer is [shift, end) on the aligned grid; g points at element `shift`
    const int64_t v0 = (int64_t)blockIdx.x * kNormRun;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kNormGroups; ++k) {
        const int64_t v = v0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
        if (v >= shift && v + 4 <= end) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(g + (v - shift));
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j >= shift && v + j < end) {
                    const double d = (double)g[v + j - shift];
                    acc += d * d;
                }
        }
    }
    const double s = block_sum_ordered(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void k_grad_norm_finish(const double* __restrict__ partial, int64_t blocks, float grad_scale, float max_norm,
                                   snn_step_control* __restrict__ ctl) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < blocks; i += kThreads) acc += partial[i];
    const double sum = block_sum_ordered(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)((double)grad_scale * sqrt(sum));
        float scale = 1.0f;
        if (max_norm > 0.0f) {   // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
            scale = max_norm / (norm + 1e-6f);
            if (scale > 1.0f) scale = 1.0f;
        }
        const int finite = isfinite(sum) ? 1 : 0;   // an inf or NaN element makes the fp64 sum of squares non-finite
        ctl->norm = norm;
        ctl->scale = scale;
        ctl->finite = finite;
        ctl->skipped += 1 - finite;
    }
}

// ------------------------------------------------------------------------------------------ launch helpers
// ema_weight = 1 - decay in (0, 1] (false for a NaN): 0 would never move the average, above 1 it would overshoot
bool ema_weight_ok(float w) { return w > 0.0f && w <= 1.0f; }

int64_t grad_norm_blocks(int64_t n, int shift) { return snn_ceil_div(n + shift, kNormRun); }

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
extern "C" int snn_adamax_step(float* param, const float* grad, float* exp_avg, float* exp_inf, int64_t n, float lr,
                               float beta1, float beta2, float eps, int step, float grad_scale, void* stream) {
    SNN_REQUIRE(param && grad && exp_avg && exp_inf && n > 0 && step >= 1, "snn_adamax_step: bad arguments");
    // clr = lr / (1 - beta1^step)
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    hipLaunchKernelGGL(k_adamax, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_inf, n, w1, beta2, eps, clr, grad_scale);
    SNN_CHECK_LAUNCH("snn_adamax_step");
    return 0;
}

extern "C" int snn_adamax_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_inf, int64_t n, float lr,
                                   float beta1, float beta2, float eps, int step, float grad_scale, float weight_decay,
                                   float clip_value, const snn_step_control* ctl, void* stream) {
    SNN_REQUIRE(param && grad && exp_avg && exp_inf && n > 0 && step >= 1, "snn_adamax_step_ctl: bad arguments");
    SNN_REQUIRE(weight_decay >= 0.0f, "snn_adamax_step_ctl: negative weight_decay");   // (false for a NaN too)
    SNN_REQUIRE(aligned(4, {ctl}), "snn_adamax_step_ctl: the control record must be 4-byte aligned");
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    if (!ctl && weight_decay == 0.0f && !(clip_value > 0.0f))   // nothing to add: the plain kernel, the same bits
        hipLaunchKernelGGL(k_adamax, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, param,
                           grad, exp_avg, exp_inf, n, w1, beta2, eps, clr, grad_scale);
    else
        hipLaunchKernelGGL(k_adamax_ctl, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, param,
                           grad, exp_avg, exp_inf, n, w1, beta2, eps, clr, grad_scale, weight_decay, clip_value, ctl);
    SNN_CHECK_LAUNCH("snn_adamax_step_ctl");
    return 0;
}

extern "C" int snn_adamax_step_ema(float* param, const float* grad, float* exp_avg, float* exp_inf, float* ema, int64_t n,
                                   float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                                   float weight_decay, float clip_value, float ema_weight, const snn_step_control* ctl,
                                   void* stream) {
    SNN_REQUIRE(param, "snn_adamax_step_ema: param is NULL");
    SNN_REQUIRE(grad, "snn_adamax_step_ema: grad is NULL");
    SNN_REQUIRE(exp_avg, "snn_adamax_step_ema: exp_avg is NULL");
    SNN_REQUIRE(exp_inf, "snn_adamax_step_ema: exp_inf is NULL");
    SNN_REQUIRE(ema, "snn_adamax_step_ema: ema is NULL");
    SNN_REQUIRE(n > 0, "snn_adamax_step_ema: n = %lld must be positive", (long long)n);
    SNN_REQUIRE(step >= 1, "snn_adamax_step_ema: step = %d must be at least 1", step);
    SNN_REQUIRE(weight_decay >= 0.0f, "snn_adamax_step_ema: negative weight_decay");   // (false for a NaN too)
    SNN_REQUIRE(ema_weight_ok(ema_weight), "snn_adamax_step_ema: ema_weight = %g is outside (0, 1]", (double)ema_weight);
    SNN_REQUIRE(aligned(4, {ctl}), "snn_adamax_step_ema: the control record must be 4-byte aligned");
    double bias_corr = 1.0 - pow((double)beta1, (double)step);
    float clr = (float)((double)lr / bias_corr);
    float w1 = (float)(1.0 - (double)beta1);
    if (!ctl && weight_decay == 0.0f && !(clip_value > 0.0f))   // where snn_adamax_step_ctl launches the plain kernel
        hipLaunchKernelGGL(k_adamax_ema<false>, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                           param, grad, exp_avg, exp_inf, ema, n, w1, beta2, eps, clr, grad_scale, 0.0f, 0.0f,
                           ema_weight, nullptr);
    else
        hipLaunchKernelGGL(k_adamax_ema<true>, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                           param, grad, exp_avg, exp_inf, ema, n, w1, beta2, eps, clr, grad_scale, weight_decay,
                           clip_value, ema_weight, ctl);
    SNN_CHECK_LAUNCH("snn_adamax_step_ema");
    return 0;
}

extern "C" int snn_ema_update(float* ema, const float* src, int64_t n, float ema_weight, const snn_step_control* ctl,
                              void* stream) {
    SNN_REQUIRE(ema, "snn_ema_update: ema is NULL");
    SNN_REQUIRE(src, "snn_ema_update: src is NULL");
    SNN_REQUIRE(n > 0, "snn_ema_update: n = %lld must be positive", (long long)n);
    SNN_REQUIRE(ema_weight_ok(ema_weight), "snn_ema_update: ema_weight = %g is outside (0, 1]", (double)ema_weight);
    SNN_REQUIRE(aligned(4, {ctl}), "snn_ema_update: the control record must be 4-byte aligned");
    hipLaunchKernelGGL(k_ema_update, dim3(snn_grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ema, src,
                       n, ema_weight, ctl);
    SNN_CHECK_LAUNCH("snn_ema_update");
    return 0;
}

extern "C" size_t snn_grad_norm_workspace_size(int64_t n) {
    return n > 0 ? (size_t)grad_norm_blocks(n, 3) * sizeof(double) : 0;   // (3: the largest shift of an unaligned base)
}

extern "C" int snn_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, void* ws,
                             snn_step_control* ctl, void* stream) {
    SNN_REQUIRE(grad && ws && ctl && n > 0, "snn_grad_norm: bad arguments");
    SNN_REQUIRE(aligned(4, {grad, ctl}) && aligned(8, {ws}),
                "snn_grad_norm: grad and ctl must be 4-byte aligned, the workspace 8-byte aligned");
    const int shift = (int)((reinterpret_cast<uintptr_t>(grad) & 15u) / 4);
    const int64_t blocks = grad_norm_blocks(n, shift);
    SNN_REQUIRE(blocks <= 0x7fffffff, "snn_grad_norm: %lld elements are more than one launch covers", (long long)n);
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_grad_norm_partial, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, grad, n, shift,
                       partial);
    SNN_CHECK_LAUNCH("snn_grad_norm");
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partial, blocks, grad_scale,
                       max_norm, ctl);
    SNN_CHECK_LAUNCH("snn_grad_norm");
    return 0;
}
