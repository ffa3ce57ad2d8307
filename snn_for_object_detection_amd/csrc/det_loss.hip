// The detection loss: one kernel family behind the nine snn_det_loss* entry points - one thread per
// anchor row, fp32 per-row arithmetic, fp64 block and grid sums in a fixed order - with a choice of the classification
// term (cross entropy | focal) and of the box term (L1 | GIoU | DIoU | CIoU).
//
//   cls  = ratio * sum_pos f / n_pos + (1 - ratio) * sum_neg f / n_neg
//          f = ce (cross entropy) or (1 - p_y)^gamma * ce (focal), ce = -log softmax(x)[y], pos: class > 0
//   box  = box_weight * sum |bbox m - off m| / (4 A V)                                   (L1)
//        = box_weight * sum over box rows (1 - IoU + penalty) / max(n_pos, 1)            (GIoU, DIoU, CIoU)
//          box rows: class > 0 and all four mask entries 1; the boxes are offset_inverse(anchor[r % A], .) of the
//          predicted and of the target offsets, the exponent argument clamped above at log(1000 / 16)
//   loss = cls + box
//
// The means of cls come in two conventions.  snn_det_loss_fwd and snn_det_loss_steps_fwd (cross entropy, L1, weight 1:
// SODa._loss, models/soda.py:259-281) divide by n_pos / n_neg as they are - an empty class gives NaN, as the reference's
// ce[pos].mean() does; snn_det_loss_ext_fwd divides by max(n, 1) and gives 0.  The gradients do not differ: the weight of
// an empty class multiplies no row.
//
// V = the frames that take part (rows / A, or the valid slots of steps[], counted on the device); rows of an empty slot
// are left out of every sum and get exact zeros as gradients.  Nothing here synchronises with the host or allocates.
#include "snn_common.h"

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 1024;
constexpr int kMaxClasses = 64;
constexpr int kMaxFrames = 1 << 20;    // frames (rows / A) snn_det_loss_ext_* take
constexpr float kExpClamp = 4.135166556742356f;   // log(1000 / 16): a decoded side is at most 62.5 anchor sides
constexpr float kIouEps = 1e-7f;
constexpr float kFourOverPiSq = 0.4052847345693511f;

__device__ __forceinline__ double block_sum(double v, double* scratch) {  // all threads get the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < kLossThreads / 64; ++k) s += scratch[k];
    return s;
}

struct Softmax {
    float mx, se, so, ce;   // row maximum, sum of exp(x - mx), the same without the label's own term, cross entropy
};
__device__ __forceinline__ Softmax row_softmax(const float* __restrict__ x, int K, int64_t y) {
    Softmax s;
    s.mx = x[0];
    for (int k = 1; k < K; ++k) s.mx = fmaxf(s.mx, x[k]);
    s.se = 0.f;
    s.so = 0.f;
    for (int k = 0; k < K; ++k) {
        const float e = expf(x[k] - s.mx);
        s.se += e;
        if (k != y) s.so += e;
    }
    // -log_softmax(x)[y] as torch forms it, log(se) - (x[y] - mx): two terms >= 0.  (mx + log(se)) - x[y] rounds at the
    // size of mx and loses the loss of a well-classified row with large logits.
    s.ce = logf(s.se) - (x[y] - s.mx);
    return s;
}

__device__ __forceinline__ bool box_row(int64_t y, const float4 mk) {
    return y > 0 && mk.x == 1.0f && mk.y == 1.0f && mk.z == 1.0f && mk.w == 1.0f;
}

struct Box {
    float cx, cy, w, h;
    bool free_w, free_h;   // the exponent argument lies below the clamp: the size follows its offset
};
// offset_inverse (utils/box.py:72-79) in centre form: centre ox * wa / 10 + cxa, size exp(min(ow / 5, clamp)) * wa
__device__ __forceinline__ Box decode_box(const float4 anc, const float4 o) {
    const float cxa = (anc.x + anc.z) / 2, cya = (anc.y + anc.w) / 2, wa = anc.z - anc.x, ha = anc.w - anc.y;
    const float aw = o.z / 5, ah = o.w / 5;
    Box b;
    b.cx = o.x * wa / 10 + cxa;
    b.cy = o.y * ha / 10 + cya;
    b.free_w = aw <= kExpClamp;
    b.free_h = ah <= kExpClamp;
    b.w = expf(b.free_w ? aw : kExpClamp) * wa;
    b.h = expf(b.free_h ? ah : kExpClamp) * ha;
    return b;
}

// 1 - IoU + penalty of the decoded prediction against the decoded target.  kGrad: *grad = d loss / d (the four raw
// predicted offsets), through the decode; alpha of CIoU is a constant there.
template <bool kGrad>
__device__ __forceinline__ float iou_loss(int mode, const float4 anc, const float4 pred, const float4 target,
                                          float4* grad) {
    const Box p = decode_box(anc, pred), g = decode_box(anc, target);
    const float px1 = p.cx - 0.5f * p.w, py1 = p.cy - 0.5f * p.h, px2 = p.cx + 0.5f * p.w, py2 = p.cy + 0.5f * p.h;
    const float gx1 = g.cx - 0.5f * g.w, gy1 = g.cy - 0.5f * g.h, gx2 = g.cx + 0.5f * g.w, gy2 = g.cy + 0.5f * g.h;
    const float ap = (px2 - px1) * (py2 - py1), ag = (gx2 - gx1) * (gy2 - gy1);
    const float dw = fminf(px2, gx2) - fmaxf(px1, gx1), dh = fminf(py2, gy2) - fmaxf(py1, gy1);
    const float iw = fmaxf(dw, 0.f), ih = fmaxf(dh, 0.f);
    const float inter = iw * ih;
    const float uni = ap + ag - inter, ue = uni + kIouEps;
    const float iou = inter / ue;
    const float cw = fmaxf(px2, gx2) - fminf(px1, gx1), ch = fmaxf(py2, gy2) - fminf(py1, gy1);
    float pen = 0.f;
    // d loss / d (inter, area of the prediction, cw, ch, squared centre distance, v)
    float c_inter = 0.f, c_ap = 0.f, c_cw = 0.f, c_ch = 0.f, c_rho = 0.f, c_v = 0.f;
    if (kGrad) {
        c_inter = -((ue + inter) / (ue * ue));
        c_ap = inter / (ue * ue);
    }
    const float ex = p.cx - g.cx, ey = p.cy - g.cy;
    float atd = 0.f, tp = 0.f, hpe = 0.f;
    if (mode == SNN_LOSS_BOX_GIOU) {
        const float C = cw * ch, ce = C + kIouEps;
        pen = (C - uni) / ce;
        if (kGrad) {
            const float dC = ue / (ce * ce);
            c_cw = dC * ch;
            c_ch = dC * cw;
            c_ap += -1.0f / ce;
            c_inter += 1.0f / ce;
        }
    } else {
        const float rho2 = ex * ex + ey * ey, c2e = (cw * cw + ch * ch) + kIouEps;
        pen = rho2 / c2e;
        if (kGrad) {
            const float dc2 = -(rho2 / (c2e * c2e));
            c_rho = 1.0f / c2e;
            c_cw = dc2 * (2.0f * cw);
            c_ch = dc2 * (2.0f * ch);
        }
        if (mode == SNN_LOSS_BOX_CIOU) {
            hpe = (py2 - py1) + kIouEps;
            tp = (px2 - px1) / hpe;
            atd = atanf((gx2 - gx1) / ((gy2 - gy1) + kIouEps)) - atanf(tp);
            const float v = kFourOverPiSq * (atd * atd);
            const float alpha = v / (((1.0f - iou) + v) + kIouEps);
            pen += alpha * v;
            c_v = alpha;
        }
    }
    if (kGrad) {
        // corners of the prediction: the intersection follows the inner, the enclosing box the outer corner
        const float ox = dw > 0.f ? ih : 0.f, oy = dh > 0.f ? iw : 0.f;   // d inter / d iw, d inter / d ih
        const float g_x1 = c_inter * (px1 > gx1 ? -ox : 0.f) + c_cw * (px1 < gx1 ? -1.0f : 0.f);
        const float g_x2 = c_inter * (px2 < gx2 ? ox : 0.f) + c_cw * (px2 > gx2 ? 1.0f : 0.f);
        const float g_y1 = c_inter * (py1 > gy1 ? -oy : 0.f) + c_ch * (py1 < gy1 ? -1.0f : 0.f);
        const float g_y2 = c_inter * (py2 < gy2 ? oy : 0.f) + c_ch * (py2 > gy2 ? 1.0f : 0.f);
        // the corners are cx -+ w / 2; ap = (x2 - x1) (y2 - y1), the squared distance and v (of x2 - x1, y2 - y1) directly
        float g_cx = (g_x1 + g_x2) + c_rho * (2.0f * ex), g_cy = (g_y1 + g_y2) + c_rho * (2.0f * ey);
        float g_w = 0.5f * (g_x2 - g_x1) + c_ap * (py2 - py1), g_h = 0.5f * (g_y2 - g_y1) + c_ap * (px2 - px1);
        if (mode == SNN_LOSS_BOX_CIOU) {
            const float dv = c_v * (kFourOverPiSq * (2.0f * atd)) * (-1.0f / (1.0f + tp * tp));   // d loss / d tp
            g_w += dv / hpe;
            g_h += dv * (-(tp / hpe));
        }
        const float wa = anc.z - anc.x, ha = anc.w - anc.y;
        grad->x = g_cx * (wa / 10);
        grad->y = g_cy * (ha / 10);
        grad->z = p.free_w ? g_w * (p.w / 5) : 0.f;
        grad->w = p.free_h ? g_h * (p.h / 5) : 0.f;
    }
    return (1.0f - iou) + pen;
}

struct LossArgs {
    const float* logits;
    const float* bbox;
    const float* offset;
    const float* mask;
    const int64_t* cls;
    const float* anchors;   // [A][4], read by the IoU box modes only
    const int* steps;       // [rows / A], nullptr: every frame takes part
    int64_t R;
    int A, K;
    float ratio;
    int cls_mode;
    float gamma;
    int box_mode;
    float box_weight;
};

// partial[block][5] = {sum f over positives, positives, sum f over negatives, negatives, box sum}
template <bool kSteps>
__global__ __launch_bounds__(kLossThreads) void k_det_loss_partial(const LossArgs a, double* __restrict__ partial) {
    __shared__ double scratch[kLossThreads / 64];
    double s_pos = 0, n_pos = 0, s_neg = 0, n_neg = 0, s_box = 0;
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * kLossThreads) {
        if (kSteps && a.steps[r / a.A] < 0) continue;
        const int64_t y = a.cls[r];
        const Softmax s = row_softmax(a.logits + r * a.K, a.K, y);
        float f = s.ce;
        if (a.cls_mode == SNN_LOSS_CLS_FOCAL) f = powf(s.so / s.se, a.gamma) * s.ce;
        if (y > 0) {
            s_pos += f;
            n_pos += 1;
        } else {
            s_neg += f;
            n_neg += 1;
        }
        const float4 bb = *reinterpret_cast<const float4*>(a.bbox + r * 4);
        const float4 of = *reinterpret_cast<const float4*>(a.offset + r * 4);
        const float4 mk = *reinterpret_cast<const float4*>(a.mask + r * 4);
        if (a.box_mode == SNN_LOSS_BOX_L1) {
            s_box += (double)fabsf(bb.x * mk.x - of.x * mk.x) + (double)fabsf(bb.y * mk.y - of.y * mk.y) +
                     (double)fabsf(bb.z * mk.z - of.z * mk.z) + (double)fabsf(bb.w * mk.w - of.w * mk.w);
        } else if (box_row(y, mk)) {
            const float4 anc = *reinterpret_cast<const float4*>(a.anchors + (r % a.A) * 4);
            s_box += iou_loss<false>(a.box_mode, anc, bb, of, nullptr);
        }
    }
    const double t0 = block_sum(s_pos, scratch), t1 = block_sum(n_pos, scratch);
    const double t2 = block_sum(s_neg, scratch), t3 = block_sum(n_neg, scratch);
    const double t4 = block_sum(s_box, scratch);
    if (threadIdx.x == 0) {
        double* p = partial + (int64_t)blockIdx.x * 5;
        p[0] = t0; p[1] = t1; p[2] = t2; p[3] = t3; p[4] = t4;
    }
}

// stats[n_stats], n_stats = 5, 6 or 9: the five totals (fixed order: reproducible), then V, then the three terms of the
// loss: ratio * mean over the positives, (1 - ratio) * mean over the negatives, the box term.  loss = (the first + the
// second) + the third.  strict_means: the two means divide by the counts as they are (an empty class: NaN), otherwise
// by max(count, 1).  frames = rows / A; with steps, V counts the valid ones among them.
__global__ __launch_bounds__(64) void k_det_loss_final(const double* __restrict__ partial, int nblocks,
                                                       const int* __restrict__ steps, int64_t frames, int A, float ratio,
                                                       int box_mode, float box_weight, bool strict_means, int n_stats,
                                                       double* __restrict__ stats, float* __restrict__ loss) {
    if (blockIdx.x != 0) return;
    int64_t v = frames;
    if (steps) {
        int c = 0;
        for (int i = threadIdx.x; i < frames; i += 64) c += steps[i] >= 0 ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        v = c;
    }
    // lane l adds the blocks l, l + 64, ... in that order, then the 64 lane sums meet in a butterfly: a fixed order for a
    // given block count (one thread walking up to 1024 x 5 partials costs more than the partial kernel itself)
    double t[5];
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += 64) s += partial[(int64_t)b * 5 + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        t[k] = s;
    }
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 5; ++k) stats[k] = t[k];
    float gt = 0.f, bg = 0.f, bx = 0.f;
    if (v > 0) {
        gt = (float)(t[0] / (strict_means ? t[1] : fmax(t[1], 1.0))) * ratio;
        bg = (float)(t[2] / (strict_means ? t[3] : fmax(t[3], 1.0))) * (1 - ratio);
        const double den = box_mode == SNN_LOSS_BOX_L1 ? 4.0 * (double)A * (double)v : fmax(t[1], 1.0);
        bx = (float)(t[4] / den) * box_weight;
    }
    if (n_stats > 5) stats[5] = (double)v;
    if (n_stats > 6) {
        stats[6] = gt;
        stats[7] = bg;
        stats[8] = bx;
    }
    *loss = (gt + bg) + bx;
}

// Reads the counts stats[1], stats[3] and, with steps, V = stats[5]; without steps V = rows / A.
template <bool kSteps>
__global__ __launch_bounds__(kLossThreads) void k_det_loss_bwd(const LossArgs a, const double* __restrict__ stats,
                                                               const float* __restrict__ g_loss,
                                                               float* __restrict__ g_logits, float* __restrict__ g_bbox) {
    const float g = *g_loss;
    const float n_pos = fmaxf((float)stats[1], 1.0f), n_neg = fmaxf((float)stats[3], 1.0f);
    const float w_pos = g * a.ratio / n_pos, w_neg = g * (1 - a.ratio) / n_neg;
    const int64_t v = kSteps ? (int64_t)stats[5] : a.R / a.A;
    const float w_box = a.box_mode == SNN_LOSS_BOX_L1 ? g * a.box_weight / (4.0f * (float)((int64_t)a.A * v))
                                                      : g * a.box_weight / n_pos;
    const int K = a.K;
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * kLossThreads) {
        if (kSteps && a.steps[r / a.A] < 0) {
            for (int k = 0; k < K; ++k) g_logits[r * K + k] = 0.f;
            *reinterpret_cast<float4*>(g_bbox + r * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float* x = a.logits + r * K;
        const int64_t y = a.cls[r];
        const Softmax s = row_softmax(x, K, y);
        float w = y > 0 ? w_pos : w_neg;
        if (a.cls_mode == SNN_LOSS_CLS_FOCAL) {
            // d ((1 - p_y)^gamma ce) / d x_k = (p_k - [k == y]) q^gamma (1 + gamma p_y ce / q), q = 1 - p_y; ce / q -> 1
            // as q -> 0, so nothing is divided by a power of q
            const float q = s.so / s.se, py = expf(x[y] - s.mx) / s.se;
            w *= q > 0.f ? powf(q, a.gamma) * (1.0f + a.gamma * py * (s.ce / q)) : (a.gamma == 0.f ? 1.0f : 0.f);
        }
        for (int k = 0; k < K; ++k) {
            const float p = expf(x[k] - s.mx) / s.se;
            g_logits[r * K + k] = w * (p - (k == y ? 1.0f : 0.0f));
        }
        const float4 bb = *reinterpret_cast<const float4*>(a.bbox + r * 4);
        const float4 of = *reinterpret_cast<const float4*>(a.offset + r * 4);
        const float4 mk = *reinterpret_cast<const float4*>(a.mask + r * 4);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.box_mode == SNN_LOSS_BOX_L1) {
            auto sgn = [](float v) { return v > 0.f ? 1.0f : (v < 0.f ? -1.0f : 0.0f); };
            o.x = w_box * sgn(bb.x * mk.x - of.x * mk.x) * mk.x;
            o.y = w_box * sgn(bb.y * mk.y - of.y * mk.y) * mk.y;
            o.z = w_box * sgn(bb.z * mk.z - of.z * mk.z) * mk.z;
            o.w = w_box * sgn(bb.w * mk.w - of.w * mk.w) * mk.w;
        } else if (box_row(y, mk)) {
            const float4 anc = *reinterpret_cast<const float4*>(a.anchors + (r % a.A) * 4);
            float4 d;
            iou_loss<true>(a.box_mode, anc, bb, of, &d);
            o = make_float4(w_box * d.x, w_box * d.y, w_box * d.z, w_box * d.w);
        }
        *reinterpret_cast<float4*>(g_bbox + r * 4) = o;
    }
}

int ext_blocks(int64_t R) {   // one row per thread and pass, at most kLossMaxBlocks blocks
    int64_t b = snn_ceil_div(R, (int64_t)kLossThreads);
    if (b > kLossMaxBlocks) b = kLossMaxBlocks;
    return b < 1 ? 1 : (int)b;
}
size_t workspace_size(int64_t rows) { return (size_t)ext_blocks(rows) * 5 * sizeof(double); }

// The launchers every entry point ends in; the arguments have been checked by the caller.  n_stats: the doubles of stats
// the caller owns (5: the totals; 6: and V; 9: and the three terms).
int launch_fwd(const char* name, const LossArgs& a, bool strict_means, int n_stats, void* workspace, double* stats,
               float* loss, void* stream) {
    const int nb = ext_blocks(a.R);
    double* partial = static_cast<double*>(workspace);
    if (a.steps)
        hipLaunchKernelGGL(k_det_loss_partial<true>, dim3((unsigned)nb), dim3(kLossThreads), 0, (hipStream_t)stream, a,
                           partial);
    else
        hipLaunchKernelGGL(k_det_loss_partial<false>, dim3((unsigned)nb), dim3(kLossThreads), 0, (hipStream_t)stream, a,
                           partial);
    hipLaunchKernelGGL(k_det_loss_final, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partial, nb, a.steps,
                       a.R / a.A, a.A, a.ratio, a.box_mode, a.box_weight, strict_means, n_stats, stats, loss);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

int launch_bwd(const char* name, const LossArgs& a, const double* stats, const float* g_loss, float* g_logits,
               float* g_bbox, void* stream) {
    const int nb = ext_blocks(a.R);
    if (a.steps)
        hipLaunchKernelGGL(k_det_loss_bwd<true>, dim3((unsigned)nb), dim3(kLossThreads), 0, (hipStream_t)stream, a, stats,
                           g_loss, g_logits, g_bbox);
    else
        hipLaunchKernelGGL(k_det_loss_bwd<false>, dim3((unsigned)nb), dim3(kLossThreads), 0, (hipStream_t)stream, a, stats,
                           g_loss, g_logits, g_bbox);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

// SODa._loss: cross entropy, L1, weight 1, no anchors
LossArgs reference_objective(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                             const float* bbox_mask, const int64_t* class_labels, const int* steps, int64_t rows, int A,
                             int K, float loss_ratio) {
    return {cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, nullptr, steps, rows, A, K, loss_ratio,
            SNN_LOSS_CLS_CE, 0.f, SNN_LOSS_BOX_L1, 1.0f};
}

}  // namespace

// ------------------------------------------------------------------------------------------ one frame per row, stats[5]
extern "C" size_t snn_det_loss_workspace_size(int64_t rows) { return workspace_size(rows); }

extern "C" int snn_det_loss_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                const float* bbox_mask, const int64_t* class_labels, int64_t rows, int K,
                                float loss_ratio, void* workspace, double* stats, float* loss, void* stream) {
    SNN_REQUIRE(cls_logits && bbox_preds && bbox_offset && bbox_mask && class_labels && workspace && stats && loss,
                "snn_det_loss_fwd: null pointer");
    SNN_REQUIRE(rows > 0 && K > 1 && K <= kMaxClasses, "snn_det_loss_fwd: bad shape");
    SNN_REQUIRE(aligned(16, {bbox_preds, bbox_offset, bbox_mask}), "snn_det_loss_fwd: box tensors must be 16-byte aligned");
    return launch_fwd("snn_det_loss_fwd",
                      reference_objective(cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, nullptr, rows, 1,
                                          K, loss_ratio), true, 5, workspace, stats, loss, stream);
}

extern "C" int snn_det_loss_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                const float* bbox_mask, const int64_t* class_labels, int64_t rows, int K,
                                float loss_ratio, const double* stats, const float* g_loss, float* g_logits,
                                float* g_bbox, void* stream) {
    SNN_REQUIRE(cls_logits && bbox_preds && bbox_offset && bbox_mask && class_labels && stats && g_loss && g_logits &&
                    g_bbox, "snn_det_loss_bwd: null pointer");
    SNN_REQUIRE(rows > 0 && K > 1 && K <= kMaxClasses, "snn_det_loss_bwd: bad shape");
    SNN_REQUIRE(aligned(16, {bbox_preds, bbox_offset, bbox_mask, g_bbox}),
                "snn_det_loss_bwd: box tensors must be 16-byte aligned");
    return launch_bwd("snn_det_loss_bwd",
                      reference_objective(cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, nullptr, rows, 1,
                                          K, loss_ratio), stats, g_loss, g_logits, g_bbox, stream);
}

// ------------------------------------------------------------------------------------------ K x B slots, stats[6]
extern "C" size_t snn_det_loss_steps_workspace_size(int K, int B, int A) { return workspace_size((int64_t)K * B * A); }

extern "C" int snn_det_loss_steps_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                      const float* bbox_mask, const int64_t* class_labels, const int* steps, int K, int B,
                                      int A, int C, float loss_ratio, void* workspace, double* stats, float* loss,
                                      void* stream) {
    SNN_REQUIRE(cls_logits && bbox_preds && bbox_offset && bbox_mask && class_labels && steps && workspace && stats &&
                    loss, "snn_det_loss_steps_fwd: null pointer");
    SNN_REQUIRE(B > 0 && A > 0 && C > 1 && C <= kMaxClasses, "snn_det_loss_steps_fwd: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps, "snn_det_loss_steps_fwd: K must be in 1 .. %d", kMaxLabelSteps);
    SNN_REQUIRE(aligned(16, {bbox_preds, bbox_offset, bbox_mask}),
                "snn_det_loss_steps_fwd: box tensors must be 16-byte aligned");
    return launch_fwd("snn_det_loss_steps_fwd",
                      reference_objective(cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, steps,
                                          (int64_t)K * B * A, A, C, loss_ratio), true, 6, workspace, stats, loss, stream);
}

extern "C" int snn_det_loss_steps_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                      const float* bbox_mask, const int64_t* class_labels, const int* steps, int K, int B,
                                      int A, int C, float loss_ratio, const double* stats, const float* g_loss,
                                      float* g_logits, float* g_bbox, void* stream) {
    SNN_REQUIRE(cls_logits && bbox_preds && bbox_offset && bbox_mask && class_labels && steps && stats && g_loss &&
                    g_logits && g_bbox, "snn_det_loss_steps_bwd: null pointer");
    SNN_REQUIRE(B > 0 && A > 0 && C > 1 && C <= kMaxClasses, "snn_det_loss_steps_bwd: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps, "snn_det_loss_steps_bwd: K must be in 1 .. %d", kMaxLabelSteps);
    SNN_REQUIRE(aligned(16, {bbox_preds, bbox_offset, bbox_mask, g_bbox}),
                "snn_det_loss_steps_bwd: box tensors must be 16-byte aligned");
    return launch_bwd("snn_det_loss_steps_bwd",
                      reference_objective(cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, steps,
                                          (int64_t)K * B * A, A, C, loss_ratio), stats, g_loss, g_logits, g_bbox, stream);
}

// ------------------------------------------------------------------------------------------ selectable, stats[9]
extern "C" size_t snn_det_loss_ext_workspace_size(int64_t rows) { return workspace_size(rows); }

// the refusals the forward and the backward of snn_det_loss_ext_* share; 0 when the arguments are taken
static int ext_check(const char* name, const LossArgs& a) {
    SNN_REQUIRE(a.logits && a.bbox && a.offset && a.mask && a.cls && a.anchors, "%s: null pointer", name);
    SNN_REQUIRE(a.K >= 1 && a.K <= kMaxClasses, "%s: K must be in 1 .. %d", name, kMaxClasses);
    SNN_REQUIRE(a.A > 0 && a.R > 0 && a.R % a.A == 0 && a.R / a.A <= kMaxFrames,
                "%s: rows must be a positive multiple of A (at most %d frames)", name, kMaxFrames);
    SNN_REQUIRE(a.cls_mode == SNN_LOSS_CLS_CE || a.cls_mode == SNN_LOSS_CLS_FOCAL, "%s: unknown cls_mode %d", name,
                a.cls_mode);
    SNN_REQUIRE(a.box_mode == SNN_LOSS_BOX_L1 || a.box_mode == SNN_LOSS_BOX_GIOU || a.box_mode == SNN_LOSS_BOX_DIOU ||
                    a.box_mode == SNN_LOSS_BOX_CIOU, "%s: unknown box_mode %d", name, a.box_mode);
    SNN_REQUIRE(a.gamma >= 0.f, "%s: gamma must be >= 0", name);   // (a NaN is refused too)
    SNN_REQUIRE(aligned(16, {a.bbox, a.offset, a.mask, a.anchors}), "%s: box tensors and anchors must be 16-byte aligned",
                name);
    return 0;
}

extern "C" int snn_det_loss_ext_fwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                    const float* bbox_mask, const int64_t* class_labels, const float* anchors,
                                    const int* steps, int64_t rows, int A, int K, float loss_ratio, int cls_mode,
                                    float gamma, int box_mode, float box_weight, void* workspace, double* stats,
                                    float* loss, void* stream) {
    const LossArgs a = {cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, rows, A, K,
                        loss_ratio, cls_mode, gamma, box_mode, box_weight};
    if (int rc = ext_check("snn_det_loss_ext_fwd", a)) return rc;
    SNN_REQUIRE(workspace && stats && loss, "snn_det_loss_ext_fwd: null pointer");
    return launch_fwd("snn_det_loss_ext_fwd", a, false, 9, workspace, stats, loss, stream);
}

extern "C" int snn_det_loss_ext_bwd(const float* cls_logits, const float* bbox_preds, const float* bbox_offset,
                                    const float* bbox_mask, const int64_t* class_labels, const float* anchors,
                                    const int* steps, int64_t rows, int A, int K, float loss_ratio, int cls_mode,
                                    float gamma, int box_mode, float box_weight, const double* stats,
                                    const float* g_loss, float* g_logits, float* g_bbox, void* stream) {
    const LossArgs a = {cls_logits, bbox_preds, bbox_offset, bbox_mask, class_labels, anchors, steps, rows, A, K,
                        loss_ratio, cls_mode, gamma, box_mode, box_weight};
    if (int rc = ext_check("snn_det_loss_ext_bwd", a)) return rc;
    SNN_REQUIRE(stats && g_loss && g_logits && g_bbox, "snn_det_loss_ext_bwd: null pointer");
    SNN_REQUIRE(aligned(16, {g_bbox}), "snn_det_loss_ext_bwd: g_bbox must be 16-byte aligned");
    return launch_bwd("snn_det_loss_ext_bwd", a, stats, g_loss, g_logits, g_bbox, stream);
}
