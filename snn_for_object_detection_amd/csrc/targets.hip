// Training targets on the device: the step after the network, before the loss (det_loss.hip).
//
//   snn_roi_assign : anchor <-> ground-truth assignment + offset / mask / class targets of one batch
//                    (utils/roi.py:18-109, utils/box.py:31-69) - one block per sample instead of ~150 tiny tensor
//                    launches per sample and a Python loop over the ground-truth rows;
//   snn_label_steps, snn_gather_steps_*, snn_roi_assign_steps : the same for every labelled timestep of a sequence.
//
// Arithmetic follows the reference expression by expression in fp32 (-ffp-contract=off), so the assignment (an
// integer result) is the reference's: first maximum wins in the per-anchor max and in the global argmax, padding rows
// (-1) of the label tensor take part in the greedy phase exactly as they do upstream (SURVEY a-11).
#include "snn_common.h"

namespace {

constexpr int kRoiThreads = 1024;

struct ArgMax {
    float v;
    int idx;
};
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {  // larger value; on ties the smaller flat index
    return (b.v > a.v || (b.v == a.v && b.idx < a.idx)) ? b : a;
}

// box_iou (utils/box.py:31-59) of one anchor and one ground-truth box
__device__ __forceinline__ float iou_pair(const float4 p, const float* __restrict__ q) {
    const float area1 = (p.z - p.x) * (p.w - p.y);
    const float area2 = (q[2] - q[0]) * (q[3] - q[1]);
    const float lx = fmaxf(p.x, q[0]), ly = fmaxf(p.y, q[1]);
    const float rx = fminf(p.z, q[2]), ry = fminf(p.w, q[3]);
    const float ow = fmaxf(rx - lx, 0.0f), oh = fmaxf(ry - ly, 0.0f);
    const float overlap = ow * oh;
    return overlap / (area1 + area2 - overlap);
}

// Targets of one anchor (roi.py:41-58, box.py:62-69): class = label + 1, offsets of the assigned box, all times the mask.
// g: the assigned label row or -1; gt: that row's (class, x1, y1, x2, y2), read only when g >= 0.
__device__ __forceinline__ void write_target_row(const float* __restrict__ anchors, int a, int g, const float* gt,
                                                 float* __restrict__ offset, float* __restrict__ mask,
                                                 int64_t* __restrict__ cls, int64_t row) {
    const float m = g >= 0 ? 1.0f : 0.0f;
    const float bx1 = g >= 0 ? gt[1] : 0.f, by1 = g >= 0 ? gt[2] : 0.f;
    const float bx2 = g >= 0 ? gt[3] : 0.f, by2 = g >= 0 ? gt[4] : 0.f;
    const float4 anc = *reinterpret_cast<const float4*>(anchors + (int64_t)a * 4);
    const float acx = (anc.x + anc.z) / 2, acy = (anc.y + anc.w) / 2, aw = anc.z - anc.x, ah = anc.w - anc.y;
    const float tcx = (bx1 + bx2) / 2, tcy = (by1 + by2) / 2, tw = bx2 - bx1, th = by2 - by1;
    float4 o;
    o.x = (10 * (tcx - acx) / aw) * m;
    o.y = (10 * (tcy - acy) / ah) * m;
    o.z = (5 * logf(1e-6f + tw / aw)) * m;
    o.w = (5 * logf(1e-6f + th / ah)) * m;
    *reinterpret_cast<float4*>(offset + row * 4) = o;
    *reinterpret_cast<float4*>(mask + row * 4) = make_float4(m, m, m, m);
    cls[row] = g >= 0 ? (int64_t)gt[0] + 1 : 0;
}

// The assignment of ONE sample: N label rows [N][5] at lab, the sample's IoU matrix iou [A][N] and map amap [A], targets
// written to the rows row0 .. row0 + A of offset / mask / cls.  Shared by k_roi_assign (a sample of the batch) and
// k_roi_assign_steps (a labelled frame of a sample, over the rows that take part): one body, the same roundings.
__device__ __forceinline__ void roi_assign_sample(const float* __restrict__ anchors, const float* lab, int A, int N,
                                                  float thr, float* __restrict__ iou, int* __restrict__ amap,
                                                  float* __restrict__ offset, float* __restrict__ mask,
                                                  int64_t* __restrict__ cls, int64_t row0) {
    __shared__ ArgMax red[kRoiThreads / 64];
    __shared__ ArgMax winner;
    const int tid = threadIdx.x;
    // ---- IoU matrix; an anchor takes the ground truth of highest IoU when that reaches the threshold (roi.py:78-93)
    for (int a = tid; a < A; a += kRoiThreads) {
        const float4 anc = *reinterpret_cast<const float4*>(anchors + (int64_t)a * 4);
        float best = 0.f;
        int arg = 0;
        for (int j = 0; j < N; ++j) {
            const float v = iou_pair(anc, lab + j * 5 + 1);
            iou[(int64_t)a * N + j] = v;
            if (j == 0 || v > best) {  // first maximum wins, as torch.max(dim=1)
                best = v;
                arg = j;
            }
        }
        amap[a] = best >= thr ? arg : -1;
    }
    __syncthreads();
    // ---- every ground-truth ROW claims the globally best remaining anchor (roi.py:95-108), padding rows included
    const int total = A * N;
    for (int round = 0; round < N; ++round) {
        ArgMax m = {-INFINITY, 0x7fffffff};
        for (int i = tid; i < total; i += kRoiThreads) {
            const float v = iou[i];
            if (v > m.v) m = {v, i};   // strictly greater: the first (lowest) index of this thread's maxima stays
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ArgMax other = {__shfl_xor(m.v, o), __shfl_xor(m.idx, o)};
            m = better(m, other);
        }
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            ArgMax w = red[0];
            for (int k = 1; k < kRoiThreads / 64; ++k) w = better(w, red[k]);
            if (w.idx == 0x7fffffff) w.idx = 0;   // every entry NaN / -inf: torch.argmax returns a valid index too
            winner = w;
        }
        __syncthreads();
        const int box_idx = winner.idx % N;
        // float division + truncation, as the reference: once A * N > 2^24 (float)idx rounds, and the quotient differs
        // from idx / N for some indices - those are the reference's assignments and are kept.  Rounded up it can reach
        // A for an index in the last anchor's row, where upstream raises IndexError: that one is held inside the
        // sample's amap / iou rows (the last anchor) instead of writing behind them.
        int anc_idx = (int)((float)winner.idx / (float)N);
        if (anc_idx > A - 1) anc_idx = A - 1;
        if (tid == 0) amap[anc_idx] = box_idx;
        for (int a = tid; a < A; a += kRoiThreads) iou[(int64_t)a * N + box_idx] = -1.0f;
        for (int j = tid; j < N; j += kRoiThreads) iou[(int64_t)anc_idx * N + j] = -1.0f;
        __syncthreads();
    }
    // ---- targets
    for (int a = tid; a < A; a += kRoiThreads) {
        const int g = amap[a];
        write_target_row(anchors, a, g, lab + (g >= 0 ? g : 0) * 5, offset, mask, cls, row0 + a);
    }
}

__global__ __launch_bounds__(kRoiThreads) void k_roi_assign(const float* __restrict__ anchors,
                                                            const float* __restrict__ labels, int A, int N, float thr,
                                                            float* __restrict__ iou_ws, int* __restrict__ amap_ws,
                                                            float* __restrict__ offset, float* __restrict__ mask,
                                                            int64_t* __restrict__ cls) {
    const int b = blockIdx.x;
    roi_assign_sample(anchors, labels + (int64_t)b * N * 5, A, N, thr, iou_ws + (int64_t)b * A * N,
                      amap_ws + (int64_t)b * A, offset, mask, cls, (int64_t)b * A);
}

// Step of the cut sequence a six-column label row (ts, class, x1, y1, x2, y2) belongs to, -1 when it is a padding row
// (class < 0) or falls outside [0, T).  ts is integer valued, so the fp32 difference is exact.
__device__ __forceinline__ int label_row_step(const float* __restrict__ row, int t0, int T) {
    const float r = row[0] - (float)t0;
    return (row[1] >= 0.f && r >= 0.f && r < (float)T) ? (int)r : -1;
}

// One block per sample: the latest K distinct steps of its real rows, ascending, into steps[0 ..][b]; -1 behind them.
__global__ __launch_bounds__(64) void k_label_steps(const float* __restrict__ labels, int B, int N, int T, int K, int t0,
                                                    int* __restrict__ steps) {
    __shared__ int found[kMaxLabelSteps];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* lab = labels + (int64_t)b * N * 6;
    int bound = T, count = 0;
    for (; count < K; ++count) {   // the largest step below the one found before; uniform over the wave
        int best = -1;
        for (int j = lane; j < N; j += 64) {
            const int s = label_row_step(lab + j * 6, t0, T);
            if (s < bound && s > best) best = s;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
        if (best < 0) break;
        if (lane == 0) found[count] = best;
        bound = best;
    }
    __syncthreads();
    if (lane < K) steps[lane * B + b] = lane < count ? found[count - 1 - lane] : -1;
}

// One block per slot (k, b) = blockIdx.x.  The rows of sample b that take part - real rows of step steps[k][b] and
// padding rows, in their order - are packed into the slot's [n][5] label tensor, then the assignment is the sample's.
__global__ __launch_bounds__(kRoiThreads) void k_roi_assign_steps(const float* __restrict__ anchors,
                                                                  const float* __restrict__ labels6,
                                                                  const int* __restrict__ steps, int B, int A, int N,
                                                                  int t0, float thr, float* iou_ws, int* amap_ws,
                                                                  float* lab_ws, float* __restrict__ offset,
                                                                  float* __restrict__ mask, int64_t* __restrict__ cls) {
    __shared__ int n_rows;
    const int slot = blockIdx.x, b = slot % B, tid = threadIdx.x;
    const int s = steps[slot];
    const int64_t row0 = (int64_t)slot * A;
    if (s < 0) {   // an empty slot: zero targets, nothing else
        for (int a = tid; a < A; a += kRoiThreads) {
            *reinterpret_cast<float4*>(offset + (row0 + a) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(mask + (row0 + a) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            cls[row0 + a] = 0;
        }
        return;
    }
    float* lab = lab_ws + (int64_t)slot * N * 5;
    if (tid == 0) {
        const float* src = labels6 + (int64_t)b * N * 6;
        int n = 0;
        for (int j = 0; j < N; ++j) {
            const float* row = src + j * 6;
            if (row[1] < 0.f || row[0] - (float)t0 == (float)s) {
                for (int c = 0; c < 5; ++c) lab[n * 5 + c] = row[1 + c];
                ++n;
            }
        }
        n_rows = n;
    }
    __threadfence_block();
    __syncthreads();
    roi_assign_sample(anchors, lab, A, n_rows, thr, iou_ws + (int64_t)slot * A * N, amap_ws + (int64_t)slot * A, offset,
                      mask, cls, row0);
}

// ------------------------------------------------------------------------------------------ labelled-frame gather
// Channels-last frames [T][B][M pixels][C] with pixel strides ld >= C.  An element is one channel (kVec: one channel
// quad) of one pixel; Cq = elements per pixel.  A step outside [0, T) is an empty slot.
constexpr int kGatherThreads = 256;

template <bool kVec> struct GatherElem { using type = float; };
template <> struct GatherElem<true> { using type = float4; };
__device__ __forceinline__ float zero_of(float) { return 0.f; }
__device__ __forceinline__ float4 zero_of(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float sum_of(float a, float b) { return a + b; }
__device__ __forceinline__ float4 sum_of(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// dst[k][b] = src[steps[k][b]][b]; zeros for an empty slot
template <bool kVec>
__global__ __launch_bounds__(kGatherThreads) void k_gather_steps_fwd(const float* __restrict__ src, int64_t ld_src,
                                                                     const int* __restrict__ steps,
                                                                     float* __restrict__ dst, int64_t ld_dst, int T,
                                                                     int B, int64_t M, int Cq, int64_t total) {
    using E = typename GatherElem<kVec>::type;
    constexpr int w = kVec ? 4 : 1;
    for (int64_t i = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kGatherThreads) {
        const int c = (int)(i % Cq);
        const int64_t pix = i / Cq, m = pix % M, slot = pix / M;
        const int b = (int)(slot % B), s = steps[slot];
        E v = zero_of(E());
        if (s >= 0 && s < T) v = *reinterpret_cast<const E*>(src + (((int64_t)s * B + b) * M + m) * ld_src + c * w);
        *reinterpret_cast<E*>(dst + (slot * M + m) * ld_dst + c * w) = v;
    }
}

// g_src[t][b] = sum over the slots k with steps[k][b] == t of g_dst[k][b], in slot order; zeros where no slot selects it
template <bool kVec>
__global__ __launch_bounds__(kGatherThreads) void k_gather_steps_bwd(const float* __restrict__ g_dst, int64_t ld_dst,
                                                                     const int* __restrict__ steps,
                                                                     float* __restrict__ g_src, int64_t ld_src, int B,
                                                                     int K, int64_t M, int Cq, int64_t total) {
    using E = typename GatherElem<kVec>::type;
    constexpr int w = kVec ? 4 : 1;
    for (int64_t i = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kGatherThreads) {
        const int c = (int)(i % Cq);
        const int64_t pix = i / Cq, m = pix % M, frame = pix / M;
        const int b = (int)(frame % B), t = (int)(frame / B);
        E acc = zero_of(E());
        for (int k = 0; k < K; ++k)
            if (steps[k * B + b] == t)
                acc = sum_of(acc, *reinterpret_cast<const E*>(g_dst + (((int64_t)k * B + b) * M + m) * ld_dst + c * w));
        *reinterpret_cast<E*>(g_src + (frame * M + m) * ld_src + c * w) = acc;
    }
}

static int gather_blocks(int64_t total) {
    int64_t b = snn_ceil_div(total, (int64_t)kGatherThreads);
    const int64_t cap = (int64_t)snn_num_cu() * 8;
    if (b > cap) b = cap;
    return b < 1 ? 1 : (int)b;
}

// ------------------------------------------------------------------------------------------ task-aligned assignment
// DESIGN section 5 "Anchor assignment".  Three launches per call, all static-shaped:
//   k_tal_prepare : one thread per (slot, anchor) - the decoded predicted box (corners) and the row maximum / sum of the
//                   softmax of its logits, to the workspace;
//   k_tal_select  : one block per (slot, label row) - topk rounds of a block arg-max over the row's candidates, each
//                   round taking the best metric that comes after the previous winner in (metric descending, anchor
//                   ascending) order; the first round computes the metrics and keeps them in LDS for the others;
//   k_tal_resolve : one block per slot - conflicts row by row (the larger overlap keeps the anchor, the lower row on
//                   ties), the fall-back rounds in row order, the targets.
// A label row is (class, x1, y1, x2, y2) at row + (stride - 5); stride 6 puts the timestep in front of it.
constexpr int kTalThreads = 256;
constexpr int kTalSelectThreads = 1024;   // the rounds are latency bound: 14 anchors per thread at the GEN1 count, not 53
constexpr int kTalMaxTopk = 64;
constexpr int kTalCache = 14336;   // metrics of one row kept in LDS between the rounds (56 KB); anchors behind it are recomputed
constexpr float kTalExpClamp = 4.135166556742356f;   // log(1000 / 16), as decode_box of det_loss.hip
constexpr float kTalIouEps = 1e-7f;
constexpr int kNoIndex = 0x7fffffff;

struct TalShape {
    int B, A, N, C, stride, t0, topk;
};

// the row takes part in slot step s (s ignored for five-column rows): a real class the logits have a column for, a box
// of positive area and, with timesteps, the slot's own step
__device__ __forceinline__ bool tal_row_takes_part(const float* __restrict__ row, const TalShape& sh, int s) {
    const float* r = row + (sh.stride - 5);
    if (!(r[0] >= 0.f && r[0] + 1.f < (float)sh.C && r[3] > r[1] && r[4] > r[2])) return false;
    return sh.stride == 5 || row[0] - (float)sh.t0 == (float)s;
}

// I / (U + eps) of the decoded prediction p and the box q = (x1, y1, x2, y2); what is not > 0 (NaN included) is 0
__device__ __forceinline__ float tal_overlap(const float4 p, const float* __restrict__ q) {
    const float ap = (p.z - p.x) * (p.w - p.y), ag = (q[2] - q[0]) * (q[3] - q[1]);
    const float iw = fmaxf(fminf(p.z, q[2]) - fmaxf(p.x, q[0]), 0.f), ih = fmaxf(fminf(p.w, q[3]) - fmaxf(p.y, q[1]), 0.f);
    const float inter = iw * ih;
    const float u = inter / ((ap + ag - inter) + kTalIouEps);
    return u > 0.f ? u : 0.f;
}

__global__ __launch_bounds__(kTalThreads) void k_tal_prepare(const float* __restrict__ anchors,
                                                             const float* __restrict__ cls_logits,
                                                             const float* __restrict__ bbox_preds, int A, int C,
                                                             int64_t total, float4* __restrict__ pbox,
                                                             float2* __restrict__ smax) {
    for (int64_t i = (int64_t)blockIdx.x * kTalThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kTalThreads) {
        const float4 anc = *reinterpret_cast<const float4*>(anchors + (i % A) * 4);
        const float4 o = *reinterpret_cast<const float4*>(bbox_preds + i * 4);
        // offset_inverse (utils/box.py:72-79) with the exponent argument clamped above, as decode_box of det_loss.hip
        const float cxa = (anc.x + anc.z) / 2, cya = (anc.y + anc.w) / 2, wa = anc.z - anc.x, ha = anc.w - anc.y;
        const float aw = o.z / 5, ah = o.w / 5;
        const float cx = o.x * wa / 10 + cxa, cy = o.y * ha / 10 + cya;
        const float w = expf(aw <= kTalExpClamp ? aw : kTalExpClamp) * wa;
        const float h = expf(ah <= kTalExpClamp ? ah : kTalExpClamp) * ha;
        pbox[i] = make_float4(cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h);
        const float* x = cls_logits + i * C;
        float mx = x[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, x[k]);
        float se = 0.f;
        for (int k = 0; k < C; ++k) se += expf(x[k] - mx);
        smax[i] = make_float2(mx, se);
    }
}

// arg-max over the block under better(): every thread gets the winner.  red: one entry per wave and one more.
template <int kThreads>
__device__ __forceinline__ ArgMax block_argmax(ArgMax m, ArgMax* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax other = {__shfl_xor(m.v, o), __shfl_xor(m.idx, o)};
        m = better(m, other);
    }
    __syncthreads();   // the previous winner has been read by everyone
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        ArgMax w = red[0];
        for (int k = 1; k < kThreads / 64; ++k) w = better(w, red[k]);
        red[kThreads / 64] = w;
    }
    __syncthreads();
    return red[kThreads / 64];
}

__global__ __launch_bounds__(kTalSelectThreads) void k_tal_select(const float* __restrict__ anchors,
                                                            const float* __restrict__ labels,
                                                            const int* __restrict__ steps,
                                                            const float* __restrict__ cls_logits,
                                                            const float4* __restrict__ pbox,
                                                            const float2* __restrict__ smax, TalShape sh, float alpha,
                                                            float beta, int* __restrict__ sel) {
    __shared__ ArgMax red[kTalSelectThreads / 64 + 1];
    __shared__ float tcache[kTalCache];
    const int slot = blockIdx.x / sh.N, j = blockIdx.x % sh.N, b = slot % sh.B, tid = threadIdx.x;
    const int A = sh.A, C = sh.C;
    const float* row = labels + ((int64_t)b * sh.N + j) * sh.stride;
    int* out = sel + (int64_t)blockIdx.x * sh.topk;
    const int s = steps ? steps[slot] : 0;
    if (s < 0 || !tal_row_takes_part(row, sh, s)) {   // uniform over the block
        if (tid < sh.topk) out[tid] = -1;
        return;
    }
    const float* q = row + (sh.stride - 5);
    const int col = (int)q[0] + 1;   // 1 .. C - 1: checked by tal_row_takes_part
    const float x1 = q[1], y1 = q[2], x2 = q[3], y2 = q[4];
    const int64_t base = (int64_t)slot * A;
    // the metric of anchor a for this row, -1 when a is no candidate
    auto metric = [&](int a) -> float {
        const float4 anc = *reinterpret_cast<const float4*>(anchors + (int64_t)a * 4);
        const float acx = (anc.x + anc.z) / 2, acy = (anc.y + anc.w) / 2;
        if (!(acx > x1 && acx < x2 && acy > y1 && acy < y2)) return -1.0f;   // candidates: centre strictly inside
        const float2 ms = smax[base + a];
        float p = expf(cls_logits[(base + a) * C + col] - ms.x) / ms.y;
        if (!(p > 0.f)) p = 0.f;
        const float u = tal_overlap(pbox[base + a], q + 1);
        const float t = powf(p, alpha) * powf(u, beta);
        return t > 0.f ? t : 0.f;
    };
    ArgMax prev = {INFINITY, -1};
    int r = 0;
    for (; r < sh.topk; ++r) {
        ArgMax m = {-1.0f, kNoIndex};
        for (int a = tid; a < A; a += kTalSelectThreads) {
            // round 0 computes every metric and keeps those of the first kTalCache anchors in LDS; a thread reads back
            // only what it wrote itself (the same a), so the cache needs no barrier
            float t;
            if (r == 0 || a >= kTalCache) {
                t = metric(a);
                if (r == 0 && a < kTalCache) tcache[a] = t;
            } else {
                t = tcache[a];
            }
            if (t < 0.f) continue;
            // after the previous winner in (metric descending, anchor ascending) order
            if (!(t < prev.v || (t == prev.v && a > prev.idx))) continue;
            if (t > m.v) m = {t, a};   // a ascends inside a thread: its first maximum stays
        }
        const ArgMax w = block_argmax<kTalSelectThreads>(m, red);
        if (w.idx == kNoIndex) break;   // fewer candidates than topk
        if (tid == 0) out[r] = w.idx;
        prev = w;
    }
    if (tid >= r && tid < sh.topk) out[tid] = -1;
}

__global__ __launch_bounds__(kRoiThreads) void k_tal_resolve(const float* __restrict__ anchors,
                                                             const float* __restrict__ labels,
                                                             const int* __restrict__ steps,
                                                             const float4* __restrict__ pbox,
                                                             const int* __restrict__ sel, TalShape sh, int* amap_ws,
                                                             float* __restrict__ offset, float* __restrict__ mask,
                                                             int64_t* __restrict__ cls, int* __restrict__ assigned_row) {
    __shared__ ArgMax red[kRoiThreads / 64 + 1];
    const int slot = blockIdx.x, b = slot % sh.B, tid = threadIdx.x;
    const int A = sh.A, N = sh.N, off = sh.stride - 5;
    const int64_t row0 = (int64_t)slot * A;
    const int s = steps ? steps[slot] : 0;
    if (s < 0) {   // an empty slot: zero targets, nothing else
        for (int a = tid; a < A; a += kRoiThreads) {
            *reinterpret_cast<float4*>(offset + (row0 + a) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(mask + (row0 + a) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            cls[row0 + a] = 0;
            if (assigned_row) assigned_row[row0 + a] = -1;
        }
        return;
    }
    const float* lab = labels + (int64_t)b * N * sh.stride;
    int* amap = amap_ws + row0;
    for (int a = tid; a < A; a += kRoiThreads) amap[a] = -1;
    __syncthreads();
    // ---- conflicts, row by row: the anchors one row selected are distinct, so a round has no two writers of one entry
    for (int j = 0; j < N; ++j) {
        if (!tal_row_takes_part(lab + j * sh.stride, sh, s)) continue;   // uniform over the block
        if (tid < sh.topk) {
            const int a = sel[((int64_t)slot * N + j) * sh.topk + tid];
            if (a >= 0) {
                const int cur = amap[a];
                const float4 p = pbox[row0 + a];
                if (cur < 0 || tal_overlap(p, lab + j * sh.stride + off + 1) > tal_overlap(p, lab + cur * sh.stride + off + 1))
                    amap[a] = j;
            }
        }
        __syncthreads();
    }
    // ---- fall-back, in row order: a row left without an anchor claims the unassigned anchor of highest IoU
    for (int j = 0; j < N; ++j) {
        if (!tal_row_takes_part(lab + j * sh.stride, sh, s)) continue;
        int has = 0;
        if (tid < sh.topk) {
            const int a = sel[((int64_t)slot * N + j) * sh.topk + tid];
            has = a >= 0 && amap[a] == j;
        }
        if (__syncthreads_or(has)) continue;
        ArgMax m = {-INFINITY, kNoIndex};
        for (int a = tid; a < A; a += kRoiThreads) {
            if (amap[a] >= 0) continue;
            const float v = iou_pair(*reinterpret_cast<const float4*>(anchors + (int64_t)a * 4), lab + j * sh.stride + off + 1);
            if (v > m.v) m = {v, a};   // first maximum wins
        }
        const ArgMax w = block_argmax<kRoiThreads>(m, red);
        if (tid == 0 && w.idx != kNoIndex) amap[w.idx] = j;
        __syncthreads();
    }
    // ---- targets
    for (int a = tid; a < A; a += kRoiThreads) {
        const int g = amap[a];
        write_target_row(anchors, a, g, lab + (g >= 0 ? g : 0) * sh.stride + off, offset, mask, cls, row0 + a);
        if (assigned_row) assigned_row[row0 + a] = g;
    }
}

}  // namespace

extern "C" size_t snn_roi_workspace_size(int B, int A, int N) {  // bytes: IoU matrix + assignment map per sample
    return (size_t)B * A * ((size_t)N * sizeof(float) + sizeof(int));
}

extern "C" int snn_roi_assign(const float* anchors, const float* labels, int B, int A, int N, float iou_threshold,
                              void* workspace, float* bbox_offset, float* bbox_mask, int64_t* class_labels,
                              void* stream) {
    SNN_REQUIRE(anchors && labels && workspace && bbox_offset && bbox_mask && class_labels, "snn_roi_assign: null pointer");
    // flat IoU indices are int, and the strided argmax loop steps kRoiThreads past the last one before it stops
    SNN_REQUIRE(B > 0 && A > 0 && N > 0 && (int64_t)A * N < 0x7fffffffLL - kRoiThreads, "snn_roi_assign: bad shape");
    SNN_REQUIRE(aligned(16, {anchors, bbox_offset, bbox_mask, workspace}),
                "snn_roi_assign: buffers must be 16-byte aligned");
    float* iou = static_cast<float*>(workspace);
    int* amap = reinterpret_cast<int*>(iou + (size_t)B * A * N);
    hipLaunchKernelGGL(k_roi_assign, dim3((unsigned)B), dim3(kRoiThreads), 0, (hipStream_t)stream, anchors, labels, A, N,
                       iou_threshold, iou, amap, bbox_offset, bbox_mask, class_labels);
    SNN_CHECK_LAUNCH("snn_roi_assign");
    return 0;
}

// ------------------------------------------------------------------------------------------ every labelled timestep
extern "C" int snn_label_steps(const float* labels, int B, int N, int T, int K, int t0, int* steps, void* stream) {
    SNN_REQUIRE(labels && steps, "snn_label_steps: null pointer");
    SNN_REQUIRE(B > 0 && N > 0 && T > 0 && t0 >= 0, "snn_label_steps: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps && K <= T, "snn_label_steps: K must be in 1 .. min(%d, T)", kMaxLabelSteps);
    hipLaunchKernelGGL(k_label_steps, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, labels, B, N, T, K, t0, steps);
    SNN_CHECK_LAUNCH("snn_label_steps");
    return 0;
}

static bool gather_vec(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int C) {
    return C % 4 == 0 && ld_a % 4 == 0 && ld_b % 4 == 0 && aligned(16, {a, b});
}

extern "C" int snn_gather_steps_fwd(const float* src, int64_t ld_src, const int* steps, float* dst, int64_t ld_dst, int T,
                                    int B, int K, int64_t M, int C, void* stream) {
    SNN_REQUIRE(src && steps && dst, "snn_gather_steps_fwd: null pointer");
    SNN_REQUIRE(T > 0 && B > 0 && M > 0 && C > 0 && ld_src >= C && ld_dst >= C, "snn_gather_steps_fwd: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps && K <= T, "snn_gather_steps_fwd: K must be in 1 .. min(%d, T)",
                kMaxLabelSteps);
    const bool vec = gather_vec(src, ld_src, dst, ld_dst, C);
    const int Cq = vec ? C / 4 : C;
    const int64_t total = (int64_t)K * B * M * Cq;
    if (vec)
        hipLaunchKernelGGL(k_gather_steps_fwd<true>, dim3((unsigned)gather_blocks(total)), dim3(kGatherThreads), 0,
                           (hipStream_t)stream, src, ld_src, steps, dst, ld_dst, T, B, M, Cq, total);
    else
        hipLaunchKernelGGL(k_gather_steps_fwd<false>, dim3((unsigned)gather_blocks(total)), dim3(kGatherThreads), 0,
                           (hipStream_t)stream, src, ld_src, steps, dst, ld_dst, T, B, M, Cq, total);
    SNN_CHECK_LAUNCH("snn_gather_steps_fwd");
    return 0;
}

extern "C" int snn_gather_steps_bwd(const float* g_dst, int64_t ld_dst, const int* steps, float* g_src, int64_t ld_src,
                                    int T, int B, int K, int64_t M, int C, void* stream) {
    SNN_REQUIRE(g_dst && steps && g_src, "snn_gather_steps_bwd: null pointer");
    SNN_REQUIRE(T > 0 && B > 0 && M > 0 && C > 0 && ld_src >= C && ld_dst >= C, "snn_gather_steps_bwd: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps && K <= T, "snn_gather_steps_bwd: K must be in 1 .. min(%d, T)",
                kMaxLabelSteps);
    const bool vec = gather_vec(g_dst, ld_dst, g_src, ld_src, C);
    const int Cq = vec ? C / 4 : C;
    const int64_t total = (int64_t)T * B * M * Cq;
    if (vec)
        hipLaunchKernelGGL(k_gather_steps_bwd<true>, dim3((unsigned)gather_blocks(total)), dim3(kGatherThreads), 0,
                           (hipStream_t)stream, g_dst, ld_dst, steps, g_src, ld_src, B, K, M, Cq, total);
    else
        hipLaunchKernelGGL(k_gather_steps_bwd<false>, dim3((unsigned)gather_blocks(total)), dim3(kGatherThreads), 0,
                           (hipStream_t)stream, g_dst, ld_dst, steps, g_src, ld_src, B, K, M, Cq, total);
    SNN_CHECK_LAUNCH("snn_gather_steps_bwd");
    return 0;
}

// bytes: per slot the IoU matrix, the assignment map and the packed [N][5] rows that take part
extern "C" size_t snn_roi_steps_workspace_size(int K, int B, int A, int N) {
    return (size_t)K * B * ((size_t)A * ((size_t)N * sizeof(float) + sizeof(int)) + (size_t)N * 5 * sizeof(float));
}

extern "C" int snn_roi_assign_steps(const float* anchors, const float* labels, const int* steps, int K, int B, int A,
                                    int N, int t0, float iou_threshold, void* workspace, float* bbox_offset,
                                    float* bbox_mask, int64_t* class_labels, void* stream) {
    SNN_REQUIRE(anchors && labels && steps && workspace && bbox_offset && bbox_mask && class_labels,
                "snn_roi_assign_steps: null pointer");
    SNN_REQUIRE(B > 0 && A > 0 && N > 0 && t0 >= 0 && (int64_t)A * N < 0x7fffffffLL - kRoiThreads,
                "snn_roi_assign_steps: bad shape");
    SNN_REQUIRE(K >= 1 && K <= kMaxLabelSteps, "snn_roi_assign_steps: K must be in 1 .. %d", kMaxLabelSteps);
    SNN_REQUIRE(aligned(16, {anchors, bbox_offset, bbox_mask, workspace}),
                "snn_roi_assign_steps: buffers must be 16-byte aligned");
    const size_t slots = (size_t)K * B;
    float* iou = static_cast<float*>(workspace);
    int* amap = reinterpret_cast<int*>(iou + slots * A * N);
    float* lab = reinterpret_cast<float*>(amap + slots * A);
    hipLaunchKernelGGL(k_roi_assign_steps, dim3((unsigned)slots), dim3(kRoiThreads), 0, (hipStream_t)stream, anchors,
                       labels, steps, B, A, N, t0, iou_threshold, iou, amap, lab, bbox_offset, bbox_mask, class_labels);
    SNN_CHECK_LAUNCH("snn_roi_assign_steps");
    return 0;
}

// ------------------------------------------------------------------------------------------ task-aligned assignment
// bytes, per slot: decoded boxes [A] float4, softmax (maximum, sum) [A] float2, assignment map [A] int, selected anchors
// [N][topk] int - in this order, so every part stays aligned when the workspace is
extern "C" size_t snn_tal_workspace_size(int S, int A, int N, int topk) {
    if (S <= 0 || A <= 0 || N <= 0 || topk <= 0) return 0;
    return (size_t)S * ((size_t)A * (sizeof(float4) + sizeof(float2) + sizeof(int)) + (size_t)N * topk * sizeof(int));
}

extern "C" int snn_tal_assign(const float* anchors, const float* labels, const int* steps, const float* cls_logits,
                              const float* bbox_preds, int K, int B, int A, int N, int C, int t0, int topk, float alpha,
                              float beta, void* workspace, float* bbox_offset, float* bbox_mask, int64_t* class_labels,
                              int* assigned_row, void* stream) {
    SNN_REQUIRE(anchors && labels && cls_logits && bbox_preds && workspace && bbox_offset && bbox_mask && class_labels,
                "snn_tal_assign: null pointer");
    SNN_REQUIRE(B > 0 && A > 0 && N > 0 && t0 >= 0 && (int64_t)A * N < 0x7fffffffLL - kRoiThreads,
                "snn_tal_assign: bad shape");
    SNN_REQUIRE(steps ? (K >= 1 && K <= kMaxLabelSteps) : K == 1,
                "snn_tal_assign: K must be in 1 .. %d with steps, 1 without", kMaxLabelSteps);
    SNN_REQUIRE((int64_t)K * B * N < 0x7fffffffLL, "snn_tal_assign: bad shape");
    SNN_REQUIRE(topk >= 1 && topk <= kTalMaxTopk, "snn_tal_assign: topk must be in 1 .. %d", kTalMaxTopk);
    SNN_REQUIRE(C >= 2 && C <= 64, "snn_tal_assign: C must be in 2 .. 64");
    SNN_REQUIRE(alpha >= 0.f && alpha <= 3.0e38f && beta >= 0.f && beta <= 3.0e38f,
                "snn_tal_assign: alpha and beta must be finite and >= 0");
    SNN_REQUIRE(aligned(16, {anchors, bbox_preds, bbox_offset, bbox_mask, workspace}),
                "snn_tal_assign: buffers must be 16-byte aligned");
    const size_t slots = (size_t)(steps ? K : 1) * B;
    float4* pbox = static_cast<float4*>(workspace);
    float2* smax = reinterpret_cast<float2*>(pbox + slots * A);
    int* amap = reinterpret_cast<int*>(smax + slots * A);
    int* sel = amap + slots * A;
    const TalShape sh = {B, A, N, C, steps ? 6 : 5, t0, topk};
    const int64_t total = (int64_t)slots * A;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tal_prepare, dim3(snn_grid_for(total, kTalThreads)), dim3(kTalThreads), 0, st, anchors,
                       cls_logits, bbox_preds, A, C, total, pbox, smax);
    SNN_CHECK_LAUNCH("snn_tal_assign");
    hipLaunchKernelGGL(k_tal_select, dim3((unsigned)(slots * N)), dim3(kTalSelectThreads), 0, st, anchors, labels, steps,
                       cls_logits, pbox, smax, sh, alpha, beta, sel);
    SNN_CHECK_LAUNCH("snn_tal_assign");
    hipLaunchKernelGGL(k_tal_resolve, dim3((unsigned)slots), dim3(kRoiThreads), 0, st, anchors, labels, steps, pbox, sel,
                       sh, amap, bbox_offset, bbox_mask, class_labels, assigned_row);
    SNN_CHECK_LAUNCH("snn_tal_assign");
    return 0;
}
