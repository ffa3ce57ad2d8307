// COCO bounding-box mAP on the device: the metric the reference computes in validation_step / test_step through
// torchmetrics.detection.MeanAveragePrecision (models/soda.py:160-182, 283-321), i.e. COCOeval for bbox, area range
// "all", no crowd boxes.  The rules restated in metrics.py are followed expression by expression.
//
//   snn_map_match      : one block per (image, class): greedy matching of the class's top-`slots` detections against
//                        the image's ground truth of that class at every IoU threshold -> a fixed-shape record per
//                        (image, class, slot): score and a bit mask "matched at threshold t"; npig[class] += count
//   snn_map_accumulate : one block per (class, maxDet, IoU threshold) over the records of the whole evaluation sorted
//                        by score: cumulative tp / fp by block scans, fp64 precision / recall, interpolated precision at
//                        the recall thresholds; then one block reduces to map, map_50, map_75, mar_<maxDet>.
//
// IoU is pycocotools' bbIou on xywh boxes whose w / h were formed in fp32 (torchmetrics converts xyxy -> xywh on the
// fp32 tensors), evaluated in fp64; the build has -ffp-contract=off, so every value is bit-identical to the host's.
#include "snn_common.h"

namespace {

constexpr int kMapThreads = 256;
constexpr int kMapWaves = kMapThreads / 64;
constexpr int kMapMaxSlots = 1024;   // detections kept per (image, class): max(max_detection_thresholds)
constexpr int kMapMaxGt = 2048;      // ground-truth rows per image: 64 lanes x 32 "taken" bits of one register
constexpr int kMapMaxIou = 31;       // IoU thresholds: bits 0..30 of a slot's mask
constexpr int kMapMaxRec = 1024;     // recall thresholds (LDS table)
constexpr unsigned kSlotUsed = 1u << 31;

// pycocotools maskApi.c bbIou, one (detection, ground truth) pair; boxes are (x, y, w, h)
__device__ __forceinline__ double coco_iou(const float4 d, const float4 g) {
    const double xd = d.x, yd = d.y, wd = d.z, hd = d.w;
    const double xg = g.x, yg = g.y, wg = g.z, hg = g.w;
    const double iw = fmin(wd + xd, wg + xg) - fmax(xd, xg);
    if (iw <= 0.0) return 0.0;
    const double ih = fmin(hd + yd, hg + yg) - fmax(yd, yg);
    if (ih <= 0.0) return 0.0;
    const double inter = iw * ih;
    return inter / (wd * hd + wg * hg - inter);
}

// dets [B][A][6] (class, score, x1, y1, x2, y2); order [B][A]: row ids by (class ascending, score descending, row id
// ascending); the rows of class c are order[b][seg[b][c] .. seg[b][c+1]).  labels [B][G][5] (class, x1, y1, x2, y2).
__global__ __launch_bounds__(kMapThreads) void k_map_match(const float* __restrict__ dets, const float* __restrict__ labels,
                                                           const int* __restrict__ order, const int* __restrict__ seg,
                                                           int A, int G, int C, int S, const double* __restrict__ iou_thr,
                                                           int T, float* __restrict__ score, unsigned* __restrict__ mask,
                                                           int* __restrict__ npig) {
    __shared__ float4 dbox[kMapMaxSlots];
    __shared__ float4 gbox[kMapMaxGt];
    __shared__ unsigned smask[kMapMaxSlots];
    __shared__ int s_ng;
    const int c = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = seg[(int64_t)b * (C + 1) + c], hi = seg[(int64_t)b * (C + 1) + c + 1];
    const int nd = min(hi - lo, S);   // truncation to the top S happens BEFORE matching (COCOeval.computeIoU)
    const int64_t rec = ((int64_t)b * C + c) * S;
    for (int i = tid; i < S; i += kMapThreads) {
        float sc = -INFINITY;
        unsigned used = 0u;
        if (i < nd) {
            const float* r = dets + ((int64_t)b * A + order[(int64_t)b * A + lo + i]) * 6;
            sc = r[1];
            dbox[i] = make_float4(r[2], r[3], r[4] - r[2], r[5] - r[3]);
            used = kSlotUsed;
        }
        score[rec + i] = sc;
        smask[i] = used;
    }
    if (wave == 0) {  // the image's ground truth of class c, compacted in row order
        const float* lab = labels + (int64_t)b * G * 5;
        int n = 0;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            bool mine = false;
            if (g < G) {
                const float k = lab[(int64_t)g * 5];
                mine = k >= 0.0f && (int)k == c;
            }
            const unsigned long long bal = __ballot(mine);
            if (mine) {
                const float* r = lab + (int64_t)g * 5;
                gbox[n + __popcll(bal & ((1ull << lane) - 1ull))] = make_float4(r[1], r[2], r[3] - r[1], r[4] - r[2]);
            }
            n += __popcll(bal);
        }
        if (lane == 0) {
            s_ng = n;
            if (n) atomicAdd(npig + c, n);   // integer: the total does not depend on the order of the blocks
        }
    }
    __syncthreads();
    const int ng = s_ng;
    // one wave per IoU threshold; the sequential rule of COCOeval.evaluateImg: detections in score order, each takes
    // the still-free ground truth of largest IoU >= min(t, 1 - 1e-10), ties to the later ground-truth row
    for (int t = wave; t < T; t += kMapWaves) {
        const double thr = fmin(iou_thr[t], 1.0 - 1e-10);
        unsigned taken = 0u;   // bit j: ground truth lane + 64 j is matched at t
        for (int d = 0; d < nd; ++d) {
            const float4 db = dbox[d];
            double bv = 0.0;
            int bi = -1;
            for (int j = 0, g = lane; g < ng; ++j, g += 64) {
                if ((taken >> j) & 1u) continue;
                const double iou = coco_iou(db, gbox[g]);
                if (iou >= thr && (bi < 0 || iou >= bv)) {   // ascending g: equal IoU moves to the later row
                    bv = iou;
                    bi = g;
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {   // wave argmax of (IoU, row), the larger row on equal IoU
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (bi >= 0) {
                if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
                if (lane == 0) atomicOr(&smask[d], 1u << t);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < S; i += kMapThreads) mask[rec + i] = smask[i];
}

// One block per (class c, maxDet index mi, IoU threshold t).  order [C][N]: record positions (image * S + slot) of
// class c sorted by score descending, stably; mask [C][N] in position order.  Writes qsum = sum over the recall
// thresholds of the interpolated precision and recall = rc[-1] (both -1 for a class without ground truth).
//
// Interpolated precision q[r] = (reverse running max of pr)[searchsorted_left(rc, r)] is the max of pr over the records
// with rc >= r (rc is non-decreasing), and on records with the same tp count pr is largest at the true positive that
// reached it.  So each true positive k contributes pr_k to q[0 .. n_k) with n_k = #{r : r <= rc_k}: one LDS atomicMax
// into bucket n_k - 1 (pr >= 0, so its bit pattern orders like its value), then a running max from the right.
__global__ __launch_bounds__(kMapThreads) void k_map_accumulate(const int* __restrict__ order,
                                                                const unsigned* __restrict__ mask,
                                                                const int* __restrict__ npig, int N, int S,
                                                                const int* __restrict__ max_dets, int M,
                                                                const double* __restrict__ rec_thr, int R, int T,
                                                                double* __restrict__ qsum, double* __restrict__ recall) {
    __shared__ unsigned long long bucket[kMapMaxRec];
    __shared__ double rthr[kMapMaxRec];
    __shared__ unsigned long long wsum[kMapWaves];
    const int c = blockIdx.x, mi = blockIdx.y, t = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t out = ((int64_t)c * M + mi) * T + t;
    const int np = npig[c];
    if (np <= 0) {
        if (tid == 0) qsum[out] = recall[out] = -1.0;
        return;
    }
    const int md = max_dets[mi];
    for (int r = tid; r < R; r += kMapThreads) {
        bucket[r] = 0ull;
        rthr[r] = rec_thr[r];
    }
    __syncthreads();
    const int* ord = order + (int64_t)c * N;
    const unsigned* msk = mask + (int64_t)c * N;
    unsigned long long carry = 0ull;   // (tp << 32) | fp of the chunks before
    for (int base = 0; base < N; base += kMapThreads) {
        const int n = base + tid;
        unsigned long long v = 0ull;
        bool tp = false;
        if (n < N) {
            const int p = ord[n];
            const unsigned m = msk[p];
            if ((m & kSlotUsed) && p % S < md) {   // an image's first maxDet detections of the class
                tp = (m >> t) & 1u;
                v = tp ? (1ull << 32) : 1ull;
            }
        }
        unsigned long long x = v;   // inclusive scan of the packed (tp, fp) counts
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned long long pre = carry, tot = carry;
#pragma unroll
        for (int w = 0; w < kMapWaves; ++w) {
            if (w < wave) pre += wsum[w];
            tot += wsum[w];
        }
        __syncthreads();   // wsum is rewritten by the next chunk
        carry = tot;
        if (tp) {
            const unsigned long long cum = pre + x;
            const double tpc = (double)(cum >> 32), fpc = (double)(cum & 0xffffffffull);
            const double pr = tpc / (fpc + tpc + 2.220446049250313e-16);   // np.spacing(1) = 2^-52
            const double rc = tpc / (double)np;
            int l = 0, h = R;   // thresholds <= rc (the table is ascending)
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (rthr[mid] <= rc) l = mid + 1;
                else h = mid;
            }
            if (l > 0) atomicMax(&bucket[l - 1], (unsigned long long)__double_as_longlong(pr));
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0ull;
        double s = 0.0;
        for (int r = R - 1; r >= 0; --r) {
            run = max(run, bucket[r]);
            s += __longlong_as_double((long long)run);
        }
        qsum[out] = s;
        recall[out] = (double)(carry >> 32) / (double)np;
    }
}

__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kMapThreads / 2; s; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// out[0] map, out[1] map_50, out[2] map_75, out[3 + mi] mar at max_dets[mi]; means over the classes with ground truth
// in fp64 (fixed reduction tree), rounded once to fp32; -1 when nothing is valid
__global__ __launch_bounds__(kMapThreads) void k_map_summary(const double* __restrict__ qsum,
                                                             const double* __restrict__ recall,
                                                             const int* __restrict__ npig, int C, int M, int T, int R,
                                                             int t50, int t75, float* __restrict__ out) {
    __shared__ double red[kMapThreads];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int c = tid; c < C; c += kMapThreads) v += npig[c] > 0 ? 1.0 : 0.0;
    const double nv = block_sum(v, red);
    const int last = M - 1;
    for (int o = 0; o < 3 + M; ++o) {
        const int mi = o < 3 ? last : o - 3;
        const int t0 = o == 1 ? t50 : o == 2 ? t75 : 0;
        const int nt = o == 1 || o == 2 ? (t0 >= 0 ? 1 : 0) : T;
        const double* src = o < 3 ? qsum : recall;
        v = 0.0;
        for (int k = tid; k < C * nt; k += kMapThreads) {
            const int c = k / nt, t = t0 + k % nt;
            if (npig[c] > 0) v += src[((int64_t)c * M + mi) * T + t];
        }
        const double s = block_sum(v, red);
        if (tid == 0) {
            const double cnt = nv * nt * (o < 3 ? R : 1);
            out[o] = cnt > 0.0 ? (float)(s / cnt) : -1.0f;
        }
    }
}

}  // namespace

extern "C" int snn_map_match(const float* dets, const float* labels, const int* order, const int* seg, int B, int A,
                             int G, int num_classes, int slots, const double* iou_thresholds, int num_iou, float* score,
                             unsigned* match_mask, int* npig, void* stream) {
    SNN_REQUIRE(dets && labels && order && seg && iou_thresholds && score && match_mask && npig,
                "snn_map_match: null pointer");
    SNN_REQUIRE(B > 0 && B <= 65535 && A > 0 && G >= 0 && num_classes > 0, "snn_map_match: bad shape");
    SNN_REQUIRE(G <= kMapMaxGt, "snn_map_match: %d ground-truth rows per image exceed the limit of %d", G, kMapMaxGt);
    SNN_REQUIRE(slots > 0 && slots <= kMapMaxSlots, "snn_map_match: %d detection slots per class (the largest maxDet) "
                "outside 1..%d", slots, kMapMaxSlots);
    SNN_REQUIRE(num_iou > 0 && num_iou <= kMapMaxIou, "snn_map_match: %d IoU thresholds outside 1..%d", num_iou,
                kMapMaxIou);
    hipLaunchKernelGGL(k_map_match, dim3((unsigned)num_classes, (unsigned)B), dim3(kMapThreads), 0, (hipStream_t)stream,
                       dets, labels, order, seg, A, G, num_classes, slots, iou_thresholds, num_iou, score, match_mask,
                       npig);
    SNN_CHECK_LAUNCH("snn_map_match");
    return 0;
}

extern "C" size_t snn_map_workspace_size(int num_classes, int num_max_dets, int num_iou) {
    if (num_classes <= 0 || num_max_dets <= 0 || num_iou <= 0) return 0;
    return 2 * (size_t)num_classes * num_max_dets * num_iou * sizeof(double);
}

extern "C" int snn_map_accumulate(const int* order, const unsigned* match_mask, const int* npig, int num_classes,
                                  int records, int slots, const int* max_dets, int num_max_dets,
                                  const double* rec_thresholds, int num_rec, int num_iou, int t50, int t75,
                                  void* workspace, float* out, void* stream) {
    SNN_REQUIRE(order && match_mask && npig && max_dets && rec_thresholds && workspace && out,
                "snn_map_accumulate: null pointer");
    SNN_REQUIRE(num_classes > 0 && records >= 0 && slots > 0 && records % slots == 0,
                "snn_map_accumulate: bad shape");
    SNN_REQUIRE(num_max_dets > 0 && num_max_dets <= 65535, "snn_map_accumulate: bad maxDet count");
    SNN_REQUIRE(num_iou > 0 && num_iou <= kMapMaxIou, "snn_map_accumulate: %d IoU thresholds outside 1..%d", num_iou,
                kMapMaxIou);
    SNN_REQUIRE(num_rec > 0 && num_rec <= kMapMaxRec, "snn_map_accumulate: %d recall thresholds outside 1..%d",
                num_rec, kMapMaxRec);
    SNN_REQUIRE(t50 < num_iou && t75 < num_iou, "snn_map_accumulate: bad threshold index");
    double* qsum = static_cast<double*>(workspace);
    double* recall = qsum + (size_t)num_classes * num_max_dets * num_iou;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_map_accumulate, dim3((unsigned)num_classes, (unsigned)num_max_dets, (unsigned)num_iou),
                       dim3(kMapThreads), 0, st, order, match_mask, npig, records, slots, max_dets, num_max_dets,
                       rec_thresholds, num_rec, num_iou, qsum, recall);
    SNN_CHECK_LAUNCH("snn_map_accumulate");
    hipLaunchKernelGGL(k_map_summary, dim3(1), dim3(kMapThreads), 0, st, qsum, recall, npig, num_classes, num_max_dets,
                       num_iou, num_rec, t50, t75, out);
    SNN_CHECK_LAUNCH("snn_map_accumulate (summary)");
    return 0;
}
