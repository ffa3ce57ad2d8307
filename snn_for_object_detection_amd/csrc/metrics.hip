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
// Beside them, the COCO area ranges (small / medium / large on pixel areas), per-class AP / AR and a box-size filter:
//   snn_map_filter_rows      : one thread per row: the class key of every detection, the class column of the labels,
//                              both with the rows a minimum diagonal / side removes turned into padding
//   snn_map_match_areas      : k_map_match's block with 16 waves, one per (range, threshold): "all" as before, and
//                              per range once more with the ground truth outside it ignored (COCOeval's gtIg / dtIg)
//                              -> per slot and range a matched and an ignored mask; npig_area[range][class]
//   snn_map_accumulate_areas : the same scan with the range folded into the grid (tp / fp from the two masks); the
//                              summary block adds map_<range>, mar_<range> and the per-class AP / AR
// The "all" result of the new entry points is the old code path: the same masks and the same six values, bit for bit.
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

// wave argmax of (IoU, row), the larger row on equal IoU; every lane ends with the result (row -1: none)
__device__ __forceinline__ void wave_argmax(double& bv, int& bi) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) {
            bv = ov;
            bi = oi;
        }
    }
}

constexpr int kMapRanges = 3;   // small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10] (pixel areas, ends inclusive)

// pixel sides of an xyxy row: the fp32 side (what the IoU uses) times the image size, in fp64
__device__ __forceinline__ void pixel_sides(const float* xyxy, double img_h, double img_w, double& wp, double& hp) {
    wp = (double)(xyxy[2] - xyxy[0]) * img_w;
    hp = (double)(xyxy[3] - xyxy[1]) * img_h;
}

// bit r: the area lies outside range r (COCOeval: area < lo || area > hi)
__device__ __forceinline__ unsigned outside_ranges(double area) {
    return (area < 0.0 || area > 1024.0 ? 1u : 0u) | (area < 1024.0 || area > 9216.0 ? 2u : 0u) |
           (area < 9216.0 || area > 1e10 ? 4u : 0u);
}

// the box-size filter of the Prophesee protocol; a limit is active only when > 0
__device__ __forceinline__ bool too_small(double wp, double hp, double min_diag, double min_side) {
    return (min_diag > 0.0 && wp * wp + hp * hp < min_diag * min_diag) || (min_side > 0.0 && (wp < min_side || hp < min_side));
}

// One thread per row of dets [B][A][6] and labels [B][G][5].  det_key [B][A]: 0 .. C-1, C = class id out of range
// (counted in *bad), C + 1 = padding or removed by the size filter; label_cls [B][G]: the class column, -1 where removed.
__global__ __launch_bounds__(kMapThreads) void k_map_filter_rows(const float* __restrict__ dets,
                                                                 const float* __restrict__ labels, int64_t n_det,
                                                                 int64_t n_lab, int C, double img_h, double img_w,
                                                                 double min_diag, double min_side,
                                                                 int* __restrict__ det_key, float* __restrict__ label_cls,
                                                                 unsigned long long* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
    if (i >= n_det + n_lab) return;
    const bool is_det = i < n_det;
    const float* r = is_det ? dets + i * 6 : labels + (i - n_det) * 5;
    float cls = r[0];
    if (cls >= 0.0f) {
        double wp, hp;
        pixel_sides(r + (is_det ? 2 : 1), img_h, img_w, wp, hp);
        if (too_small(wp, hp, min_diag, min_side)) cls = -1.0f;
    }
    if (is_det) det_key[i] = cls < 0.0f ? C + 1 : cls >= (float)C ? C : (int)cls;
    else label_cls[i - n_det] = cls;
    if (cls >= (float)C) atomicAdd(bad, 1ull);   // rare; an integer, so the total does not depend on the order
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
            wave_argmax(bv, bi);
            if (bi >= 0) {
                if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
                if (lane == 0) atomicOr(&smask[d], 1u << t);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < S; i += kMapThreads) mask[rec + i] = smask[i];
}

// k_map_match with the area ranges beside "all".  label_cls [B][G] is the class column of the labels (the row filter's
// output).  A block has 16 waves and (1 + nr) * T work items (range a, threshold t), one wave each: a = 0 is
// k_map_match's matching, statement for statement (mask, score, npig: the same bits); a = 1 + r matches again with the
// ground truth outside range r ignored.  COCOeval.evaluateImg sorts the ground truth stably by the ignore flag and stops
// at the first ignored row once a non-ignored one is matched: a detection takes the free non-ignored row of largest IoU
// (ties to the later row) and looks among the free ignored rows, by the same rule, only when no non-ignored row
// qualifies.  A detection matched to an ignored row, or unmatched with its own area outside the range, is ignored.
// area_matched / area_ignored [B][C][nr][S]: bit t per slot; npig_area [nr][C] counts the non-ignored rows.
// LDS: 79 KiB static (one workgroup may hold up to 160 KiB on gfx950).
constexpr int kMapAreaThreads = 1024;
constexpr int kMapAreaWaves = kMapAreaThreads / 64;

__global__ __launch_bounds__(kMapAreaThreads) void k_map_match_areas(
    const float* __restrict__ dets, const float* __restrict__ labels, const float* __restrict__ label_cls,
    const int* __restrict__ order, const int* __restrict__ seg, int A, int G, int C, int S,
    const double* __restrict__ iou_thr, int T, double img_h, double img_w, int nr, float* __restrict__ score,
    unsigned* __restrict__ mask, unsigned* __restrict__ area_matched, unsigned* __restrict__ area_ignored,
    int* __restrict__ npig, int* __restrict__ npig_area) {
    __shared__ float4 dbox[kMapMaxSlots];
    __shared__ float4 gbox[kMapMaxGt];
    __shared__ unsigned smatch[1 + kMapRanges][kMapMaxSlots];   // [0]: "all", with the slot-used bit
    __shared__ unsigned signore[kMapRanges][kMapMaxSlots];
    __shared__ unsigned char dout[kMapMaxSlots];   // bit r: the detection's area is outside range r
    __shared__ unsigned char gout[kMapMaxGt];      // the same for the compacted ground truth: ignored in range r
    __shared__ int s_ng;
    const int c = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = seg[(int64_t)b * (C + 1) + c], hi = seg[(int64_t)b * (C + 1) + c + 1];
    const int nd = min(hi - lo, S);
    const int64_t rec = ((int64_t)b * C + c) * S;
    for (int i = tid; i < S; i += kMapAreaThreads) {
        float sc = -INFINITY;
        unsigned used = 0u;
        if (i < nd) {
            const float* r = dets + ((int64_t)b * A + order[(int64_t)b * A + lo + i]) * 6;
            sc = r[1];
            dbox[i] = make_float4(r[2], r[3], r[4] - r[2], r[5] - r[3]);
            double wp, hp;
            pixel_sides(r + 2, img_h, img_w, wp, hp);
            dout[i] = (unsigned char)outside_ranges(wp * hp);
            used = kSlotUsed;
        }
        score[rec + i] = sc;
        smatch[0][i] = used;
        for (int r = 0; r < nr; ++r) smatch[1 + r][i] = signore[r][i] = 0u;
    }
    if (wave == 0) {
        const float* lab = labels + (int64_t)b * G * 5;
        const float* cls = label_cls + (int64_t)b * G;
        int n = 0, inside[kMapRanges] = {0, 0, 0};
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            bool mine = false;
            unsigned out = 0u;
            if (g < G) {
                const float k = cls[g];
                mine = k >= 0.0f && (int)k == c;
            }
            const unsigned long long bal = __ballot(mine);
            if (mine) {
                const float* r = lab + (int64_t)g * 5;
                const int at = n + __popcll(bal & ((1ull << lane) - 1ull));
                gbox[at] = make_float4(r[1], r[2], r[3] - r[1], r[4] - r[2]);
                double wp, hp;
                pixel_sides(r + 1, img_h, img_w, wp, hp);   // the area once per row
                out = outside_ranges(wp * hp);
                gout[at] = (unsigned char)out;
            }
            n += __popcll(bal);
#pragma unroll
            for (int r = 0; r < kMapRanges; ++r) inside[r] += __popcll(__ballot(mine && !((out >> r) & 1u)));
        }
        if (lane == 0) {
            s_ng = n;
            if (n) atomicAdd(npig + c, n);
            for (int r = 0; r < nr; ++r)
                if (inside[r]) atomicAdd(npig_area + r * C + c, inside[r]);
        }
    }
    __syncthreads();
    const int ng = s_ng;
    for (int item = wave; item < (1 + nr) * T; item += kMapAreaWaves) {
        const int a = item / T, t = item % T, r = a - 1;
        const double thr = fmin(iou_thr[t], 1.0 - 1e-10);
        unsigned taken = 0u;
        if (a == 0) {   // "all", as k_map_match
            for (int d = 0; d < nd; ++d) {
                const float4 db = dbox[d];
                double bv = 0.0;
                int bi = -1;
                for (int j = 0, g = lane; g < ng; ++j, g += 64) {
                    if ((taken >> j) & 1u) continue;
                    const double iou = coco_iou(db, gbox[g]);
                    if (iou >= thr && (bi < 0 || iou >= bv)) {
                        bv = iou;
                        bi = g;
                    }
                }
                wave_argmax(bv, bi);
                if (bi >= 0) {
                    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
                    if (lane == 0) atomicOr(&smatch[0][d], 1u << t);
                }
            }
            continue;
        }
        for (int d = 0; d < nd; ++d) {
            const float4 db = dbox[d];
            double bv = 0.0, iv = 0.0;   // best free non-ignored / ignored row of this lane
            int bi = -1, ii = -1;
            for (int j = 0, g = lane; g < ng; ++j, g += 64) {
                if ((taken >> j) & 1u) continue;
                const double iou = coco_iou(db, gbox[g]);
                if (iou < thr) continue;
                if ((gout[g] >> r) & 1u) {
                    if (ii < 0 || iou >= iv) {
                        iv = iou;
                        ii = g;
                    }
                } else if (bi < 0 || iou >= bv) {
                    bv = iou;
                    bi = g;
                }
            }
            wave_argmax(bv, bi);
            bool ignored = false;
            if (bi < 0) {   // wave-uniform: no non-ignored row qualifies anywhere
                wave_argmax(iv, ii);
                bi = ii;
                ignored = bi >= 0;
            }
            if (bi >= 0) {
                if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
                if (lane == 0) atomicOr(&smatch[a][d], 1u << t);
            } else {
                ignored = (dout[d] >> r) & 1u;
            }
            if (ignored && lane == 0) atomicOr(&signore[r][d], 1u << t);
        }
    }
    __syncthreads();
    for (int i = tid; i < S; i += kMapAreaThreads) {
        mask[rec + i] = smatch[0][i];
        for (int r = 0; r < nr; ++r) {
            const int64_t at = (((int64_t)b * C + c) * nr + r) * S + i;
            area_matched[at] = smatch[1 + r][i];
            area_ignored[at] = signore[r][i];
        }
    }
}

// One block per (class c, maxDet index mi, IoU threshold t).  order [C][N]: record positions (image * S + slot) of
// class c sorted by score descending, stably; mask [C][N] in position order.  Writes qsum = sum over the recall
// thresholds of the interpolated precision and recall = rc[-1] (both -1 for a class without ground truth).
//
// Interpolated precision q[r] = (reverse running max of pr)[searchsorted_left(rc, r)] is the max of pr over the records
// with rc >= r (rc is non-decreasing), and on records with the same tp count pr is largest at the true positive that
// reached it.  So each true positive k contributes pr_k to q[0 .. n_k) with n_k = #{r : r <= rc_k}: one LDS atomicMax
// into bucket n_k - 1 (pr >= 0, so its bit pattern orders like its value), then a running max from the right.
//
// kAreas: blockIdx.z = a * T + t with a = 0 for "all" and a = 1 + r for range r, whose records come from area_matched /
// area_ignored [C][nr][N] (a record ignored at t is neither tp nor fp) and whose ground-truth count is npig_area[r][c];
// qsum / recall are then [1 + nr][C][M][T].
template <bool kAreas>
__global__ __launch_bounds__(kMapThreads) void k_map_accumulate(const int* __restrict__ order,
                                                                const unsigned* __restrict__ mask,
                                                                const unsigned* __restrict__ area_matched,
                                                                const unsigned* __restrict__ area_ignored,
                                                                const int* __restrict__ npig,
                                                                const int* __restrict__ npig_area, int N, int S,
                                                                const int* __restrict__ max_dets, int M,
                                                                const double* __restrict__ rec_thr, int R, int T,
                                                                int nr, double* __restrict__ qsum,
                                                                double* __restrict__ recall) {
    __shared__ unsigned long long bucket[kMapMaxRec];
    __shared__ double rthr[kMapMaxRec];
    __shared__ unsigned long long wsum[kMapWaves];
    const int c = blockIdx.x, mi = blockIdx.y;
    const int a = kAreas ? blockIdx.z / T : 0, t = kAreas ? blockIdx.z % T : blockIdx.z;
    const int C = gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t out = (((int64_t)a * C + c) * M + mi) * T + t;
    const int np = a ? npig_area[(a - 1) * C + c] : npig[c];
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
    const unsigned* amt = a ? area_matched + ((int64_t)c * nr + a - 1) * N : nullptr;
    const unsigned* aig = a ? area_ignored + ((int64_t)c * nr + a - 1) * N : nullptr;
    unsigned long long carry = 0ull;   // (tp << 32) | fp of the chunks before
    for (int base = 0; base < N; base += kMapThreads) {
        const int n = base + tid;
        unsigned long long v = 0ull;
        bool tp = false;
        if (n < N) {
            const int p = ord[n];
            const unsigned m = msk[p];
            if ((m & kSlotUsed) && p % S < md) {   // an image's first maxDet detections of the class
                if (!a) {
                    tp = (m >> t) & 1u;
                    v = tp ? (1ull << 32) : 1ull;
                } else if (!((aig[p] >> t) & 1u)) {   // an ignored record keeps its slot and counts as neither
                    tp = (amt[p] >> t) & 1u;
                    v = tp ? (1ull << 32) : 1ull;
                }
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

// number of classes with ground truth
__device__ double valid_classes(const int* __restrict__ np, int C, double* red) {
    double v = 0.0;
    for (int c = threadIdx.x; c < C; c += kMapThreads) v += np[c] > 0 ? 1.0 : 0.0;
    return block_sum(v, red);
}

// mean of src[c][mi][t0 .. t0 + nt) over the nv classes with ground truth, each entry a sum of `per` values; fp64 with
// a fixed reduction tree, rounded once to fp32; -1 when nothing is valid
__device__ float class_mean(const double* __restrict__ src, const int* __restrict__ np, double nv, int C, int M, int T,
                            int mi, int t0, int nt, int per, double* red) {
    double v = 0.0;
    for (int k = threadIdx.x; k < C * nt; k += kMapThreads) {
        const int c = k / nt, t = t0 + k % nt;
        if (np[c] > 0) v += src[((int64_t)c * M + mi) * T + t];
    }
    const double s = block_sum(v, red);
    const double cnt = nv * nt * per;
    return cnt > 0.0 ? (float)(s / cnt) : -1.0f;
}

// out[0] map, out[1] map_50, out[2] map_75, out[3 + mi] mar at max_dets[mi]; then, per range r, map_<r> and mar_<r> at
// the largest maxDet from the range's own qsum / recall block and ground-truth counts.  out_class (may be null) [2][C]:
// a class's AP (mean over thresholds x recall thresholds) and AR at the largest maxDet for "all", -1 without ground truth.
__global__ __launch_bounds__(kMapThreads) void k_map_summary(const double* __restrict__ qsum,
                                                             const double* __restrict__ recall,
                                                             const int* __restrict__ npig,
                                                             const int* __restrict__ npig_area, int C, int M, int T, int R,
                                                             int t50, int t75, int nr, float* __restrict__ out,
                                                             float* __restrict__ out_class) {
    __shared__ double red[kMapThreads];
    const int tid = threadIdx.x;
    const int last = M - 1;
    const double nv = valid_classes(npig, C, red);
    for (int o = 0; o < 3 + M; ++o) {
        const int mi = o < 3 ? last : o - 3;
        const int t0 = o == 1 ? t50 : o == 2 ? t75 : 0;
        const int nt = o == 1 || o == 2 ? (t0 >= 0 ? 1 : 0) : T;
        const float v = class_mean(o < 3 ? qsum : recall, npig, nv, C, M, T, mi, t0, nt, o < 3 ? R : 1, red);
        if (tid == 0) out[o] = v;
    }
    for (int r = 0; r < nr; ++r) {
        const int64_t at = (int64_t)(1 + r) * C * M * T;
        const int* np = npig_area + r * C;
        const double nva = valid_classes(np, C, red);
        const float ap = class_mean(qsum + at, np, nva, C, M, T, last, 0, T, R, red);
        const float ar = class_mean(recall + at, np, nva, C, M, T, last, 0, T, 1, red);
        if (tid == 0) {
            out[3 + M + 2 * r] = ap;
            out[3 + M + 2 * r + 1] = ar;
        }
    }
    if (out_class)
        for (int c = tid; c < C; c += kMapThreads) {
            double ap = 0.0, ar = 0.0;
            for (int t = 0; t < T; ++t) {
                ap += qsum[((int64_t)c * M + last) * T + t];
                ar += recall[((int64_t)c * M + last) * T + t];
            }
            out_class[c] = npig[c] > 0 ? (float)(ap / ((double)T * R)) : -1.0f;
            out_class[C + c] = npig[c] > 0 ? (float)(ar / (double)T) : -1.0f;
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
    hipLaunchKernelGGL(k_map_accumulate<false>, dim3((unsigned)num_classes, (unsigned)num_max_dets, (unsigned)num_iou),
                       dim3(kMapThreads), 0, st, order, match_mask, (const unsigned*)nullptr, (const unsigned*)nullptr,
                       npig, (const int*)nullptr, records, slots, max_dets, num_max_dets, rec_thresholds, num_rec,
                       num_iou, 0, qsum, recall);
    SNN_CHECK_LAUNCH("snn_map_accumulate");
    hipLaunchKernelGGL(k_map_summary, dim3(1), dim3(kMapThreads), 0, st, qsum, recall, npig, (const int*)nullptr,
                       num_classes, num_max_dets, num_iou, num_rec, t50, t75, 0, out, (float*)nullptr);
    SNN_CHECK_LAUNCH("snn_map_accumulate (summary)");
    return 0;
}

extern "C" int snn_map_filter_rows(const float* dets, const float* labels, int B, int A, int G, int num_classes,
                                   double img_h, double img_w, double min_box_diag, double min_box_side, int* det_key,
                                   float* label_cls, int64_t* bad, void* stream) {
    SNN_REQUIRE(dets && labels && det_key && label_cls && bad, "snn_map_filter_rows: null pointer");
    SNN_REQUIRE(B > 0 && A > 0 && G > 0 && num_classes > 0, "snn_map_filter_rows: bad shape");
    SNN_REQUIRE((int64_t)B * ((int64_t)A + G) <= 0x7fffffff, "snn_map_filter_rows: %lld rows exceed the 31-bit row index",
                (long long)B * ((long long)A + G));
    SNN_REQUIRE(img_h > 0.0 && img_w > 0.0, "snn_map_filter_rows: image size %g x %g must be positive", img_h, img_w);
    SNN_REQUIRE(min_box_diag >= 0.0 && min_box_side >= 0.0, "snn_map_filter_rows: min_box_diag %g / min_box_side %g must "
                "be >= 0 (0: off)", min_box_diag, min_box_side);
    const int64_t n_det = (int64_t)B * A, n_lab = (int64_t)B * G;
    hipLaunchKernelGGL(k_map_filter_rows, dim3((unsigned)snn_ceil_div(n_det + n_lab, kMapThreads)), dim3(kMapThreads), 0,
                       (hipStream_t)stream, dets, labels, n_det, n_lab, num_classes, img_h, img_w, min_box_diag,
                       min_box_side, det_key, label_cls, reinterpret_cast<unsigned long long*>(bad));
    SNN_CHECK_LAUNCH("snn_map_filter_rows");
    return 0;
}

extern "C" int snn_map_match_areas(const float* dets, const float* labels, const float* label_cls, const int* order,
                                   const int* seg, int B, int A, int G, int num_classes, int slots,
                                   const double* iou_thresholds, int num_iou, double img_h, double img_w, int num_ranges,
                                   float* score, unsigned* match_mask, unsigned* area_matched, unsigned* area_ignored,
                                   int* npig, int* npig_area, void* stream) {
    SNN_REQUIRE(dets && labels && label_cls && order && seg && iou_thresholds && score && match_mask && npig,
                "snn_map_match_areas: null pointer");
    SNN_REQUIRE(num_ranges == 0 || num_ranges == kMapRanges, "snn_map_match_areas: num_ranges %d is neither 0 nor %d "
                "(small, medium, large)", num_ranges, kMapRanges);
    SNN_REQUIRE(num_ranges == 0 || (area_matched && area_ignored && npig_area),
                "snn_map_match_areas: null area pointer with num_ranges %d", num_ranges);
    SNN_REQUIRE(B > 0 && B <= 65535 && A > 0 && G >= 0 && num_classes > 0, "snn_map_match_areas: bad shape");
    SNN_REQUIRE(G <= kMapMaxGt, "snn_map_match_areas: %d ground-truth rows per image exceed the limit of %d", G,
                kMapMaxGt);
    SNN_REQUIRE(slots > 0 && slots <= kMapMaxSlots, "snn_map_match_areas: %d detection slots per class (the largest "
                "maxDet) outside 1..%d", slots, kMapMaxSlots);
    SNN_REQUIRE(num_iou > 0 && num_iou <= kMapMaxIou, "snn_map_match_areas: %d IoU thresholds outside 1..%d", num_iou,
                kMapMaxIou);
    SNN_REQUIRE(img_h > 0.0 && img_w > 0.0, "snn_map_match_areas: image size %g x %g must be positive", img_h, img_w);
    hipLaunchKernelGGL(k_map_match_areas, dim3((unsigned)num_classes, (unsigned)B), dim3(kMapAreaThreads), 0,
                       (hipStream_t)stream, dets, labels, label_cls, order, seg, A, G, num_classes, slots, iou_thresholds,
                       num_iou, img_h, img_w, num_ranges, score, match_mask, area_matched, area_ignored, npig, npig_area);
    SNN_CHECK_LAUNCH("snn_map_match_areas");
    return 0;
}

extern "C" size_t snn_map_areas_workspace_size(int num_classes, int num_max_dets, int num_iou, int num_ranges) {
    if (num_ranges != 0 && num_ranges != kMapRanges) return 0;
    return (1 + num_ranges) * snn_map_workspace_size(num_classes, num_max_dets, num_iou);
}

extern "C" int snn_map_accumulate_areas(const int* order, const unsigned* match_mask, const unsigned* area_matched,
                                        const unsigned* area_ignored, const int* npig, const int* npig_area,
                                        int num_classes, int records, int slots, const int* max_dets, int num_max_dets,
                                        const double* rec_thresholds, int num_rec, int num_iou, int t50, int t75,
                                        int num_ranges, void* workspace, float* out, float* out_class, void* stream) {
    SNN_REQUIRE(order && match_mask && npig && max_dets && rec_thresholds && workspace && out,
                "snn_map_accumulate_areas: null pointer");
    SNN_REQUIRE(num_ranges == 0 || num_ranges == kMapRanges, "snn_map_accumulate_areas: num_ranges %d is neither 0 nor "
                "%d (small, medium, large)", num_ranges, kMapRanges);
    SNN_REQUIRE(num_ranges == 0 || (area_matched && area_ignored && npig_area),
                "snn_map_accumulate_areas: null area pointer with num_ranges %d", num_ranges);
    SNN_REQUIRE(num_classes > 0 && records >= 0 && slots > 0 && records % slots == 0,
                "snn_map_accumulate_areas: bad shape");
    SNN_REQUIRE(num_max_dets > 0 && num_max_dets <= 65535, "snn_map_accumulate_areas: bad maxDet count");
    SNN_REQUIRE(num_iou > 0 && num_iou <= kMapMaxIou, "snn_map_accumulate_areas: %d IoU thresholds outside 1..%d",
                num_iou, kMapMaxIou);
    SNN_REQUIRE(num_rec > 0 && num_rec <= kMapMaxRec, "snn_map_accumulate_areas: %d recall thresholds outside 1..%d",
                num_rec, kMapMaxRec);
    SNN_REQUIRE(t50 < num_iou && t75 < num_iou, "snn_map_accumulate_areas: bad threshold index");
    const size_t block = (size_t)num_classes * num_max_dets * num_iou;   // per "all" / range: [C][M][T]
    double* qsum = static_cast<double*>(workspace);
    double* recall = qsum + (1 + num_ranges) * block;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_map_accumulate<true>,
                       dim3((unsigned)num_classes, (unsigned)num_max_dets, (unsigned)(num_iou * (1 + num_ranges))),
                       dim3(kMapThreads), 0, st, order, match_mask, area_matched, area_ignored, npig, npig_area, records,
                       slots, max_dets, num_max_dets, rec_thresholds, num_rec, num_iou, num_ranges, qsum, recall);
    SNN_CHECK_LAUNCH("snn_map_accumulate_areas");
    hipLaunchKernelGGL(k_map_summary, dim3(1), dim3(kMapThreads), 0, st, qsum, recall, npig, npig_area, num_classes,
                       num_max_dets, num_iou, num_rec, t50, t75, num_ranges, out, out_class);
    SNN_CHECK_LAUNCH("snn_map_accumulate_areas (summary)");
    return 0;
}
