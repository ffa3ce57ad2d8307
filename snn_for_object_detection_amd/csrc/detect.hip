// Detection decode on the device: the tail of SODa.predict (models/soda.py:202-233,
// utils/box.py:72-153) without host round trips.
//
//   snn_detect_decode : per anchor conf = max_k p[k], class = argmax - 1 (background = -1), box = offset_inverse
//   snn_nms_sorted    : per-class greedy non-maximum suppression over candidates sorted by descending confidence
//   snn_detect_decode_batched / snn_nms_sorted_batched / snn_detect_assemble : the same for N frames in three launches,
//                       the last one writing the output rows (utils/box.py:121-153) of every frame
//
// Arithmetic follows the reference expression by expression (fp32, -ffp-contract=off), so the kept sets are those
// of utils/box.py:82-99 (pinned by tests/golden/detect_nms*.npz).
#include "snn_common.h"

namespace {

constexpr int kNmsThreads = 256;

// offset_inverse (utils/box.py:72-79) of one anchor
__device__ __forceinline__ void decode_box(const float* __restrict__ anc, const float* __restrict__ off, float* out) {
    const float ax1 = anc[0], ay1 = anc[1], ax2 = anc[2], ay2 = anc[3];
    const float acx = (ax1 + ax2) / 2, acy = (ay1 + ay2) / 2, aw = ax2 - ax1, ah = ay2 - ay1;
    const float cx = (off[0] * aw / 10) + acx;
    const float cy = (off[1] * ah / 10) + acy;
    const float w = expf(off[2] / 5) * aw;
    const float h = expf(off[3] / 5) * ah;
    out[0] = cx - 0.5f * w;
    out[1] = cy - 0.5f * h;
    out[2] = cx + 0.5f * w;
    out[3] = cy + 0.5f * h;
}

__global__ void k_detect_decode(const float* __restrict__ prob, const float* __restrict__ offsets,
                                const float* __restrict__ anchors, int rows, int A, int K,
                                float* __restrict__ conf, int* __restrict__ cls, float* __restrict__ boxes) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;  // row of [frames][A]; its anchor is a % A
    if (a >= rows) return;
    const float* p = prob + (int64_t)a * K;
    float best = p[0];
    int arg = 0;
    for (int k = 1; k < K; ++k)
        if (p[k] > best) {  // first maximum wins, as torch.max
            best = p[k];
            arg = k;
        }
    conf[a] = best;
    cls[a] = arg - 1;
    decode_box(anchors + (int64_t)(a % A) * 4, offsets + (int64_t)a * 4, boxes + (int64_t)a * 4);
}

// box_iou (utils/box.py:31-59) of two corner boxes
__device__ __forceinline__ float iou_of(const float4 p, const float4 q) {
    const float area1 = (p.z - p.x) * (p.w - p.y);
    const float area2 = (q.z - q.x) * (q.w - q.y);
    const float lx = fmaxf(p.x, q.x), ly = fmaxf(p.y, q.y);
    const float rx = fminf(p.z, q.z), ry = fminf(p.w, q.w);
    const float ow = fmaxf(rx - lx, 0.0f), oh = fmaxf(ry - ly, 0.0f);
    const float overlap = ow * oh;
    return overlap / (area1 + area2 - overlap);
}

// One block per class.  `order` holds anchor ids sorted by (class ascending, confidence descending); the members of
// the block's class are order[lo .. hi).  Greedy NMS in chunks of 256 candidates:
//   1. every candidate of the chunk is tested against the boxes kept so far (parallel over candidates);
//   2. the chunk's own 256 x 256 suppression relation is formed as bit masks (parallel), and one thread walks the
//      chunk in order applying them - the only sequential part, 256 trivial steps.
// Kept ids are appended to kept[lo ..) in keep order; their number is returned (to every thread).
__device__ __forceinline__ int nms_class_block(const float* __restrict__ boxes, const int* __restrict__ order,
                                               const int lo, const int hi, float thr, int* __restrict__ kept,
                                               unsigned char* __restrict__ kept_flag, int* __restrict__ kept_rank) {
    __shared__ float4 cand[kNmsThreads];
    __shared__ float4 ktile[kNmsThreads];
    __shared__ unsigned long long mask[kNmsThreads][kNmsThreads / 64];
    __shared__ unsigned char alive[kNmsThreads];
    __shared__ int s_nkept, s_new;
    __shared__ int newly[kNmsThreads];
    const int tid = threadIdx.x;
    if (tid == 0) s_nkept = 0;
    __syncthreads();
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    for (int base = lo; base < hi; base += kNmsThreads) {
        const int n = min(kNmsThreads, hi - base);
        const int my = tid < n ? order[base + tid] : -1;
        const float4 mine = tid < n ? bx[my] : make_float4(0.f, 0.f, 0.f, 0.f);
        cand[tid] = mine;
        bool live = tid < n;
        // 1. against everything kept so far (tiles of 256 kept boxes staged through LDS)
        const int nk = s_nkept;
        for (int kb = 0; kb < nk; kb += kNmsThreads) {
            const int m = min(kNmsThreads, nk - kb);
            __syncthreads();
            if (tid < m) ktile[tid] = bx[kept[lo + kb + tid]];
            __syncthreads();
            if (live)
                for (int j = 0; j < m; ++j)
                    if (!(iou_of(ktile[j], mine) <= thr)) {  // the reference KEEPS iou <= thr (box.py:95-97): a NaN IoU suppresses
                        live = false;
                        break;
                    }
        }
        alive[tid] = live ? 1 : 0;
        __syncthreads();
        // 2. suppression masks inside the chunk: bit j of row i = candidate i suppresses the later candidate j
        unsigned long long m4[kNmsThreads / 64] = {0ull, 0ull, 0ull, 0ull};
        if (tid < n)
            for (int j = tid + 1; j < n; ++j)
                if (!(iou_of(mine, cand[j]) <= thr)) m4[j >> 6] |= 1ull << (j & 63);
#pragma unroll
        for (int w = 0; w < kNmsThreads / 64; ++w) mask[tid][w] = m4[w];
        __syncthreads();
        if (tid == 0) {
            unsigned long long gone[kNmsThreads / 64] = {0ull, 0ull, 0ull, 0ull};
            int cnt = 0;
            for (int i = 0; i < n; ++i) {
                if (!alive[i] || ((gone[i >> 6] >> (i & 63)) & 1ull)) continue;
                newly[cnt++] = i;
#pragma unroll
                for (int w = 0; w < kNmsThreads / 64; ++w) gone[w] |= mask[i][w];
            }
            s_new = cnt;
        }
        __syncthreads();
        const int cnt = s_new, nk0 = s_nkept;
        __syncthreads();  // everyone has read the counters before thread 0 advances them
        if (tid < cnt) {
            const int id = order[base + newly[tid]];
            kept[lo + nk0 + tid] = id;
            kept_flag[id] = 1;
            kept_rank[id] = nk0 + tid;
        }
        // kept[] is re-read through global memory by the next chunk's step 1: agent-scope fence (write back + L1
        // invalidate) so that no stale line of this CU's L1 is served
        if (tid == 0) s_nkept = nk0 + cnt;
        __threadfence();
        __syncthreads();
    }
    return s_nkept;
}

// the members of class c are order[seg[c] .. seg[c+1]); nkept[c] receives the number kept
__global__ __launch_bounds__(kNmsThreads) void k_nms_sorted(const float* __restrict__ boxes,
                                                            const int* __restrict__ order,
                                                            const int* __restrict__ seg, float thr,
                                                            int* __restrict__ kept, int* __restrict__ nkept,
                                                            unsigned char* __restrict__ kept_flag,
                                                            int* __restrict__ kept_rank) {
    const int c = blockIdx.x;
    const int n = nms_class_block(boxes, order, seg[c], seg[c + 1], thr, kept, kept_flag, kept_rank);
    if (threadIdx.x == 0) nkept[c] = n;
}

// One block per (class, frame).  `order` holds row ids of [N][A] sorted by (frame, class ascending, confidence
// descending, anchor ascending); seg[N][C + 1] counts inside the frame, so frame n's class c is
// order[n * A + seg[n][c] .. n * A + seg[n][c + 1]).  kept / kept_flag / kept_rank are indexed as in k_nms_sorted, by row.
__global__ __launch_bounds__(kNmsThreads) void k_nms_sorted_batched(const float* __restrict__ boxes,
                                                                    const int* __restrict__ order,
                                                                    const int* __restrict__ seg, int A, int C,
                                                                    float thr, int* __restrict__ kept,
                                                                    int* __restrict__ nkept,
                                                                    unsigned char* __restrict__ kept_flag,
                                                                    int* __restrict__ kept_rank) {
    const int n = blockIdx.x / C, c = blockIdx.x % C;
    const int* fseg = seg + (int64_t)n * (C + 1);
    // a seg that is not a non-decreasing sequence inside [0, A] would index out of the frame: treat the class as empty
    int lo = fseg[c], hi = fseg[c + 1];
    if (lo < 0 || hi > A || lo > hi) lo = hi = 0;
    const int cnt = nms_class_block(boxes, order, n * A + lo, n * A + hi, thr, kept, kept_flag, kept_rank);
    if (threadIdx.x == 0) nkept[(int64_t)n * C + c] = cnt;
}

constexpr int kAssembleMaxClasses = 1024;

// Output rows of multibox_detection (utils/box.py:121-153), one block per frame: kept rows first in class-then-score
// order (class_off[class] + rank), the others behind them in anchor order (exclusive block scan of the not-kept flags
// over A, 256 rows at a time); rows below pos_threshold get class -1 and confidence 1 - conf.
__global__ __launch_bounds__(kNmsThreads) void k_detect_assemble(const float* __restrict__ conf,
                                                                 const int* __restrict__ cls,
                                                                 const float* __restrict__ boxes,
                                                                 const int* __restrict__ nkept,
                                                                 const unsigned char* __restrict__ kept_flag,
                                                                 const int* __restrict__ kept_rank, int A, int C,
                                                                 float pos_threshold, float* __restrict__ out) {
    __shared__ int class_off[kAssembleMaxClasses + 1];
    __shared__ int wave_sum[kNmsThreads / 64];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int run = 0;
        for (int c = 0; c < C; ++c) {
            class_off[c] = run;
            run += nkept[(int64_t)n * C + c];
        }
        class_off[C] = run;
    }
    __syncthreads();
    int rest = class_off[C];  // position of the next not-kept row
    const int64_t row0 = (int64_t)n * A;
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    for (int base = 0; base < A; base += kNmsThreads) {
        const int a = base + tid;
        const bool valid = a < A;
        const bool is_kept = valid && kept_flag[row0 + a] != 0;
        const int nk = (valid && !is_kept) ? 1 : 0;
        int incl = nk;  // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kNmsThreads / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        __syncthreads();  // wave_sum is rewritten by the next chunk
        if (valid) {
            const float p = conf[row0 + a];
            const int k = cls[row0 + a];
            const int pos = is_kept ? class_off[min(max(k, 0), C - 1)] + kept_rank[row0 + a] : rest + before + incl - nk;
            const bool weak = p < pos_threshold;
            const float4 b = bx[row0 + a];
            if (pos >= 0 && pos < A) {  // (always, for flags / ranks written by k_nms_sorted_batched)
                float2* o = reinterpret_cast<float2*>(out + (row0 + pos) * 6);
                o[0] = make_float2((is_kept && !weak) ? (float)k : -1.0f, weak ? 1 - p : p);
                o[1] = make_float2(b.x, b.y);
                o[2] = make_float2(b.z, b.w);
            }
        }
        rest += total;
    }
}

}  // namespace

extern "C" int snn_detect_decode(const float* cls_prob, const float* offsets, const float* anchors, int A, int K,
                                 float* conf, int* cls, float* boxes, void* stream) {
    SNN_REQUIRE(cls_prob && offsets && anchors && conf && cls && boxes, "snn_detect_decode: null pointer");
    SNN_REQUIRE(A > 0 && K > 1, "snn_detect_decode: bad shape");
    hipLaunchKernelGGL(k_detect_decode, dim3((A + 255) / 256), dim3(256), 0, (hipStream_t)stream, cls_prob, offsets,
                       anchors, A, A, K, conf, cls, boxes);
    SNN_CHECK_LAUNCH("snn_detect_decode");
    return 0;
}

extern "C" int snn_nms_sorted(const float* boxes, const int* order, const int* seg, int num_classes,
                              float iou_threshold, int* kept, int* nkept, unsigned char* kept_flag, int* kept_rank,
                              void* stream) {
    SNN_REQUIRE(boxes && order && seg && kept && nkept && kept_flag && kept_rank, "snn_nms_sorted: null pointer");
    SNN_REQUIRE(num_classes > 0 && num_classes <= 65535, "snn_nms_sorted: bad class count");
    SNN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15u) == 0, "snn_nms_sorted: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(k_nms_sorted, dim3((unsigned)num_classes), dim3(kNmsThreads), 0, (hipStream_t)stream, boxes,
                       order, seg, iou_threshold, kept, nkept, kept_flag, kept_rank);
    SNN_CHECK_LAUNCH("snn_nms_sorted");
    return 0;
}

extern "C" int snn_detect_decode_batched(const float* cls_prob, const float* offsets, const float* anchors, int N, int A,
                                         int K, float* conf, int* cls, float* boxes, void* stream) {
    SNN_REQUIRE(cls_prob && offsets && anchors && conf && cls && boxes, "snn_detect_decode_batched: null pointer");
    SNN_REQUIRE(N > 0 && A > 0 && K > 1 && (int64_t)N * A <= INT32_MAX - 256, "snn_detect_decode_batched: bad shape");
    const int rows = N * A;
    hipLaunchKernelGGL(k_detect_decode, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, cls_prob, offsets,
                       anchors, rows, A, K, conf, cls, boxes);
    SNN_CHECK_LAUNCH("snn_detect_decode_batched");
    return 0;
}

extern "C" int snn_nms_sorted_batched(const float* boxes, const int* order, const int* seg, int N, int A,
                                      int num_classes, float iou_threshold, int* kept, int* nkept,
                                      unsigned char* kept_flag, int* kept_rank, void* stream) {
    SNN_REQUIRE(boxes && order && seg && kept && nkept && kept_flag && kept_rank,
                "snn_nms_sorted_batched: null pointer");
    SNN_REQUIRE(N > 0 && A > 0 && (int64_t)N * A <= INT32_MAX - 256, "snn_nms_sorted_batched: bad shape");
    SNN_REQUIRE(num_classes > 0 && num_classes <= 65535 && (int64_t)N * num_classes <= INT32_MAX,
                "snn_nms_sorted_batched: bad class count");
    SNN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15u) == 0, "snn_nms_sorted_batched: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(k_nms_sorted_batched, dim3((unsigned)(N * num_classes)), dim3(kNmsThreads), 0,
                       (hipStream_t)stream, boxes, order, seg, A, num_classes, iou_threshold, kept, nkept, kept_flag,
                       kept_rank);
    SNN_CHECK_LAUNCH("snn_nms_sorted_batched");
    return 0;
}

extern "C" int snn_detect_assemble(const float* conf, const int* cls, const float* boxes, const int* nkept,
                                   const unsigned char* kept_flag, const int* kept_rank, int N, int A, int num_classes,
                                   float pos_threshold, float* out, void* stream) {
    SNN_REQUIRE(conf && cls && boxes && nkept && kept_flag && kept_rank && out, "snn_detect_assemble: null pointer");
    SNN_REQUIRE(N > 0 && A > 0 && (int64_t)N * A <= INT32_MAX - 256, "snn_detect_assemble: bad shape");
    SNN_REQUIRE(num_classes > 0 && num_classes <= kAssembleMaxClasses, "snn_detect_assemble: bad class count");
    SNN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0,
                "snn_detect_assemble: boxes must be 16-byte and out 8-byte aligned");
    hipLaunchKernelGGL(k_detect_assemble, dim3((unsigned)N), dim3(kNmsThreads), 0, (hipStream_t)stream, conf, cls, boxes,
                       nkept, kept_flag, kept_rank, A, num_classes, pos_threshold, out);
    SNN_CHECK_LAUNCH("snn_detect_assemble");
    return 0;
}
