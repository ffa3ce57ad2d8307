// The event feed for gfx950: events -> [T][B][H][W][2] frames (a scatter of idempotent 1.0f stores into a zero-filled
// buffer) and the label side of the augmentation.  k_events takes one sample's pre-binned events; k_events_batch bins the
// raw timestamps of a whole batch and applies a per-sample flip / zoom / shift / random drop, reading the events either as
// four arrays or as the 8-byte records of a Prophesee DAT recording.  HBM-bound on the read, uncoalesced 4-byte stores by
// nature; include/snn_hip.h states the rules.  The count / time-surface / voxel-grid representations replace the store
// by integer atomics on the same buffer viewed as uint32 (order independent, so bit-reproducible) and k_events_finalize
// turns the accumulators into fp32 values in place.
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;

__global__ void k_events(const int32_t* __restrict__ tb, const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                         const int32_t* __restrict__ ps, int64_t n, float* __restrict__ frames, int T, int H, int W) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        int t = tb[e], x = xs[e], y = ys[e], p = ps[e];
        if (t < 0 || t >= T || y < 0 || y >= H || p < 0 || p > 1) continue;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        frames[(((int64_t)t * H + y) * W + x) * 2 + p] = 1.0f;  // idempotent store: races are benign
    }
}

// ------------------------------------------------------------------------------------------ batch scatter
// Where the events of a batch come from: load(e) gives event e as the scatter uses it, the time zero- or sign-extended
// to 64 bits.
struct Event {
    uint64_t t;
    int x, y, p;
};
struct TupleEvents {   // four arrays
    const int64_t* ts;
    const int32_t *xs, *ys, *ps;
    __device__ __forceinline__ Event load(int64_t e) const { return {(uint64_t)ts[e], xs[e], ys[e], ps[e]}; }
};
// The records of a DAT recording, 8 bytes each: the timestamp in microseconds and one word holding x (bits 0-13), y
// (14-27) and the polarity (28; bits 29-31 are not read).  One 8-byte load per lane, so a wave reads 512 contiguous
// bytes.  No field can be negative, so of the field rules only y >= H and x > W - 1 are left once this is inlined.
struct PackedEvents {
    const uint2* words;
    __device__ __forceinline__ Event load(int64_t e) const {
        const uint2 rec = words[e];
        return {rec.x, (int)(rec.y & 0x3FFFu), (int)((rec.y >> 14) & 0x3FFFu), (int)((rec.y >> 28) & 1u)};
    }
};

constexpr int kLdsB = 64;   // batches up to this size keep offsets, window starts and the table in LDS

__device__ __forceinline__ uint32_t fmix32(uint32_t u) {   // murmur3's finaliser
    u ^= u >> 16;
    u *= 0x85EBCA6Bu;
    u ^= u >> 13;
    u *= 0xC2B2AE35u;
    u ^= u >> 16;
    return u;
}

// The scatter with the binning of the raw timestamps and a per-sample flip / zoom / shift / random drop inside it
// (include/snn_hip.h states the rules).  A thread finds the sample of its event by binary search over the batch's
// offsets.  AUG = false: no table is read (the identity), the field checks alone decide what is stored.  REP says what
// is written (rule 7): the 1.0f store, or an integer atomic on the cell's bits - a count, the latest offset inside the
// bin + 1, or Q16 weights to the two bins whose centres enclose the event.  The atomics return nothing.
template <class Source, bool AUG, int REP = SNN_EVREP_BINARY>
__global__ __launch_bounds__(kThreads) void k_events_batch(
        const Source src, const int64_t* __restrict__ offsets, const int64_t* __restrict__ t0s,
        const int32_t* __restrict__ aug, int64_t n, float* __restrict__ frames, int T, int B, int H, int W,
        int64_t step_us, uint64_t window_us) {
    __shared__ int64_t s_off[kLdsB + 1];
    __shared__ int64_t s_t0[kLdsB];
    __shared__ int32_t s_aug[AUG ? kLdsB * 8 : 1];
    const int64_t* off = offsets;
    const int64_t* t0 = t0s;
    const int32_t* tab = aug;
    if (B <= kLdsB) {  // block-uniform
        for (int i = threadIdx.x; i <= B; i += kThreads) s_off[i] = offsets[i];
        for (int i = threadIdx.x; i < B; i += kThreads) s_t0[i] = t0s[i];
        if (AUG)
            for (int i = threadIdx.x; i < B * 8; i += kThreads) s_aug[i] = aug[i];
        __syncthreads();
        off = s_off, t0 = s_t0;
        if (AUG) tab = s_aug;
    }
    const bool narrow = window_us <= 0xFFFFFFFFull;  // the quotient of an event inside the window fits 32-bit division
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        const Event ev = src.load(e);   // issued before the search: its latency hides behind the LDS reads
        int lo = 0, hi = B;  // the last sample whose slice starts at or before e (empty samples share a start)
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (off[mid] <= e) lo = mid; else hi = mid;
        }
        const int b = lo;
        const int64_t j = e - off[b];
        if (j < 0 || e >= off[b + 1]) continue;  // an event no slice owns
        // floor((t - t0) / step) in [0, T)  <=>  0 <= t - t0 < T * step
        const int64_t d = (int64_t)(ev.t - (uint64_t)t0[b]);
        if (d < 0 || (uint64_t)d >= window_us) continue;
        const int t = narrow ? (int)((uint32_t)d / (uint32_t)step_us) : (int)(d / step_us);
        int x = ev.x;
        const int y = ev.y, p = ev.p;
        if (y < 0 || y >= H || p < 0 || p > 1) continue;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        int xo = x, yo = y;
        if (AUG) {
            const int32_t* row = tab + b * 8;
            const uint32_t drop = (uint32_t)row[4];
            if (drop) {
                const uint32_t k = fmix32((uint32_t)row[5] + 0x9E3779B9u * (uint32_t)((uint64_t)j >> 32));
                if (fmix32((uint32_t)j ^ k) < drop) continue;
            }
            if (row[0]) x = W - 1 - x;
            const int64_t a = row[1];
            const int64_t xw = (((int64_t)(2 * x + 1) * a) >> 17) + row[2];
            const int64_t yw = (((int64_t)(2 * y + 1) * a) >> 17) + row[3];
            if (xw < 0 || xw >= W || yw < 0 || yw >= H) continue;  // outside the frame: dropped, for any table contents
            xo = (int)xw, yo = (int)yw;
        }
        // 0 <= t < T, 0 <= b < B, 0 <= yo < H, 0 <= xo < W, p in {0, 1}: inside the buffer for any event contents
        const int64_t cell = ((((int64_t)t * B + b) * H + yo) * W + xo) * 2 + p;
        if constexpr (REP == SNN_EVREP_BINARY) {
            frames[cell] = 1.0f;  // idempotent store: races are benign
        } else {
            unsigned int* acc = reinterpret_cast<unsigned int*>(frames);
            if constexpr (REP == SNN_EVREP_COUNT) {
                atomicAdd(acc + cell, 1u);
            } else {
                const uint64_t r = (uint64_t)d - (uint64_t)t * (uint64_t)step_us;   // 0 <= r < step_us
                if constexpr (REP == SNN_EVREP_TIME) {
                    atomicMax(acc + cell, (unsigned int)(r + 1));   // step_us <= 2^32 - 1 (checked by the launcher)
                } else {
                    // u = 2d - step_us = 2 t step_us + (2r - step_us):  k = t, rem = 2r - step_us in the second half of
                    // the bin, k = t - 1, rem = 2r + step_us in the first.  step_us < 2^40, so rem 2^16 < 2^57.
                    const uint64_t step = (uint64_t)step_us;
                    const bool late = 2 * r >= step;
                    const uint64_t rem = late ? 2 * r - step : 2 * r + step;
                    const unsigned int q = step < (1ull << 15) ? ((unsigned int)rem << 16) / (2u * (unsigned int)step)
                                                               : (unsigned int)((rem << 16) / (2 * step));   // < 2^16
                    const int k = late ? t : t - 1;   // -1 .. T - 1
                    const int64_t bin = (int64_t)B * H * W * 2;
                    const int64_t at = cell + (int64_t)(k - t) * bin;   // the same cell of bin k
                    if (k >= 0) atomicAdd(acc + at, 65536u - q);
                    if (k + 1 <= T - 1 && q > 0) atomicAdd(acc + at + bin, q);
                }
            }
        }
    }
}

// Accumulators -> values, in place: every operation one fp32 round-to-nearest (include/snn_hip.h states the three
// forms).  frames is 4-byte aligned only: the elements in front of the first 16-byte boundary and behind the last whole
// uint4 go one by one (block 0), the rest as 16-byte accesses.  `lim` is the clip on the accumulator (0xFFFFFFFF: none).
template <int REP>
__device__ __forceinline__ unsigned int rep_value(unsigned int a, unsigned int lim, float step_f, float scale) {
    float v;
    if constexpr (REP == SNN_EVREP_COUNT)
        v = (float)(a < lim ? a : lim);
    else if constexpr (REP == SNN_EVREP_TIME)
        v = __fdiv_rn((float)a, step_f);
    else
        v = __fmul_rn((float)(a < lim ? a : lim), 1.0f / 65536.0f);
    return __float_as_uint(__fmul_rn(v, scale));   // a = 0 stays +0.0f: scale is finite and positive
}

template <int REP>
__global__ __launch_bounds__(kThreads) void k_events_finalize(unsigned int* __restrict__ acc, int64_t n, unsigned int lim,
                                                              float step_f, float scale) {
    int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(acc) >> 2) & 3)) & 3);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 4;
    const int64_t tail = n - head - nvec * 4;   // 0 .. 3
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < head) acc[t] = rep_value<REP>(acc[t], lim, step_f, scale);
        else if (t >= 4 && t - 4 < tail) {
            unsigned int* q = acc + head + nvec * 4 + (t - 4);
            *q = rep_value<REP>(*q, lim, step_f, scale);
        }
    }
    uint4* vec = reinterpret_cast<uint4*>(acc + head);
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kThreads) {
        uint4 a = vec[v];
        a.x = rep_value<REP>(a.x, lim, step_f, scale), a.y = rep_value<REP>(a.y, lim, step_f, scale);
        a.z = rep_value<REP>(a.z, lim, step_f, scale), a.w = rep_value<REP>(a.w, lim, step_f, scale);
        vec[v] = a;
    }
}

// The boxes of the same transform.  One block per sample; a row is kept when enough of it stays visible and it stays
// large enough, the kept rows move to the front of the sample in their order (ballot + block scan), -1 rows behind.
__global__ __launch_bounds__(kThreads) void k_labels_aug(const float* __restrict__ in, float* __restrict__ out,
                                                         const int32_t* __restrict__ aug, int N, int width, float Wf,
                                                         float Hf, float min_visible, float min_size_px) {
    __shared__ int s_wave[kThreads / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* row = aug + (int64_t)b * 8;
    const bool flip = row[0] != 0;
    const float s = (float)row[1] * (1.0f / 65536.0f);
    const float dx = (float)row[2] / Wf, dy = (float)row[3] / Hf;
    const float* src = in + (int64_t)b * N * width;
    float* dst = out + (int64_t)b * N * width;
    const int c0 = width - 5;  // the class column
    int kept = 0;              // rows kept by the chunks before this one (block-uniform)
    for (int base = 0; base < N; base += kThreads) {
        const int i = base + threadIdx.x;
        float v[6];
        bool keep = false;
        if (i < N) {
            for (int c = 0; c < width; ++c) v[c] = src[(int64_t)i * width + c];
            if (v[c0] >= 0.0f) {
                float x1 = v[c0 + 1], y1 = v[c0 + 2], x2 = v[c0 + 3], y2 = v[c0 + 4];
                if (flip) {
                    const float f = x1;
                    x1 = 1.0f - x2;
                    x2 = 1.0f - f;
                }
                x1 = __fadd_rn(__fmul_rn(x1, s), dx), x2 = __fadd_rn(__fmul_rn(x2, s), dx);
                y1 = __fadd_rn(__fmul_rn(y1, s), dy), y2 = __fadd_rn(__fmul_rn(y2, s), dy);
                const float a0 = (x2 - x1) * (y2 - y1);
                x1 = fminf(fmaxf(x1, 0.0f), 1.0f), x2 = fminf(fmaxf(x2, 0.0f), 1.0f);
                y1 = fminf(fmaxf(y1, 0.0f), 1.0f), y2 = fminf(fmaxf(y2, 0.0f), 1.0f);
                const float w = x2 - x1, h = y2 - y1;
                keep = w * h >= min_visible * a0 && w * Wf >= min_size_px && h * Hf >= min_size_px;
                v[c0 + 1] = x1, v[c0 + 2] = y1, v[c0 + 3] = x2, v[c0 + 4] = y2;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = kept + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) pos += s_wave[w];
            total += s_wave[w];
        }
        if (keep)  // pos <= i < N
            for (int c = 0; c < width; ++c) dst[(int64_t)pos * width + c] = v[c];
        kept += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    for (int64_t k = (int64_t)kept * width + threadIdx.x; k < (int64_t)N * width; k += kThreads) dst[k] = -1.0f;
}

// ------------------------------------------------------------------------------------------ launch helpers
// What the two batch entry points do before they launch: their argument checks, in one order, and the zero fill.  `name`
// is the entry point in every text; `tables` / `events` say whether its table pointers / event pointers are there,
// `events_what` is its word for the latter, `misaligned` its alignment refusal (NULL: nothing to refuse).
int events_batch_prologue(const char* name, bool tables, bool events, const char* events_what, const char* misaligned,
                          int64_t n_events, float* frames, int T, int B, int H, int W, int64_t step_us,
                          hipStream_t stream) {
    SNN_REQUIRE(tables, "%s: null pointer", name);
    SNN_REQUIRE(T > 0 && B > 0 && H > 0 && W > 0 && n_events >= 0, "%s: bad shape", name);
    SNN_REQUIRE(step_us > 0, "%s: step_us must be positive, got %lld", name, (long long)step_us);
    SNN_REQUIRE(step_us <= INT64_MAX / T, "%s: T * step_us overflows 64 bits", name);
    // 2 T B H W < 2^31, asked without forming a product that could overflow
    SNN_REQUIRE((int64_t)T * B <= ((1ll << 30) - 1) / ((int64_t)H * W), "%s: a frame buffer of 2^31 elements or more",
                name);
    SNN_REQUIRE(n_events == 0 || events, "%s: null event %s", name, events_what);
    SNN_REQUIRE(!misaligned, "%s: %s", name, misaligned);
    const int64_t cells = (int64_t)T * B * H * W;
    hipError_t me = hipMemsetAsync(frames, 0, sizeof(float) * (size_t)cells * 2, stream);
    SNN_REQUIRE(me == hipSuccess, "%s: memset failed: %s", name, hipGetErrorString(me));
    return 0;
}

// What the kernels take of a representation: the clip range of each, and the step the time offset (uint32) and the
// voxel weight (rem 2^16 in 64 bits) are computed for.  The one statement of it: snn_events_rep_supported answers from it.
bool events_rep_ok(int rep, int64_t step_us, int clip) {
    if (step_us <= 0) return false;
    switch (rep) {
        case SNN_EVREP_BINARY: return clip == 0;
        case SNN_EVREP_COUNT: return clip >= 0 && clip <= (1 << 24);
        case SNN_EVREP_TIME: return clip == 0 && step_us <= 0xFFFFFFFFll;
        case SNN_EVREP_VOXEL: return clip >= 0 && clip <= 65535 && step_us < (1ll << 40);
    }
    return false;
}

// The refusals the *_rep entry points add to the prologue's, by name, before anything is touched.
int events_rep_check(const char* name, int rep, int clip, float scale, int64_t step_us, int64_t n_events) {
    SNN_REQUIRE(rep >= SNN_EVREP_BINARY && rep <= SNN_EVREP_VOXEL, "%s: unknown representation %d (0 binary, 1 count, "
                "2 time, 3 voxel)", name, rep);
    SNN_REQUIRE(std::isfinite(scale) && scale > 0.0f, "%s: scale must be finite and positive, got %g", name,
                (double)scale);
    SNN_REQUIRE(rep != SNN_EVREP_BINARY || scale == 1.0f, "%s: the binary representation takes scale 1 only, got %g",
                name, (double)scale);
    if (step_us > 0) {   // (a step_us <= 0 is the prologue's refusal)
        SNN_REQUIRE(events_rep_ok(rep, step_us, 0), "%s: step_us %lld is too large for this representation (time: at "
                    "most 2^32 - 1, voxel: below 2^40)", name, (long long)step_us);
        SNN_REQUIRE(events_rep_ok(rep, step_us, clip), "%s: clip %d is out of range for this representation (binary and "
                    "time: 0, count: 0 .. 2^24, voxel: 0 .. 65535)", name, clip);
    }
    SNN_REQUIRE(rep == SNN_EVREP_BINARY || n_events < (1ll << 32), "%s: n_events of 2^32 or more (the accumulators are "
                "32 bits wide)", name);
    return 0;
}

// The scatter of representation `rep` from `src` and, for the integer accumulators, the finalize pass behind it.
template <class Source>
void events_rep_launch(const Source src, const int64_t* offsets, const int64_t* t0, const int32_t* aug, int64_t n_events,
                       float* frames, int T, int B, int H, int W, int64_t step_us, int rep, int clip, float scale,
                       hipStream_t stream) {
    const dim3 grid(snn_grid_for(n_events, kThreads)), block(kThreads);
    const uint64_t window_us = (uint64_t)(step_us * T);
#define SNN_EVENTS_REP_CASE(REP)                                                                                        \
    case REP:                                                                                                           \
        if (aug)                                                                                                        \
            hipLaunchKernelGGL((k_events_batch<Source, true, REP>), grid, block, 0, stream, src, offsets, t0, aug,      \
                               n_events, frames, T, B, H, W, step_us, window_us);                                       \
        else                                                                                                            \
            hipLaunchKernelGGL((k_events_batch<Source, false, REP>), grid, block, 0, stream, src, offsets, t0, aug,     \
                               n_events, frames, T, B, H, W, step_us, window_us);                                       \
        break;
    switch (rep) {
        SNN_EVENTS_REP_CASE(SNN_EVREP_BINARY)
        SNN_EVENTS_REP_CASE(SNN_EVREP_COUNT)
        SNN_EVENTS_REP_CASE(SNN_EVREP_TIME)
        SNN_EVENTS_REP_CASE(SNN_EVREP_VOXEL)
    }
#undef SNN_EVENTS_REP_CASE
    if (rep == SNN_EVREP_BINARY) return;
    const int64_t n = (int64_t)T * B * H * W * 2;   // < 2^31 (the prologue)
    unsigned int* acc = reinterpret_cast<unsigned int*>(frames);
    const dim3 fgrid(snn_grid_for(snn_ceil_div(n, 4), kThreads));
    const float step_f = (float)step_us;   // fl(step_us)
    if (rep == SNN_EVREP_COUNT)
        hipLaunchKernelGGL(k_events_finalize<SNN_EVREP_COUNT>, fgrid, block, 0, stream, acc, n,
                           clip ? (unsigned int)clip : 0xFFFFFFFFu, step_f, scale);
    else if (rep == SNN_EVREP_TIME)
        hipLaunchKernelGGL(k_events_finalize<SNN_EVREP_TIME>, fgrid, block, 0, stream, acc, n, 0xFFFFFFFFu, step_f, scale);
    else
        hipLaunchKernelGGL(k_events_finalize<SNN_EVREP_VOXEL>, fgrid, block, 0, stream, acc, n,
                           clip ? (unsigned int)clip << 16 : 0xFFFFFFFFu, step_f, scale);
}

}  // namespace

// -------------------------------------------------------------------------------------------- C ABI
extern "C" int snn_events_to_frames(const int32_t* t_bin, const int32_t* x, const int32_t* y, const int32_t* p,
                                    int64_t n_events, float* frames, int T, int H, int W, void* stream) {
    SNN_REQUIRE(frames && T > 0 && H > 0 && W > 0 && n_events >= 0, "snn_events_to_frames: bad arguments");
    hipError_t me = hipMemsetAsync(frames, 0, sizeof(float) * (size_t)T * H * W * 2, (hipStream_t)stream);
    SNN_REQUIRE(me == hipSuccess, "snn_events_to_frames: memset failed: %s", hipGetErrorString(me));
    if (n_events == 0) return 0;
    SNN_REQUIRE(t_bin && x && y && p, "snn_events_to_frames: null event arrays");
    hipLaunchKernelGGL(k_events, dim3(snn_grid_for(n_events, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, t_bin,
                       x, y, p, n_events, frames, T, H, W);
    SNN_CHECK_LAUNCH("snn_events_to_frames");
    return 0;
}

extern "C" int snn_events_to_frames_aug(const int64_t* t_us, const int32_t* x, const int32_t* y, const int32_t* p,
                                        const int64_t* offsets, const int64_t* t0, const int32_t* aug,
                                        int64_t n_events, float* frames, int T, int B, int H, int W, int64_t step_us,
                                        void* stream) {
    if (int rc = events_batch_prologue("snn_events_to_frames_aug",
                                       frames && offsets && t0 && aug,   // tables: "null pointer" without one
                                       t_us && x && y && p, "arrays",    // events: "null event arrays"
                                       nullptr,                          // misaligned: this entry point asks nothing
                                       n_events, frames, T, B, H, W, step_us, (hipStream_t)stream))
        return rc;
    if (n_events == 0) return 0;
    hipLaunchKernelGGL((k_events_batch<TupleEvents, true>), dim3(snn_grid_for(n_events, kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, TupleEvents{t_us, x, y, p}, offsets, t0, aug, n_events, frames, T, B, H, W,
                       step_us, (uint64_t)(step_us * T));
    SNN_CHECK_LAUNCH("snn_events_to_frames_aug");
    return 0;
}

extern "C" int snn_events_to_frames_packed(const uint32_t* words, const int64_t* offsets, const int64_t* t0,
                                           const int32_t* aug, int64_t n_events, float* frames, int T, int B, int H,
                                           int W, int64_t step_us, void* stream) {
    const bool is_aligned = aligned(8, {words, offsets, t0}) && aligned(4, {aug, frames});
    if (int rc = events_batch_prologue(
            "snn_events_to_frames_packed",
            frames && offsets && t0,   // tables: "null pointer" without one (aug may be NULL: the identity)
            words, "words",            // events: "null event words"
            is_aligned ? nullptr : "words, offsets and t0 must be 8-byte aligned, aug and frames 4-byte aligned",
            n_events, frames, T, B, H, W, step_us, (hipStream_t)stream))
        return rc;
    if (n_events == 0) return 0;
    const PackedEvents src{reinterpret_cast<const uint2*>(words)};
    const dim3 grid(snn_grid_for(n_events, kThreads));
    const uint64_t window_us = (uint64_t)(step_us * T);
    if (aug)
        hipLaunchKernelGGL((k_events_batch<PackedEvents, true>), grid, dim3(kThreads), 0, (hipStream_t)stream, src,
                           offsets, t0, aug, n_events, frames, T, B, H, W, step_us, window_us);
    else
        hipLaunchKernelGGL((k_events_batch<PackedEvents, false>), grid, dim3(kThreads), 0, (hipStream_t)stream, src,
                           offsets, t0, aug, n_events, frames, T, B, H, W, step_us, window_us);
    SNN_CHECK_LAUNCH("snn_events_to_frames_packed");
    return 0;
}

extern "C" int snn_events_rep_supported(int rep, int64_t step_us, int clip) {
    return events_rep_ok(rep, step_us, clip) ? 1 : 0;
}

extern "C" int snn_events_to_frames_aug_rep(const int64_t* t_us, const int32_t* x, const int32_t* y, const int32_t* p,
                                            const int64_t* offsets, const int64_t* t0, const int32_t* aug,
                                            int64_t n_events, float* frames, int T, int B, int H, int W,
                                            int64_t step_us, int rep, int clip, float scale, void* stream) {
    const char* name = "snn_events_to_frames_aug_rep";
    if (int rc = events_rep_check(name, rep, clip, scale, step_us, n_events)) return rc;
    if (int rc = events_batch_prologue(name,
                                       frames && offsets && t0,          // tables (aug may be NULL: the identity)
                                       t_us && x && y && p, "arrays",    // events: "null event arrays"
                                       nullptr,                          // misaligned: this entry point asks nothing
                                       n_events, frames, T, B, H, W, step_us, (hipStream_t)stream))
        return rc;
    if (n_events == 0) return 0;
    events_rep_launch(TupleEvents{t_us, x, y, p}, offsets, t0, aug, n_events, frames, T, B, H, W, step_us, rep, clip,
                      scale, (hipStream_t)stream);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_events_to_frames_packed_rep(const uint32_t* words, const int64_t* offsets, const int64_t* t0,
                                               const int32_t* aug, int64_t n_events, float* frames, int T, int B,
                                               int H, int W, int64_t step_us, int rep, int clip, float scale,
                                               void* stream) {
    const char* name = "snn_events_to_frames_packed_rep";
    if (int rc = events_rep_check(name, rep, clip, scale, step_us, n_events)) return rc;
    const bool is_aligned = aligned(8, {words, offsets, t0}) && aligned(4, {aug, frames});
    if (int rc = events_batch_prologue(
            name,
            frames && offsets && t0,   // tables: "null pointer" without one (aug may be NULL: the identity)
            words, "words",            // events: "null event words"
            is_aligned ? nullptr : "words, offsets and t0 must be 8-byte aligned, aug and frames 4-byte aligned",
            n_events, frames, T, B, H, W, step_us, (hipStream_t)stream))
        return rc;
    if (n_events == 0) return 0;
    events_rep_launch(PackedEvents{reinterpret_cast<const uint2*>(words)}, offsets, t0, aug, n_events, frames, T, B, H,
                      W, step_us, rep, clip, scale, (hipStream_t)stream);
    SNN_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int snn_labels_augment(const float* labels_in, float* labels_out, const int32_t* aug, int B, int N, int width,
                                  int W, int H, float min_visible, float min_size_px, void* stream) {
    SNN_REQUIRE(B > 0 && N >= 0 && W > 0 && H > 0, "snn_labels_augment: bad shape");
    SNN_REQUIRE(width == 5 || width == 6, "snn_labels_augment: rows of %d columns (5 or 6)", width);
    if (N == 0) return 0;
    SNN_REQUIRE(labels_in && labels_out && aug, "snn_labels_augment: null pointer");
    SNN_REQUIRE(labels_in != labels_out, "snn_labels_augment: in place is not supported");
    hipLaunchKernelGGL(k_labels_aug, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, labels_in, labels_out, aug, N,
                       width, (float)W, (float)H, min_visible, min_size_px);
    SNN_CHECK_LAUNCH("snn_labels_augment");
    return 0;
}
