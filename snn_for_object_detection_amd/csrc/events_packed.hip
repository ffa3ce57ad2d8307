// Event voxelisation straight from the records of a Prophesee DAT recording: the scatter of k_events_aug
// (elementwise.hip) with the event fields unpacked in the kernel.  A record is 8 bytes - the timestamp in microseconds
// and one word holding x (bits 0-13), y (14-27) and the polarity (28) - and is read with one 8-byte load per lane, so a
// wave reads 512 contiguous bytes; include/snn_hip.h states the rules.  HBM-bound on the read, uncoalesced 4-byte
// stores by nature.
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsB = 64;   // batches up to this size keep offsets, window starts and the table in LDS

static unsigned grid_for(int64_t n) {
    int64_t b = snn_ceil_div(n, kThreads);
    if (b > snn_max_blocks()) b = snn_max_blocks();
    if (b < 1) b = 1;
    return (unsigned)b;
}

__device__ __forceinline__ uint32_t fmix32(uint32_t u) {   // murmur3's finaliser, as in k_events_aug
    u ^= u >> 16;
    u *= 0x85EBCA6Bu;
    u ^= u >> 13;
    u *= 0xC2B2AE35u;
    u ^= u >> 16;
    return u;
}

// AUG = false: no table is read (the identity), the field checks alone decide what is stored.
template <bool AUG>
__global__ __launch_bounds__(kThreads) void k_events_packed(
        const uint2* __restrict__ words, const int64_t* __restrict__ offsets, const int64_t* __restrict__ t0s,
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
        const uint2 rec = words[e];   // issued before the search: its latency hides behind the LDS reads
        int lo = 0, hi = B;  // the last sample whose slice starts at or before e (empty samples share a start)
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (off[mid] <= e) lo = mid; else hi = mid;
        }
        const int b = lo;
        const int64_t j = e - off[b];
        if (j < 0 || e >= off[b + 1]) continue;  // an event no slice owns
        // floor((t - t0) / step) in [0, T)  <=>  0 <= t - t0 < T * step; t is the 32-bit field zero-extended
        const int64_t d = (int64_t)((uint64_t)rec.x - (uint64_t)t0[b]);
        if (d < 0 || (uint64_t)d >= window_us) continue;
        const int t = narrow ? (int)((uint32_t)d / (uint32_t)step_us) : (int)(d / step_us);
        int x = (int)(rec.y & 0x3FFFu);
        const int y = (int)((rec.y >> 14) & 0x3FFFu), p = (int)((rec.y >> 28) & 1u);  // bits 29-31 are not read
        if (y >= H) continue;
        x = x > W - 1 ? W - 1 : x;
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
        // 0 <= t < T, 0 <= b < B, 0 <= yo < H, 0 <= xo < W, p in {0, 1}: inside the buffer for any word contents
        frames[((((int64_t)t * B + b) * H + yo) * W + xo) * 2 + p] = 1.0f;  // idempotent store: races are benign
    }
}

}  // namespace

extern "C" int snn_events_to_frames_packed(const uint32_t* words, const int64_t* offsets, const int64_t* t0,
                                           const int32_t* aug, int64_t n_events, float* frames, int T, int B, int H,
                                           int W, int64_t step_us, void* stream) {
    SNN_REQUIRE(frames && offsets && t0, "snn_events_to_frames_packed: null pointer");
    SNN_REQUIRE(T > 0 && B > 0 && H > 0 && W > 0 && n_events >= 0, "snn_events_to_frames_packed: bad shape");
    SNN_REQUIRE(step_us > 0, "snn_events_to_frames_packed: step_us must be positive, got %lld", (long long)step_us);
    SNN_REQUIRE(step_us <= INT64_MAX / T, "snn_events_to_frames_packed: T * step_us overflows 64 bits");
    // 2 T B H W < 2^31, asked without forming a product that could overflow
    SNN_REQUIRE((int64_t)T * B <= ((1ll << 30) - 1) / ((int64_t)H * W),
                "snn_events_to_frames_packed: a frame buffer of 2^31 elements or more");
    SNN_REQUIRE(n_events == 0 || words, "snn_events_to_frames_packed: null event words");
    SNN_REQUIRE(aligned(8, {words, offsets, t0}) && aligned(4, {aug, frames}),
                "snn_events_to_frames_packed: words, offsets and t0 must be 8-byte aligned, aug and frames 4-byte aligned");
    const int64_t cells = (int64_t)T * B * H * W;
    hipError_t me = hipMemsetAsync(frames, 0, sizeof(float) * (size_t)cells * 2, (hipStream_t)stream);
    SNN_REQUIRE(me == hipSuccess, "snn_events_to_frames_packed: memset failed: %s", hipGetErrorString(me));
    if (n_events == 0) return 0;
    const uint2* rec = reinterpret_cast<const uint2*>(words);
    const uint64_t window_us = (uint64_t)(step_us * T);
    if (aug)
        hipLaunchKernelGGL(k_events_packed<true>, dim3(grid_for(n_events)), dim3(kThreads), 0, (hipStream_t)stream, rec,
                           offsets, t0, aug, n_events, frames, T, B, H, W, step_us, window_us);
    else
        hipLaunchKernelGGL(k_events_packed<false>, dim3(grid_for(n_events)), dim3(kThreads), 0, (hipStream_t)stream, rec,
                           offsets, t0, aug, n_events, frames, T, B, H, W, step_us, window_us);
    SNN_CHECK_LAUNCH("snn_events_to_frames_packed");
    return 0;
}
