// Activity counts (gfx950): how many elements of a channels-last tensor src[T][M][ld] satisfy a predicate, per channel
// (and per timestep) - the spikes of a LIF layer from what its forward scan left (spike tensor, saved potentials, bit
// mask) and the non-zero operands of a convolution.  A streaming reduction bound by the read of src: nothing here touches
// the scans or the convolutions, and nothing is summed in floating point.
//
// One block holds a tile of LX channel groups (a power of two, LX consecutive lanes = consecutive addresses of one pixel
// row) by 1024 / LX pixel rows and walks down its `rows` rows of one timestep with per-lane 32-bit counters.  Lanes of a
// wave that hold the same channels are then combined across lanes, the waves of the block through LDS, and one lane per
// channel issues ONE 64-bit integer atomic add per (block, timestep, channel): integer sums are exact in any order.
#include "snn_common.h"
#include <algorithm>

namespace {

// One block of 16 waves per compute unit: what a kernel of this kind pays for, besides its reads, is the number of adders
// per count - with 256-thread blocks, four to a compute unit, the 1024 blocks of a layer-sized call that sums over the
// timesteps spent as long on their atomics (65 us) as on a third of their reads.
constexpr int kThreads = 1024;
constexpr int kWave = 64;
constexpr int kMinPasses = 16;    // passes of a block over its tile at the least: what amortises the block's reduction
constexpr int kMaskMaxLX = 16;    // mask words per row and block (512 channels): LX / 2 counters per lane
constexpr int64_t kMaxRows = 1 << 30;   // per block: a 32-bit counter holds at most one count per row

struct ActPlan {
    int vec;      // channels per access: 4 / 1; mask: 32 (one word)
    int lx;       // channel groups (of vec channels) side by side in a block
    int chunks;   // blocks side by side over the channels
    int64_t rows; // pixel rows per block
    int64_t gx, gy;   // grid: row blocks; T * chunks
};

static int pow2_at_least(int64_t n) {
    int p = 1;
    while (p < n && p < kThreads) p <<= 1;
    return p;
}

static ActPlan act_plan(int kind, int T, int64_t M, int C, bool vec4) {
    ActPlan p;
    const bool mask = kind == SNN_ACT_MASK;
    p.vec = mask ? 32 : (vec4 ? 4 : 1);
    const int64_t groups = C / p.vec;
    p.lx = pow2_at_least(groups);
    if (mask && p.lx > kMaskMaxLX) p.lx = kMaskMaxLX;
    p.chunks = (int)snn_ceil_div(groups, p.lx);
    const int ry = kThreads / p.lx;
    p.gy = (int64_t)T * p.chunks;
    // fill the chip (one block = 16 waves per compute unit, each lane with four loads in flight), but never with blocks
    // that see fewer than kMinPasses passes: all blocks are resident at once and reach their atomics together
    const int64_t want = std::max<int64_t>(1, (int64_t)snn_num_cu() / p.gy);
    int64_t rows = std::max<int64_t>(snn_ceil_div(M, want), (int64_t)kMinPasses * ry);
    rows = std::min<int64_t>(snn_ceil_div(rows, ry) * ry, kMaxRows);
    p.rows = rows;
    p.gx = snn_ceil_div(M, rows);
    return p;
}

// the predicate on the fp32 bit pattern of an element (a bf16 element is the upper half of one)
template <bool ABOVE> __device__ __forceinline__ unsigned act_hit(unsigned bits, float th) {
    if constexpr (ABOVE) return __builtin_bit_cast(float, bits) > th ? 1u : 0u;   // strict; NaN is not above
    else return (bits & 0x7fffffffu) != 0u ? 1u : 0u;                             // -0.0 is zero; NaN, denormals are not
}

template <int VEC, bool BF> struct ActLoad;
template <> struct ActLoad<4, false> {
    typedef unsigned raw __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ unsigned bits(raw r, int j) { return r[j]; }
};
template <> struct ActLoad<4, true> {
    typedef snn_u32x2 raw;
    static __device__ __forceinline__ unsigned bits(raw r, int j) { return (j & 1) ? (r[j >> 1] & 0xffff0000u) : (r[j >> 1] << 16); }
};
template <> struct ActLoad<1, false> {
    typedef unsigned raw;
    static __device__ __forceinline__ unsigned bits(raw r, int) { return r; }
};
template <> struct ActLoad<1, true> {
    typedef unsigned short raw;
    static __device__ __forceinline__ unsigned bits(raw r, int) { return (unsigned)r << 16; }
};

// VEC channels per access; BF: bf16 elements; ABOVE: x > th, else x != 0.  lx = 1 << lx_log2.
template <int VEC, bool BF, bool ABOVE>
__global__ __launch_bounds__(kThreads) void k_activity_count(const void* __restrict__ src, int64_t ld, float th, int64_t M,
                                                             int C, int lx_log2, int chunks, int64_t rows, int per_step,
                                                             unsigned long long* __restrict__ counts) {
    typedef ActLoad<VEC, BF> L;
    typedef typename L::raw Raw;
    constexpr int ES = BF ? 2 : 4;
    const int lx = 1 << lx_log2;
    const int tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2, ry = kThreads >> lx_log2;
    const int t = blockIdx.y / chunks, chunk = blockIdx.y % chunks;
    const int c = (chunk * lx + tx) * VEC;
    const bool live = c < C;   // (VEC == 4: C % 4 == 0, so a live group is whole)
    const int64_t row0 = (int64_t)blockIdx.x * rows;
    const int64_t n = rows < M - row0 ? rows : M - row0;
    unsigned cnt[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) cnt[j] = 0;
    if (live) {
        const char* base = static_cast<const char*>(src) + (((int64_t)t * M + row0) * ld + c) * ES;
        const int64_t pitch = ld * ES;
        int64_t r = ty;
        // four independent loads in flight per lane, no bound check between them
        for (; r + 3 * (int64_t)ry < n; r += 4 * (int64_t)ry) {
            Raw v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const Raw*>(base + (r + (int64_t)k * ry) * pitch);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) cnt[j] += act_hit<ABOVE>(L::bits(v[k], j), th);
            }
        }
        for (; r < n; r += ry) {
            const Raw v = *reinterpret_cast<const Raw*>(base + r * pitch);
#pragma unroll
            for (int j = 0; j < VEC; ++j) cnt[j] += act_hit<ABOVE>(L::bits(v, j), th);
        }
    }
    // lanes of a wave with the same tx (lx < 64): butterfly over the lane bits above lx
    for (int off = kWave / 2; off >= lx; off >>= 1) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) cnt[j] += (unsigned)__shfl_xor((int)cnt[j], off);
    }
    // ... then the waves (lx < 64: lane tx of each of the 16 holds the wave's sum) or the block's ry thread rows (lx >= 64)
    __shared__ unsigned sm[kThreads * VEC];
    const int lane = threadIdx.x & (kWave - 1);
    const bool narrow = lx < kWave;
    const int group = narrow ? (int)(threadIdx.x / kWave) : ty;
    const int ngroups = narrow ? kThreads / kWave : ry;
    if (!narrow || lane < lx) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) sm[(group * lx + tx) * VEC + j] = cnt[j];
    }
    __syncthreads();
    // one thread per channel of the tile, consecutive threads on consecutive counts: a wave's atomic is 512 contiguous bytes
    unsigned long long* dst = counts + (per_step ? (int64_t)t * C : 0) + (int64_t)chunk * lx * VEC;
    const int tile = lx * VEC;
    for (int i = threadIdx.x; i < tile && chunk * tile + i < C; i += kThreads) {
        unsigned long long total = 0;
        for (int g = 0; g < ngroups; ++g) total += sm[g * tile + i];
        if (total) atomicAdd(dst + i, total);
    }
}

// lanes k = col (mod LX) of a wave
template <int LX> constexpr unsigned long long act_column_pattern() {
    unsigned long long p = 0;
    for (int k = 0; k < kWave; k += LX) p |= 1ull << k;
    return p;
}

// The bit mask: one lane loads one word (32 channels of one pixel), LX word columns side by side.  Bit b of all 64 words
// of a wave is one __ballot; lane j keeps the ballot of bit j % 32 and counts, by __popcll under the column's lane
// pattern, the columns j / 32, j / 32 + 2, ...: LX / 2 counters per lane (one for LX <= 2), not 32.
template <int LX>
__global__ __launch_bounds__(kThreads) void k_activity_count_mask(const uint32_t* __restrict__ src, int64_t ld, int64_t M,
                                                                  int C, int chunks, int64_t rows, int per_step,
                                                                  unsigned long long* __restrict__ counts) {
    constexpr int RY = kThreads / LX;
    constexpr int NC = LX >= 2 ? LX / 2 : 1;
    constexpr unsigned long long kPat = act_column_pattern<LX>();
    const int tx = threadIdx.x % LX, ty = threadIdx.x / LX;
    const int t = blockIdx.y / chunks, chunk = blockIdx.y % chunks;
    const int words = C / 32;
    const bool live = chunk * LX + tx < words;   // words past C / 32 (ld > C / 32) are never loaded
    const int64_t row0 = (int64_t)blockIdx.x * rows;
    const int64_t n = rows < M - row0 ? rows : M - row0;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int b = lane & 31, h = lane >> 5;
    const uint32_t* base = src + ((int64_t)t * M + row0) * ld + chunk * LX + tx;
    unsigned cnt[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) cnt[q] = 0;
    // (the trip count is the same for every lane: __ballot needs the whole wave)
    for (int64_t r0 = 0; r0 < n; r0 += 4 * RY) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t r = r0 + (int64_t)k * RY + ty;
            w[k] = (live && r < n) ? base[r * ld] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned long long mine = 0;
#pragma unroll
            for (int bit = 0; bit < 32; ++bit) {
                const unsigned long long bal = __ballot((w[k] >> bit) & 1u);
                mine = (b == bit) ? bal : mine;
            }
#pragma unroll
            for (int q = 0; q < NC; ++q) cnt[q] += (unsigned)__popcll(mine & (kPat << (LX >= 2 ? h + 2 * q : 0)));
        }
    }
    __shared__ unsigned sm[(kThreads / kWave) * LX * 32];   // [wave][column][bit]
    if (LX >= 2 || h == 0) {
#pragma unroll
        for (int q = 0; q < NC; ++q) sm[(wave * LX + (LX >= 2 ? h + 2 * q : 0)) * 32 + b] = cnt[q];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LX * 32; i += kThreads) {
        const int wc = chunk * LX + (i >> 5);
        if (wc >= words) continue;
        unsigned long long total = 0;
#pragma unroll
        for (int wv = 0; wv < kThreads / kWave; ++wv) total += sm[wv * LX * 32 + i];
        if (total) atomicAdd(counts + (per_step ? (int64_t)t * C : 0) + (int64_t)wc * 32 + (i & 31), total);
    }
}

// what both entry points refuse, under the name of the one that was called
static int act_check(const char* fn, int kind, int T, int64_t M, int C, int64_t ld) {
    SNN_REQUIRE(kind >= SNN_ACT_NONZERO_F32 && kind <= SNN_ACT_MASK, "%s: unknown kind %d", fn, kind);
    SNN_REQUIRE(T > 0 && M > 0 && C > 0, "%s: non-positive shape (T %d, M %lld, C %d)", fn, T, (long long)M, C);
    const bool mask = kind == SNN_ACT_MASK;
    SNN_REQUIRE(!mask || C % 32 == 0, "%s: a mask holds whole words: C %% 32 != 0 (C %d)", fn, C);
    SNN_REQUIRE(ld >= (mask ? C / 32 : C), "%s: ld too small (%lld for %d %s)", fn, (long long)ld, mask ? C / 32 : C,
                mask ? "words" : "channels");
    return 0;
}

static bool act_vec4(int kind, int C, int64_t ld, bool ptr_aligned) {
    return kind != SNN_ACT_MASK && multiples(4, {C, ld}) && ptr_aligned;
}

static int act_grid_ok(const char* fn, const ActPlan& p) {
    SNN_REQUIRE(p.gx <= 0x7fffffffLL && p.gy <= 65535, "%s: shape too large for one launch (grid %lld x %lld)", fn,
                (long long)p.gx, (long long)p.gy);
    return 0;
}

}  // namespace

extern "C" int snn_activity_count_plan(int kind, int T, int64_t M, int C, int64_t ld, int aligned_ptr, int64_t* out) {
    const char* const fn = "snn_activity_count_plan";
    SNN_REQUIRE(out, "%s: null pointer", fn);
    if (int rc = act_check(fn, kind, T, M, C, ld)) return rc;
    const ActPlan p = act_plan(kind, T, M, C, act_vec4(kind, C, ld, aligned_ptr != 0));
    if (int rc = act_grid_ok(fn, p)) return rc;
    out[0] = p.vec;
    out[1] = p.rows;
    out[2] = p.gx;
    out[3] = p.gy;
    return 0;
}

extern "C" int snn_activity_count(const void* src, int kind, int64_t ld, float threshold, int T, int64_t M, int C,
                                  int per_step, int64_t* counts, int accumulate, void* stream) {
    const char* const fn = "snn_activity_count";
    SNN_REQUIRE(src && counts, "%s: null pointer", fn);
    if (int rc = act_check(fn, kind, T, M, C, ld)) return rc;
    const bool bf = kind == SNN_ACT_NONZERO_BF16 || kind == SNN_ACT_ABOVE_BF16;
    const bool above = kind == SNN_ACT_ABOVE_F32 || kind == SNN_ACT_ABOVE_BF16;
    const ActPlan p = act_plan(kind, T, M, C, act_vec4(kind, C, ld, aligned(bf ? 8 : 16, {src})));
    if (int rc = act_grid_ok(fn, p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)C * (per_step ? (size_t)T : 1), st);
        SNN_REQUIRE(e == hipSuccess, "%s: clearing the counts failed: %s", fn, hipGetErrorString(e));
    }
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(counts);
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    bool launched;
    if (kind == SNN_ACT_MASK) {
        launched = dispatch(
            [&](auto LX) {
                hipLaunchKernelGGL((k_activity_count_mask<LX()>), grid, dim3(kThreads), 0, st,
                                   static_cast<const uint32_t*>(src), ld, M, C, p.chunks, p.rows, per_step, dst);
                return true;
            },
            OneOf<1, 2, 4, 8, 16>{p.lx});
    } else {
        int lx_log2 = 0;
        while ((1 << lx_log2) < p.lx) ++lx_log2;
        launched = dispatch(
            [&](auto VEC, auto BF, auto ABOVE) {
                hipLaunchKernelGGL((k_activity_count<VEC(), BF(), ABOVE()>), grid, dim3(kThreads), 0, st, src, ld, threshold,
                                   M, C, lx_log2, p.chunks, p.rows, per_step, dst);
                return true;
            },
            OneOf<1, 4>{p.vec}, Flag{bf}, Flag{above});
    }
    SNN_REQUIRE(launched, "%s: no kernel instance (kind %d, %d channels per access)", fn, kind, p.vec);
    SNN_CHECK_LAUNCH(fn);
    return 0;
}
