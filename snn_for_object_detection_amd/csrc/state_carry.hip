// Carried detector state (training on consecutive windows of a recording): put the samples that start a new recording
// back to rest in EVERY tensor of the state tree with one launch.  Which samples those are is device data (first[B]),
// so the host never asks: a block whose sample goes on returns after one 4-byte load.
#include "snn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunks = 16;    // blocks per (tensor, sample); each walks its share of the block with stride kChunks * kThreads
constexpr int kRowWords = 3;   // int64 per table row: address, fp32 elements per sample, rest value (fp32 bits, low word)

// grid (chunk, sample, tensor).  A sample's block is n consecutive floats at base + b * n, 4-byte aligned only: the
// floats in front of the first 16-byte boundary and behind the last whole float4 are stored one by one (by chunk 0), the
// rest as float4.
__global__ void k_state_reset(const int64_t* __restrict__ table, const int32_t* __restrict__ first) {
    const int b = blockIdx.y;
    if (first[b] == 0) return;
    const int64_t* row = table + (int64_t)blockIdx.z * kRowWords;
    const int64_t n = row[1];
    float* base = reinterpret_cast<float*>(row[0]) + (int64_t)b * n;
    const float rest = __int_as_float((int)(row[2] & 0xffffffff));
    int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(base) >> 2) & 3)) & 3);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 4;
    const int64_t tail = n - head - nvec * 4;   // 0 .. 3
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < head) base[t] = rest;
        else if (t >= 4 && t - 4 < tail) base[head + nvec * 4 + (t - 4)] = rest;
    }
    float4* vec = reinterpret_cast<float4*>(base + head);
    const float4 r4 = make_float4(rest, rest, rest, rest);
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += (int64_t)kChunks * kThreads) vec[v] = r4;
}

}  // namespace

extern "C" int snn_state_reset(const int64_t* table, int n, int B, const int32_t* first, void* stream) {
    SNN_REQUIRE(table && first && n > 0 && B > 0, "snn_state_reset: bad arguments");
    SNN_REQUIRE(n <= 65535 && B <= 65535, "snn_state_reset: more than 65535 tensors or samples");
    hipLaunchKernelGGL(k_state_reset, dim3(kChunks, (unsigned)B, (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream,
                       table, first);
    SNN_CHECK_LAUNCH("snn_state_reset");
    return 0;
}
