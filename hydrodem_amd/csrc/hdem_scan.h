// Exclusive scan of a uint32 array on the device, in place: the ranks
// behind a bitmap.  Not part of the C ABI.  sums: one workgroup per chunk adds its chunk up;
// one: the one workgroup over the chunk sums; apply: the scan inside each chunk plus its offset.
// Integer adds only: exact.  hdem_depressions.hip and hdem_streamnet.hip hold older private
// copies of these three kernels.
#pragma once

#include "hdem_internal.h"

constexpr int HDEM_SCAN_NT = 256;
constexpr int HDEM_SCAN_PER = 16;          // elements per thread
constexpr int HDEM_SCAN_CHUNK = HDEM_SCAN_NT * HDEM_SCAN_PER;
constexpr int HDEM_SCAN_ONE_NT = 1024;     // the one workgroup over the chunk sums

static __global__ __launch_bounds__(HDEM_SCAN_NT) void hdem_scan_sums_kernel(
    const uint32_t *__restrict__ count, int64_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * HDEM_SCAN_CHUNK;
    uint32_t sum = 0;
    for (int k = 0; k < HDEM_SCAN_PER; ++k) {
        const int64_t i = lo + k * HDEM_SCAN_NT + threadIdx.x;
        if (i < n) sum += count[i];
    }
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s_sum;
}

static __global__ __launch_bounds__(HDEM_SCAN_ONE_NT) void hdem_scan_one_kernel(
    uint32_t *__restrict__ sums, int64_t n)
{
    __shared__ uint32_t part[HDEM_SCAN_ONE_NT];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + HDEM_SCAN_ONE_NT - 1) / HDEM_SCAN_ONE_NT;
    const int64_t lo = tid * chunk < n ? tid * chunk : n;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    uint32_t sum = 0;
    for (int64_t t = lo; t < hi; ++t) sum += sums[t];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < HDEM_SCAN_ONE_NT; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (int64_t t = lo; t < hi; ++t) {
        const uint32_t v = sums[t];
        sums[t] = run;
        run += v;
    }
}

static __global__ __launch_bounds__(HDEM_SCAN_NT) void hdem_scan_apply_kernel(
    uint32_t *__restrict__ count, int64_t n, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t part[HDEM_SCAN_NT];
    const int tid = threadIdx.x;
    // a thread takes HDEM_SCAN_PER consecutive elements
    const int64_t lo = (int64_t)blockIdx.x * HDEM_SCAN_CHUNK + (int64_t)tid * HDEM_SCAN_PER;
    uint32_t v[HDEM_SCAN_PER];
    uint32_t sum = 0;
    for (int k = 0; k < HDEM_SCAN_PER; ++k) {
        v[k] = lo + k < n ? count[lo + k] : 0u;
        sum += v[k];
    }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < HDEM_SCAN_NT; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t run = sums[blockIdx.x] + part[tid] - sum;
    for (int k = 0; k < HDEM_SCAN_PER; ++k) {
        if (lo + k < n) count[lo + k] = run;
        run += v[k];
    }
}

// chunk sums that a scan of n elements needs room for
static inline int64_t hdem_scan_chunks(int64_t n)
{
    return (n + HDEM_SCAN_CHUNK - 1) / HDEM_SCAN_CHUNK;
}

// count[0 .. n) becomes its exclusive scan; sums: hdem_scan_chunks(n) words of scratch.
// Three launches on `stream`, no synchronisation.
static inline void hdem_scan_exclusive(hipStream_t stream, uint32_t *count, int64_t n,
                                       uint32_t *sums)
{
    const int64_t chunks = hdem_scan_chunks(n);
    if (n <= 0) return;
    hipLaunchKernelGGL(hdem_scan_sums_kernel, dim3((unsigned)chunks), dim3(HDEM_SCAN_NT), 0,
                       stream, count, n, sums);
    hipLaunchKernelGGL(hdem_scan_one_kernel, dim3(1), dim3(HDEM_SCAN_ONE_NT), 0, stream, sums,
                       chunks);
    hipLaunchKernelGGL(hdem_scan_apply_kernel, dim3((unsigned)chunks), dim3(HDEM_SCAN_NT), 0,
                       stream, count, n, sums);
}
