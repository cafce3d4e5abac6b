// The ranks behind a bitmap, for every operator that numbers what it finds:
// the exclusive scan of a uint32 array on the device, in place, the rank of a set bit read off
// the scanned counts, and the arena views of such a table.  Not part of the C ABI.
// The scan: sums, one workgroup per chunk adds its chunk up; one, the one workgroup over the
// chunk sums; apply, the scan inside each chunk plus its offset.  Integer adds only: exact.
// The zonal statistics, the stream network and the depressions scan their word counts with all
// three; the watersheds scan a count per tile with `one` alone.
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

// count[0 .. n) becomes its exclusive scan, by one workgroup: one launch on `stream`.  For the
// chunk sums below and for counts that are few (one per tile).
static inline void hdem_scan_exclusive_small(hipStream_t stream, uint32_t *count, int64_t n)
{
    hipLaunchKernelGGL(hdem_scan_one_kernel, dim3(1), dim3(HDEM_SCAN_ONE_NT), 0, stream, count, n);
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
    hdem_scan_exclusive_small(stream, sums, chunks);
    hipLaunchKernelGGL(hdem_scan_apply_kernel, dim3((unsigned)chunks), dim3(HDEM_SCAN_NT), 0,
                       stream, count, n, sums);
}

// The rank of bit sh of a word b whose scanned count is `before`: the set bits in front of it.
__device__ __forceinline__ uint32_t hdem_rank_in(unsigned long long b, int sh, uint32_t before)
{
    return before + (uint32_t)__popcll(b & ((1ull << sh) - 1ull));
}
// The rank of bit sh of word w, or false: the bit is not set or its rank is not below K.
__device__ __forceinline__ bool hdem_rank_of(const unsigned long long *__restrict__ bits,
                                             const uint32_t *__restrict__ before, size_t w, int sh,
                                             uint32_t K, uint32_t &r)
{
    const unsigned long long b = bits[w];
    if (!((b >> sh) & 1ull)) return false;
    r = hdem_rank_in(b, sh, before[w]);
    return r < K;
}

// The table behind those ranks as views of an arena: bits u64 per word | counts u32 per word
// (the scan turns them into `before`) | chunk sums u32, each view 16-byte aligned.
struct hdem_rank_table {
    unsigned long long *bits;
    uint32_t *count, *sums;
};
static inline size_t hdem_rank_table_bytes(int64_t words)
{
    return hdem_round16((size_t)words * 8) + hdem_round16((size_t)words * 4) +
           hdem_round16((size_t)hdem_scan_chunks(words) * 4);
}
// at: 16-byte aligned, with hdem_rank_table_bytes(words) bytes behind it
static inline void hdem_rank_table_at(char *at, int64_t words, hdem_rank_table *t)
{
    t->bits = reinterpret_cast<unsigned long long *>(at), at += hdem_round16((size_t)words * 8);
    t->count = reinterpret_cast<uint32_t *>(at), at += hdem_round16((size_t)words * 4);
    t->sums = reinterpret_cast<uint32_t *>(at);
}
