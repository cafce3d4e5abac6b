// Zonal statistics: one row per zone of a label raster (new operator; ZonalStatistics,
// DemToBasins).
//
// In: zones, a uint32 H x W raster (0: no zone, ids in 1 ... H * W), and optionally a raster of
// values (float32, uint32 or uint8).  The K ids present are numbered 0 ... K - 1 in ascending
// order; row r of every column describes the r-th id.
//   1  (zonal_mark_kernel, zonal_popc_kernel, hdem_scan.h)  ranks.  One bit per id in 64-bit
//      words.  A workgroup per 64 x 64 tile; a wave is a tile row, and only the first lane of a
//      run of equal ids goes on; those put their id into a set in LDS (open addressing, 4 096
//      slots >= the ids of a tile), and the lane that put it there sets the bit: one global
//      atomicOr per (tile, zone) at most.  Then the count per word, K as their sum, and the
//      exclusive scan: rank(id) = scanned count of its word + popcount of the bits in front.
//   2  (zonal_tile_kernel)  per tile again.  What the lanes of a run add is reduced inside the
//      wave first (the counts, the box and `first` follow from the run's two ends; the values
//      take a segmented shuffle reduction), the run's first lane looks the rank up and adds the
//      run to the tile's table in LDS (open addressing, SLOTS slots, PROBES probes), then one
//      global atomic per (tile, row, column) that has something to add.  A run that finds no
//      slot within PROBES probes adds to the global columns directly and is counted
//      (`overflow`): a tile with more zones than slots is legal and exact, only slower.
//      Instantiated without values (28 B per slot) and once per value type (56 B per slot).
//      min / max are gathered as one 64-bit word each: the order-preserving key of the value in
//      the high half, the flat index in the low half (min), its complement (max), so that ties
//      go to the smallest index under atomicMin / atomicMax.
//   3  (zonal_final_kernel, zonal_id_kernel)  min, max, at_min, at_max out of the packed words;
//      the ids out of the bitmap.
// Counts, mins, maxs and integer sums only: exact, independent of the schedule.  No walk: the
// probe loops are capped (the set's at its size, which a tile cannot fill: reaching it is
// counted and refused).  A rank is compared with K before it indexes a column, so a wrong K
// writes nowhere.  -DHDEM_ZONAL_PLAIN: step 2 without the run reduction and the table, global
// atomics cell by cell (the comparison build of DESIGN 3.18).
// Workspace (arena): 12 B per 64 cells (bitmap + counts), 16 B per zone when min, max, at_min
// or at_max is wanted.
#include "hdem_d8tile.h"
#include "hdem_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int NT = 256;               // threads per workgroup
constexpr int MARK_SLOTS = 4096;      // the id set of the mark kernel: a tile holds 4 096 ids
constexpr int SLOTS = 512;            // table slots of the tile kernel
constexpr int SLOT_BITS = 9;
constexpr int PROBES = 16;            // then the run takes the global path
constexpr size_t HEAD = 256;          // bytes of the counter block
constexpr uint32_t NONE = 0xFFFFFFFFu;
static_assert(SLOTS == 1 << SLOT_BITS, "the hash takes the top SLOT_BITS bits");
static_assert(TS == 64, "a tile row is a wave and a word of the box masks");

struct zonal_counters {
    u64 zones;                        // ids present
    u64 unzoned;                      // cells with id 0
    u64 over;                         // cells with an id above H * W
    u64 clamped;                      // float cells whose q(v) was clamped
    u64 overflow;                     // cells that took the global path of the tile pass
    u64 capped;                       // inserts into the id set that found no slot
    u64 foreign;                      // runs whose rank is not below K
    unsigned int max_id;
};
static_assert(sizeof(zonal_counters) <= HEAD, "counters outgrew their block");

__device__ __forceinline__ unsigned int wave_sum(unsigned int v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// 1.  The bit of every id present.  bits is zero on entry.
__global__ __launch_bounds__(NT) void zonal_mark_kernel(const uint32_t *__restrict__ zones, int H,
                                                        int W, int tiles_x, uint32_t cells,
                                                        u64 *__restrict__ bits,
                                                        zonal_counters *__restrict__ cnt)
{
    __shared__ uint32_t s_set[MARK_SLOTS];
    __shared__ unsigned int s_cnt[4];            // unzoned, over, capped, max id
    const int tid = threadIdx.x, lane = tid & 63;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 4) s_cnt[tid] = 0;
    for (int s = tid; s < MARK_SLOTS; s += NT) s_set[s] = 0u;
    __syncthreads();

    unsigned int unzoned = 0, over = 0, capped = 0, largest = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= tile.th) break;                // (whole waves: a wave is a row)
        const bool inside = lx < tile.tw;
        uint32_t id = 0;
        if (inside) id = zones[(size_t)(tile.y0 + ly) * W + tile.x0 + lx];
        unzoned += inside && id == 0u;
        over += id > cells;
        largest = max(largest, id);
        const uint32_t z = id > cells ? 0u : id;
        const uint32_t before = __shfl_up(z, 1);
        if (z && (lane == 0 || z != before)) {   // the first lane of a run
            uint32_t slot = (z * 2654435761u) >> 20;             // 12 bits
            int probe = 0;
            for (; probe < MARK_SLOTS; ++probe) {
                const uint32_t seen = atomicCAS(&s_set[slot], 0u, z);
                if (seen == 0u) atomicOr(&bits[(z - 1u) >> 6], 1ull << ((z - 1u) & 63u));
                if (seen == 0u || seen == z) break;
                slot = (slot + 1) & (MARK_SLOTS - 1);
            }
            capped += probe == MARK_SLOTS;       // more ids than cells: not from this kernel
        }
    }
    unzoned = wave_sum(unzoned), over = wave_sum(over), capped = wave_sum(capped);
    for (int m = 32; m >= 1; m >>= 1) largest = max(largest, (unsigned int)__shfl_xor(largest, m));
    if (lane == 0) {
        if (unzoned) atomicAdd(&s_cnt[0], unzoned);
        if (over) atomicAdd(&s_cnt[1], over);
        if (capped) atomicAdd(&s_cnt[2], capped);
        atomicMax(&s_cnt[3], largest);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->unzoned, (u64)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->over, (u64)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->capped, (u64)s_cnt[2]);
        if (s_cnt[3]) atomicMax(&cnt->max_id, s_cnt[3]);
    }
}

__global__ __launch_bounds__(NT) void zonal_popc_kernel(int64_t words, const u64 *__restrict__ bits,
                                                        uint32_t *__restrict__ count,
                                                        zonal_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * NT + threadIdx.x;
    unsigned int n = 0;
    if (w < words) count[w] = n = (unsigned int)__popcll(bits[w]);
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_sum, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(&cnt->zones, (u64)s_sum);
}

// The row of id z (1 ... cells), or false: its bit is not set or its rank is not below K.
__device__ __forceinline__ bool row_of(uint32_t z, uint32_t K, const u64 *__restrict__ bits,
                                       const uint32_t *__restrict__ before, uint32_t &r)
{
    const uint32_t at = z - 1u;
    return hdem_rank_of(bits, before, at >> 6, (int)(at & 63u), K, r);
}

// 2.  The columns the tile pass adds to (null: not wanted) and what a run, a cell or a slot adds.
struct zonal_cols {
    uint32_t *count, *first, *row_min, *row_max, *col_min, *col_max, *valid;
    u64 *pmin, *pmax, *sum;
};
struct zonal_add {
    uint32_t count, first, valid;
    u64 rows, cols;                   // the tile rows and columns touched, one bit each
    u64 pmin, pmax, sum;
};

__device__ __forceinline__ void add_global(const zonal_cols &c, size_t r, int y0, int x0,
                                           const zonal_add &a)
{
    if (c.count) atomicAdd(&c.count[r], a.count);
    if (c.first) atomicMin(&c.first[r], a.first);
    if (c.row_min) atomicMin(&c.row_min[r], (uint32_t)(y0 + __builtin_ctzll(a.rows)));
    if (c.row_max) atomicMax(&c.row_max[r], (uint32_t)(y0 + 63 - __builtin_clzll(a.rows)));
    if (c.col_min) atomicMin(&c.col_min[r], (uint32_t)(x0 + __builtin_ctzll(a.cols)));
    if (c.col_max) atomicMax(&c.col_max[r], (uint32_t)(x0 + 63 - __builtin_clzll(a.cols)));
    if (c.valid && a.valid) atomicAdd(&c.valid[r], a.valid);
    if (c.pmin && a.pmin != ~0ull) atomicMin(&c.pmin[r], a.pmin);
    if (c.pmax && a.pmax != 0ull) atomicMax(&c.pmax[r], a.pmax);
    if (c.sum && a.sum) atomicAdd(&c.sum[r], a.sum);
}

// The value of cell g: false for a NaN.  key: its order-preserving key; q: what it adds to the
// sum (two's complement); clamped: q(v) hit its bound.
template <int VT>
__device__ __forceinline__ bool value_of(const void *__restrict__ values, size_t g, double scale,
                                         uint32_t &key, u64 &q, unsigned int &clamped)
{
    if (VT == HDEM_ZONAL_F32) {
        const float f = static_cast<const float *>(values)[g];
        if (f != f) return false;
        key = key_of(f);
        double d = rint((double)f * scale);      // exact product, one rounding to nearest even
        const double bound = 2147483647.0;
        if (d > bound) d = bound, ++clamped;
        if (d < -bound) d = -bound, ++clamped;
        q = (u64)(long long)d;
    } else if (VT == HDEM_ZONAL_U32) {
        key = static_cast<const uint32_t *>(values)[g];
        q = key;
    } else {
        key = static_cast<const uint8_t *>(values)[g];
        q = key;
    }
    return true;
}

template <int VT>
__global__ __launch_bounds__(NT) void zonal_tile_kernel(
    const uint32_t *__restrict__ zones, const void *__restrict__ values, double scale, int H, int W,
    int tiles_x, uint32_t cells, uint32_t K, const u64 *__restrict__ bits,
    const uint32_t *__restrict__ before, zonal_cols cols, zonal_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[3];            // clamped, overflow, foreign
    const int tid = threadIdx.x, lane = tid & 63;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    if (tid < 3) s_cnt[tid] = 0;
#ifndef HDEM_ZONAL_PLAIN
    constexpr int VSLOTS = VT ? SLOTS : 1;
    __shared__ uint32_t s_key[SLOTS];            // 1 + row
    __shared__ uint32_t s_count[SLOTS], s_first[SLOTS];
    __shared__ u64 s_rows[SLOTS], s_cols[SLOTS];
    __shared__ uint32_t s_valid[VSLOTS];
    __shared__ u64 s_pmin[VSLOTS], s_pmax[VSLOTS], s_sum[VSLOTS];
    for (int s = tid; s < SLOTS; s += NT) {
        s_key[s] = 0u, s_count[s] = 0u, s_first[s] = NONE, s_rows[s] = 0ull, s_cols[s] = 0ull;
        if (VT) s_valid[s] = 0u, s_pmin[s] = ~0ull, s_pmax[s] = 0ull, s_sum[s] = 0ull;
    }
#endif
    __syncthreads();

    unsigned int clamped = 0, overflow = 0, foreign = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;      // lx is the lane
        if (ly >= tile.th) break;                // (whole waves: a wave is a row)
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        uint32_t z = 0;
        if (lx < tile.tw) z = zones[g];
        if (z > cells) z = 0u;                   // counted by the mark kernel; the call is refused
        zonal_add a = {1u, (uint32_t)g, 0u, 1ull << ly, 1ull << lx, ~0ull, 0ull, 0ull};
        if (VT && z) {
            uint32_t key;
            u64 q;
            if (value_of<VT>(values, g, scale, key, q, clamped)) {
                a.valid = 1u;
                a.pmin = ((u64)key << 32) | (uint32_t)g;
                a.pmax = ((u64)key << 32) | (uint32_t)~(uint32_t)g;
                a.sum = q;
            }
        }
#ifdef HDEM_ZONAL_PLAIN
        if (z) {
            uint32_t r;
            if (row_of(z, K, bits, before, r)) add_global(cols, r, y0, x0, a);
            else ++foreign;
        }
#else
        // the run of equal ids that the lane lies in: lanes first ... last
        const uint32_t left = __shfl_up(z, 1);
        const bool head = lane == 0 || z != left;
        const u64 heads = __ballot(head);
        const int first = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int last = above ? lane + __builtin_ctzll(above) : 63;
        if (VT) {
            // segmented reduction towards the first lane; stops at the longest run's length
            for (int d = 1; d < 64; d <<= 1) {
                if (!__any(z && lane + d <= last)) break;
                const uint32_t valid = __shfl_down(a.valid, d);
                const u64 pmin = __shfl_down(a.pmin, d), pmax = __shfl_down(a.pmax, d);
                const u64 sum = __shfl_down(a.sum, d);
                if (lane + d <= last) {
                    a.valid += valid;
                    a.pmin = pmin < a.pmin ? pmin : a.pmin;
                    a.pmax = pmax > a.pmax ? pmax : a.pmax;
                    a.sum += sum;
                }
            }
        }
        if (head && z) {
            a.count = (uint32_t)(last - first + 1);
            a.cols = (~0ull >> (63 - last)) & ~((1ull << first) - 1ull);
            uint32_t r;
            if (!row_of(z, K, bits, before, r)) {
                ++foreign;
            } else {
                const uint32_t key = r + 1u;
                uint32_t slot = (key * 2654435761u) >> (32 - SLOT_BITS);
                int probe = 0;
                for (; probe < PROBES; ++probe) {
                    const uint32_t seen = atomicCAS(&s_key[slot], 0u, key);
                    if (seen == 0u || seen == key) break;
                    slot = (slot + 1) & (SLOTS - 1);
                }
                if (probe < PROBES) {
                    atomicAdd(&s_count[slot], a.count);
                    atomicMin(&s_first[slot], a.first);
                    atomicOr(&s_rows[slot], a.rows);
                    atomicOr(&s_cols[slot], a.cols);
                    if (VT && a.valid) {
                        atomicAdd(&s_valid[slot], a.valid);
                        atomicMin(&s_pmin[slot], a.pmin);
                        atomicMax(&s_pmax[slot], a.pmax);
                        if (a.sum) atomicAdd(&s_sum[slot], a.sum);
                    }
                } else {                         // no slot: straight to the columns
                    overflow += a.count;
                    add_global(cols, r, y0, x0, a);
                }
            }
        }
#endif
    }
    clamped = wave_sum(clamped), overflow = wave_sum(overflow), foreign = wave_sum(foreign);
    if (lane == 0) {
        if (clamped) atomicAdd(&s_cnt[0], clamped);
        if (overflow) atomicAdd(&s_cnt[1], overflow);
        if (foreign) atomicAdd(&s_cnt[2], foreign);
    }
    __syncthreads();

#ifndef HDEM_ZONAL_PLAIN
    // one global atomic per (tile, row) and column that the tile adds to; key - 1 < K
    for (int s = tid; s < SLOTS; s += NT) {
        const uint32_t key = s_key[s];
        if (!key) continue;
        zonal_add a = {s_count[s], s_first[s], 0u, s_rows[s], s_cols[s], ~0ull, 0ull, 0ull};
        if (VT) a.valid = s_valid[s], a.pmin = s_pmin[s], a.pmax = s_pmax[s], a.sum = s_sum[s];
        add_global(cols, key - 1u, y0, x0, a);
    }
#endif
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->clamped, (u64)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->overflow, (u64)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->foreign, (u64)s_cnt[2]);
    }
}

// 3.  min, max (in the values' type) and their cells out of the packed words.  A row without a
// valid cell kept the words it was given: all ones and 0.
template <int VT>
__global__ __launch_bounds__(NT) void zonal_final_kernel(uint32_t K, const u64 *__restrict__ pmin,
                                                         const u64 *__restrict__ pmax, void *mn,
                                                         void *mx, uint32_t *__restrict__ at_min,
                                                         uint32_t *__restrict__ at_max)
{
    const uint32_t r = blockIdx.x * NT + threadIdx.x;
    if (r >= K) return;
    const u64 a = pmin[r], b = pmax[r];
    const bool none = a == ~0ull;
    const uint32_t lo = (uint32_t)(a >> 32), hi = (uint32_t)(b >> 32);
    if (VT == HDEM_ZONAL_F32) {
        const float nan = __uint_as_float(0x7FC00000u);
        if (mn) static_cast<float *>(mn)[r] = none ? nan : float_of(lo);
        if (mx) static_cast<float *>(mx)[r] = none ? nan : float_of(hi);
    } else if (VT == HDEM_ZONAL_U32) {
        if (mn) static_cast<uint32_t *>(mn)[r] = none ? 0u : lo;
        if (mx) static_cast<uint32_t *>(mx)[r] = none ? 0u : hi;
    } else {
        if (mn) static_cast<uint8_t *>(mn)[r] = none ? 0u : (uint8_t)lo;
        if (mx) static_cast<uint8_t *>(mx)[r] = none ? 0u : (uint8_t)hi;
    }
    if (at_min) at_min[r] = (uint32_t)a;
    if (at_max) at_max[r] = ~(uint32_t)b;
}

// The ids of word w have the ranks before[w], before[w] + 1, ...: one thread per word.
__global__ __launch_bounds__(NT) void zonal_id_kernel(int64_t words, uint32_t K,
                                                      const u64 *__restrict__ bits,
                                                      const uint32_t *__restrict__ before,
                                                      uint32_t *__restrict__ id)
{
    const int64_t w = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (w >= words) return;
    u64 m = bits[w];
    for (uint32_t r = before[w]; m && r < K; m &= m - 1ull, ++r)
        id[r] = (uint32_t)(w * 64 + __builtin_ctzll(m) + 1);
}

// out[c] = column[row of zones[c]], fill where there is no row.
__global__ __launch_bounds__(NT) void zonal_broadcast_kernel(
    int64_t n, const uint32_t *__restrict__ zones, uint32_t cells, uint32_t K,
    const u64 *__restrict__ bits, const uint32_t *__restrict__ before,
    const uint32_t *__restrict__ column, uint32_t fill, uint32_t *__restrict__ out)
{
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c >= n) return;
    const uint32_t z = zones[c];
    uint32_t r, v = fill;
    if (z != 0u && z <= cells && row_of(z, K, bits, before, r)) v = column[r];
    out[c] = v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct zonal_call {
    const uint32_t *zones;
    int H, W;
    const void *values;
    int value_type, frac_bits;
    int64_t K;
    uint32_t *id, *count, *first, *row_min, *row_max, *col_min, *col_max, *valid;
    void *mn, *mx;
    uint32_t *at_min, *at_max;
    void *sum;
    int flags;
    hdem_zonal_stats *stats;
};

// the arena of a call: counters | bits u64 per word | counts u32 per word | chunk sums u32 |
// packed min, packed max u64 per row (when wanted)
struct zonal_ws : hdem_rank_table {
    int64_t words;
    zonal_counters *cnt;
    u64 *pmin, *pmax;
};

int zonal_carve(hdem_ctx *ctx, int64_t cells, size_t packed_rows, zonal_ws *ws)
{
    ws->words = (cells + 63) / 64;
    const size_t table_bytes = hdem_rank_table_bytes(ws->words);
    const size_t packed_bytes = hdem_round16(packed_rows * 8);
    char *at = static_cast<char *>(hdem_arena(ctx, HEAD + table_bytes + 2 * packed_bytes));
    if (!at) return HDEM_ERR_OOM;
    ws->cnt = reinterpret_cast<zonal_counters *>(at), at += HEAD;
    hdem_rank_table_at(at, ws->words, ws), at += table_bytes;
    ws->pmin = packed_rows ? reinterpret_cast<u64 *>(at) : nullptr, at += packed_bytes;
    ws->pmax = packed_rows ? reinterpret_cast<u64 *>(at) : nullptr;
    return HDEM_OK;
}

// Step 1 on the context's stream: the bitmap, K in the counters, and the ranks when `scan`.
int zonal_ranks(hdem_ctx *ctx, const uint32_t *zones, int H, int W, const d8_grid &g,
                const zonal_ws &ws, bool scan)
{
    HDEM_HIP_CHECK(hipMemsetAsync(ws.cnt, 0, HEAD, ctx->stream));
    HDEM_HIP_CHECK(hipMemsetAsync(ws.bits, 0, (size_t)ws.words * 8, ctx->stream));
    hipLaunchKernelGGL(zonal_mark_kernel, dim3((unsigned)g.tiles), dim3(NT), 0, ctx->stream, zones,
                       H, W, g.tiles_x, (uint32_t)((int64_t)H * W), ws.bits, ws.cnt);
    hipLaunchKernelGGL(zonal_popc_kernel, dim3((unsigned)((ws.words + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, ws.words, ws.bits, ws.count, ws.cnt);
    if (scan) hdem_scan_exclusive(ctx->stream, ws.count, ws.words, ws.sums);
    HDEM_HIP_CHECK(hipGetLastError());
    return HDEM_OK;
}

int zonal_read(hdem_ctx *ctx, const zonal_ws &ws, zonal_counters *host)
{
    HDEM_HIP_CHECK(hipMemcpyAsync(host, ws.cnt, sizeof(*host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return HDEM_OK;
}

void zonal_fill_stats(hdem_zonal_stats *st, const zonal_counters &host)
{
    st->zones = (int64_t)host.zones;
    st->unzoned = (int64_t)host.unzoned;
    st->clamped = (int64_t)host.clamped;
    st->overflow = (int64_t)host.overflow;
    st->over_range = (int64_t)host.over;
    st->capped = (int64_t)host.capped;
    st->max_id = host.max_id;
}

// what the raster itself is refused for, whichever entry point read it
int zonal_report(const zonal_counters &host, int64_t cells)
{
    HDEM_REQUIRE(!host.over, HDEM_ERR_BAD_ARG,
                 "zone ids lie in 1 ... H * W = %lld: %llu cells hold a larger id, the largest is "
                 "%u (relabel first)",
                 (long long)cells, host.over, host.max_id);
    HDEM_REQUIRE(!host.capped, HDEM_ERR_NOT_CONVERGED,
                 "zonal statistics: %llu cells found no slot in their tile's id set", host.capped);
    return HDEM_OK;
}

int zonal_report_count(const zonal_counters &host, int64_t K)
{
    HDEM_REQUIRE((int64_t)host.zones == K && !host.foreign, HDEM_ERR_BAD_ARG,
                 "K = %lld is not the number of zones of this raster: it holds %llu (%llu runs of "
                 "cells found no row)",
                 (long long)K, host.zones, host.foreign);
    return HDEM_OK;
}

int check_raster(hdem_ctx *ctx, const uint32_t *zones, int H, int W, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, zones, zones, H, W)) return rc;
    return d8_grid_of("zonal statistics", H, W, g);
}

int check_args(hdem_ctx *ctx, const zonal_call &a, d8_grid *g)
{
    if (int rc = check_raster(ctx, a.zones, a.H, a.W, g)) return rc;
    HDEM_REQUIRE(!a.flags, HDEM_ERR_BAD_ARG, "unknown zonal statistics flags 0x%x", a.flags);
    HDEM_REQUIRE(a.value_type >= HDEM_ZONAL_NONE && a.value_type <= HDEM_ZONAL_U8, HDEM_ERR_BAD_ARG,
                 "unknown value type %d", a.value_type);
    HDEM_REQUIRE((a.value_type == HDEM_ZONAL_NONE) == !a.values, HDEM_ERR_BAD_ARG,
                 "values must be null with HDEM_ZONAL_NONE and only then");
    HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 30, HDEM_ERR_BAD_ARG,
                 "frac_bits is 0 ... 30, got %d", a.frac_bits);
    HDEM_REQUIRE(a.K >= 0 && a.K <= (int64_t)a.H * a.W, HDEM_ERR_BAD_ARG,
                 "K is the number of zones, 0 ... H * W: got %lld", (long long)a.K);
    HDEM_REQUIRE(a.values || !(a.valid || a.mn || a.mx || a.at_min || a.at_max || a.sum),
                 HDEM_ERR_BAD_ARG, "valid, min, max, at_min, at_max and sum need values");
    HDEM_REQUIRE(a.id || a.count || a.first || a.row_min || a.row_max || a.col_min || a.col_max ||
                     a.valid || a.mn || a.mx || a.at_min || a.at_max || a.sum,
                 HDEM_ERR_BAD_ARG, "no output wanted: give at least one column");
    return d8_check_stats(a.stats, "hdem_zonal_stats");
}

typedef hdem_event_timer<4> step_timer;   // marks around the three steps

template <int VT>
void launch_tile_and_final(hdem_ctx *ctx, const zonal_call &a, const d8_grid &g, const zonal_ws &ws,
                           const zonal_cols &cols, step_timer &steps)
{
    const uint32_t K = (uint32_t)a.K;
    hipLaunchKernelGGL(zonal_tile_kernel<VT>, dim3((unsigned)g.tiles), dim3(NT), 0, ctx->stream,
                       a.zones, a.values, (double)(1ll << a.frac_bits), a.H, a.W, g.tiles_x,
                       (uint32_t)((int64_t)a.H * a.W), K, ws.bits, ws.count, cols, ws.cnt);
    steps.mark(2);
    if constexpr (VT != HDEM_ZONAL_NONE)
        if (ws.pmin)
            hipLaunchKernelGGL(zonal_final_kernel<VT>, dim3((K + NT - 1) / NT), dim3(NT), 0,
                           ctx->stream, K, ws.pmin, ws.pmax, a.mn, a.mx, a.at_min, a.at_max);
}

int zonal_count_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W, const d8_grid &g,
                    int64_t *K, hdem_zonal_stats *stats)
{
    const int64_t cells = (int64_t)H * W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_zonal_stats st = {};
    st.tile_h = TS, st.tile_w = TS;
    zonal_ws ws;
    if (int rc = zonal_carve(ctx, cells, 0, &ws)) return rc;
    step_timer steps(ctx, stats != nullptr);
    if (int rc = steps.start()) return rc;
    steps.mark(0);
    if (int rc = zonal_ranks(ctx, zones, H, W, g, ws, false)) return rc;
    steps.mark(1);
    zonal_counters host = {};
    if (int rc = zonal_read(ctx, ws, &host)) return rc;
    zonal_fill_stats(&st, host);
    st.ms_rank = steps.ms(0, 1);
    d8_publish(stats, st);
    if (K) *K = (int64_t)host.zones;
    return zonal_report(host, cells);
}

int zonal_table_dev(hdem_ctx *ctx, const zonal_call &a, const d8_grid &g)
{
    const int64_t cells = (int64_t)a.H * a.W;
    const size_t n = (size_t)a.K;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_zonal_stats st = {};
    st.tile_h = TS, st.tile_w = TS;
    d8_publish(a.stats, st);
    const bool packed = a.mn || a.mx || a.at_min || a.at_max;
    zonal_ws ws;
    if (int rc = zonal_carve(ctx, cells, packed ? n : 0, &ws)) return rc;
    step_timer steps(ctx, a.stats != nullptr);
    if (int rc = steps.start()) return rc;

    steps.mark(0);
    if (int rc = zonal_ranks(ctx, a.zones, a.H, a.W, g, ws, n != 0)) return rc;
    steps.mark(1);
    if (n) {
        // what every column holds before the first add
        const zonal_cols cols = {a.count, a.first, a.row_min, a.row_max, a.col_min, a.col_max,
                                 a.valid, ws.pmin, ws.pmax, static_cast<u64 *>(a.sum)};
        for (uint32_t *zero : {a.count, a.row_max, a.col_max, a.valid})
            if (zero) HDEM_HIP_CHECK(hipMemsetAsync(zero, 0, n * 4, ctx->stream));
        for (uint32_t *ones : {a.first, a.row_min, a.col_min})
            if (ones) HDEM_HIP_CHECK(hipMemsetAsync(ones, 0xFF, n * 4, ctx->stream));
        if (a.sum) HDEM_HIP_CHECK(hipMemsetAsync(a.sum, 0, n * 8, ctx->stream));
        if (packed) {
            HDEM_HIP_CHECK(hipMemsetAsync(ws.pmin, 0xFF, n * 8, ctx->stream));
            HDEM_HIP_CHECK(hipMemsetAsync(ws.pmax, 0, n * 8, ctx->stream));
        }
        if (a.value_type == HDEM_ZONAL_NONE) launch_tile_and_final<HDEM_ZONAL_NONE>(ctx, a, g, ws, cols, steps);
        else if (a.value_type == HDEM_ZONAL_F32) launch_tile_and_final<HDEM_ZONAL_F32>(ctx, a, g, ws, cols, steps);
        else if (a.value_type == HDEM_ZONAL_U32) launch_tile_and_final<HDEM_ZONAL_U32>(ctx, a, g, ws, cols, steps);
        else launch_tile_and_final<HDEM_ZONAL_U8>(ctx, a, g, ws, cols, steps);
        if (a.id)
            hipLaunchKernelGGL(zonal_id_kernel, dim3((unsigned)((ws.words + NT - 1) / NT)), dim3(NT),
                               0, ctx->stream, ws.words, (uint32_t)a.K, ws.bits, ws.count, a.id);
        HDEM_HIP_CHECK(hipGetLastError());
    } else {
        steps.mark(2);
    }
    steps.mark(3);
    zonal_counters host = {};
    if (int rc = zonal_read(ctx, ws, &host)) return rc;
    zonal_fill_stats(&st, host);
    st.ms_rank = steps.ms(0, 1);
    st.ms_tile = steps.ms(1, 2);
    st.ms_final = steps.ms(2, 3);
    d8_publish(a.stats, st);
    if (int rc = zonal_report(host, cells)) return rc;
    return zonal_report_count(host, a.K);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_zonal_count_u32_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W,
                                        int64_t *K, hdem_zonal_stats *stats)
{
    d8_grid g;
    if (int rc = check_raster(ctx, zones, H, W, &g)) return rc;
    if (int rc = d8_check_stats(stats, "hdem_zonal_stats")) return rc;
    return zonal_count_dev(ctx, zones, H, W, g, K, stats);
}

extern "C" int hdem_zonal_count_u32(hdem_ctx *ctx, const uint32_t *zones, int H, int W, int64_t *K,
                                    hdem_zonal_stats *stats)
{
    d8_grid g;
    if (int rc = check_raster(ctx, zones, H, W, &g)) return rc;
    if (int rc = d8_check_stats(stats, "hdem_zonal_stats")) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dbuf dzones;
    if (int rc = dzones.upload(ctx, zones, (size_t)H * W * 4)) return rc;
    return zonal_count_dev(ctx, dzones.as<const uint32_t>(), H, W, g, K, stats);
}

extern "C" int hdem_zonal_table_u32_dev(
    hdem_ctx *ctx, const uint32_t *zones, int H, int W, const void *values, int value_type,
    int frac_bits, int64_t K, uint32_t *id, uint32_t *count, uint32_t *first, uint32_t *row_min,
    uint32_t *row_max, uint32_t *col_min, uint32_t *col_max, uint32_t *valid, void *min, void *max,
    uint32_t *at_min, uint32_t *at_max, void *sum, int flags, hdem_zonal_stats *stats)
{
    const zonal_call a = {zones, H, W, values, value_type, frac_bits, K, id, count, first, row_min,
                          row_max, col_min, col_max, valid, min, max, at_min, at_max, sum, flags,
                          stats};
    d8_grid g;
    if (int rc = check_args(ctx, a, &g)) return rc;
    return zonal_table_dev(ctx, a, g);
}

extern "C" int hdem_zonal_table_u32(
    hdem_ctx *ctx, const uint32_t *zones, int H, int W, const void *values, int value_type,
    int frac_bits, int64_t K, uint32_t *id, uint32_t *count, uint32_t *first, uint32_t *row_min,
    uint32_t *row_max, uint32_t *col_min, uint32_t *col_max, uint32_t *valid, void *min, void *max,
    uint32_t *at_min, uint32_t *at_max, void *sum, int flags, hdem_zonal_stats *stats)
{
    zonal_call a = {zones, H, W, values, value_type, frac_bits, K, id, count, first, row_min,
                    row_max, col_min, col_max, valid, min, max, at_min, at_max, sum, flags, stats};
    d8_grid g;
    if (int rc = check_args(ctx, a, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W, k = (size_t)K;
    const size_t value_bytes = value_type == HDEM_ZONAL_U8 ? 1 : 4;
    hdem_dbuf dzones, dvalues, dout[13];
    if (int rc = dzones.upload(ctx, zones, n * 4)) return rc;
    if (int rc = dvalues.upload(ctx, values, n * value_bytes)) return rc;
    // the thirteen columns in the ABI's order
    void *const host_out[13] = {id, count, first, row_min, row_max, col_min, col_max, valid, min,
                                max, at_min, at_max, sum};
    size_t out_bytes[13];
    for (int c = 0; c < 13; ++c) out_bytes[c] = k * (c == 12 ? 8 : c == 8 || c == 9 ? value_bytes : 4);
    for (int c = 0; c < 13; ++c)
        if (host_out[c] && out_bytes[c])
            if (int rc = dout[c].alloc(ctx, out_bytes[c])) return rc;
    a.zones = dzones.as<const uint32_t>();
    a.values = dvalues.p;
    if (k) {
        a.id = dout[0].as<uint32_t>(), a.count = dout[1].as<uint32_t>();
        a.first = dout[2].as<uint32_t>(), a.row_min = dout[3].as<uint32_t>();
        a.row_max = dout[4].as<uint32_t>(), a.col_min = dout[5].as<uint32_t>();
        a.col_max = dout[6].as<uint32_t>(), a.valid = dout[7].as<uint32_t>();
        a.mn = dout[8].p, a.mx = dout[9].p;
        a.at_min = dout[10].as<uint32_t>(), a.at_max = dout[11].as<uint32_t>();
        a.sum = dout[12].p;
    }
    if (int rc = zonal_table_dev(ctx, a, g)) return rc;
    for (int c = 0; c < 13; ++c)
        if (dout[c].p)
            if (int rc = dout[c].download(host_out[c], out_bytes[c])) return rc;
    return HDEM_OK;
}

extern "C" int hdem_zonal_broadcast_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W,
                                        int64_t K, const void *column, uint32_t fill, void *out)
{
    d8_grid g;
    if (int rc = check_raster(ctx, zones, H, W, &g)) return rc;
    const int64_t cells = (int64_t)H * W;
    HDEM_REQUIRE(out, HDEM_ERR_BAD_ARG, "the output raster is null");
    HDEM_REQUIRE(K >= 0 && K <= cells, HDEM_ERR_BAD_ARG,
                 "K is the number of zones, 0 ... H * W: got %lld", (long long)K);
    HDEM_REQUIRE(column || !K, HDEM_ERR_BAD_ARG, "the column is null");
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    zonal_ws ws;
    if (int rc = zonal_carve(ctx, cells, 0, &ws)) return rc;
    if (int rc = zonal_ranks(ctx, zones, H, W, g, ws, true)) return rc;
    hipLaunchKernelGGL(zonal_broadcast_kernel, dim3((unsigned)((cells + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, cells, zones, (uint32_t)cells, (uint32_t)K, ws.bits, ws.count,
                       static_cast<const uint32_t *>(column), fill, static_cast<uint32_t *>(out));
    HDEM_HIP_CHECK(hipGetLastError());
    zonal_counters host = {};
    if (int rc = zonal_read(ctx, ws, &host)) return rc;
    if (int rc = zonal_report(host, cells)) return rc;
    return zonal_report_count(host, K);
}
