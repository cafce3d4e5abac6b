// D8 watershed labelling (new operator; Watersheds).
//
// label[c] = the label of the first *stop* on c's D8 path, c included.  A stop is a terminal
// cell (code 0 or pointing outside the raster) or, in pour-point mode, a seeded cell.
//   outlet mode      label of a terminal cell = 1 + its flat index
//   pour-point mode  label of a seeded cell = its seed, of an unseeded terminal cell = 0
//   compact mode     outlet mode renumbered 1 ... K (K terminal cells), outlets[k-1] = index
// Codes are those of hdem_flowacc.hip, and so is the structure: 64 x 64 tiles, 252 perimeter
// slots per tile, a forest over the slots.  A label travels down -> up by pointer jumping:
// plain loads and stores, no arrival counting.
//   A  (watershed_tile_kernel)   per tile: every cell's in-tile receiver, then 16-bit pointer
//      doubling in LDS (<= 12 rounds, leaves when a round changes nothing) until every cell
//      points at a stop or at an *exit* (an unseeded cell whose receiver lies in a
//      neighbouring tile).  Writes 2 B per cell (which stop / which exit) and one forest
//      word per perimeter slot: "resolved, label L" when the frame cell's in-tile path ends
//      in a stop, else "next = the slot of the cell that its exit drains into".  A seeded
//      frame cell is a stop like any other, so the word of a seeded cell that an exit of the
//      neighbouring tile drains into is resolved by the tile that owns it: no tile looks at
//      the seeds of its halo.
//   S  (watershed_scan_kernel)   compact mode only: exclusive scan of the tiles' terminal
//      counts; a terminal's label is 1 + offset of its tile + its rank inside the tile.
//   B  (watershed_forest_kernel) in-place pointer jumping over the slot words, up to 4 jumps
//      per node and launch.  A word is (resolved << 32 | label or next slot), read and written
//      whole, and a node only ever replaces its pointer by its pointer's pointer, so whatever
//      a racing reader sees is an ancestor and a round at least halves every chain.  The host
//      enqueues ceil(log2 slots) + 1 launches; a launch whose predecessor left nothing
//      unresolved returns at once (the count stays on the device), so a cycle costs the full
//      schedule and nothing more.
//   C  (watershed_final_kernel)  per tile, streaming: the tile's 252 resolved words in LDS,
//      2 B per cell in, 4 B per cell out.  Counts what never resolved (a cycle).
#include "hdem_internal.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int NT = 256;               // threads per forest / final workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each; A takes
                                      // 1.35x as long with 256 and 1.43x with 1024)
constexpr int TS = 64;                // tile edge
constexpr int TC = TS * TS;           // cells per tile (12-bit local index)
constexpr int PER = 4 * TS - 4;       // perimeter slots per tile
constexpr int DOUBLINGS = 12;         // 2^12 >= the longest path inside a tile (4095 steps)
constexpr int JUMPS = 4;              // forest jumps per node and launch (B at 16384^2:
                                      // 0.47 ms with 1, 0.39 with 4, 0.49 with 16)
constexpr int MAX_ROUNDS = 32;        // forest launches: slots < 2^31
constexpr int SCAN_NT = 1024;
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile, cell not seeded
constexpr uint16_t STOP = 0xFFFF;     // rl[]: terminal, seeded, or outside the raster
constexpr uint16_t T_EXIT = 0x8000;   // per-cell target: perimeter slot of the exit reached
constexpr uint16_t T_RANK = 0x4000;   // per-cell target, compact mode: a terminal's own rank
constexpr uint64_t RESOLVED = 1ull << 32;

struct watershed_counters {
    unsigned long long terminals;     // terminal cells
    unsigned long long exits;         // exit cells (forest pointers of their own)
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells that never reached a stop
    unsigned long long stuck_slots;   // forest words that never resolved
    unsigned long long unresolved[MAX_ROUNDS];   // forest words left after each round
};

// bit b of a code -> (dy, dx), packed (d + 1) in 4 bits per entry
__device__ __forceinline__ int code_dy(int b) { return ((0x00012221u >> (4 * b)) & 3) - 1; }
__device__ __forceinline__ int code_dx(int b) { return ((0x21000122u >> (4 * b)) & 3) - 1; }

// perimeter slot of a frame cell: top row, bottom row, left column, right column
__device__ __forceinline__ int perim_pos(int ly, int lx)
{
    return ly == 0 ? lx : ly == TS - 1 ? TS + lx : lx == 0 ? 2 * TS + ly - 1 : 3 * TS - 2 + ly - 1;
}
__device__ __forceinline__ void perim_cell(int p, int &ly, int &lx)
{
    if (p < TS) { ly = 0; lx = p; }
    else if (p < 2 * TS) { ly = TS - 1; lx = p - TS; }
    else if (p < 3 * TS - 2) { ly = p - 2 * TS + 1; lx = 0; }
    else { ly = p - (3 * TS - 2) + 1; lx = TS - 1; }
}

// Slot of local frame position (ny, nx) that lies one cell outside tile (ty, tx): the
// perimeter slot of that cell in the tile that holds it.
__device__ __forceinline__ int64_t slot_of(int ty, int tx, int tiles_x, int ny, int nx)
{
    const int sy = ny < 0 ? -1 : ny >= TS ? 1 : 0;
    const int sx = nx < 0 ? -1 : nx >= TS ? 1 : 0;
    const int64_t tile = (int64_t)(ty + sy) * tiles_x + (tx + sx);
    return tile * PER + perim_pos(ny - sy * TS, nx - sx * TS);
}

__device__ __forceinline__ uint64_t word_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void word_store(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A.  COMPACT: also rank the tile's terminal cells (order: pass, wave, lane).
template <bool COMPACT>
__global__ __launch_bounds__(TNT) void watershed_tile_kernel(
    const uint8_t *__restrict__ d8, const uint32_t *__restrict__ seeds, int H, int W, int tiles_x,
    uint16_t *__restrict__ target, uint64_t *__restrict__ word, uint32_t *__restrict__ tile_count,
    watershed_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[TC];
    __shared__ uint16_t rl[TC];
    __shared__ uint16_t jump[2][TC];
    __shared__ uint32_t wave_terms[TC / 64];     // COMPACT: terminals per (pass, wave)
    __shared__ unsigned int s_cnt[4];            // invalid codes, terminals, exits, stuck cells

    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    const int64_t base = (int64_t)blockIdx.x * PER;

    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    // receivers; a stop or an exit points at itself
    unsigned int bad = 0, terms = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        uint16_t r = STOP;
        int c = 0;
        bool terminal = false;
        if (ly < th && lx < tw) {
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            c = d8[g];
            terminal = true;
            if (c & (c - 1)) {
                ++bad;
            } else if (c) {
                const int b = __builtin_ctz(c);
                const int ny = ly + code_dy(b), nx = lx + code_dx(b);
                const int gy = y0 + ny, gx = x0 + nx;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    terminal = false;
                    if (!seeds || seeds[g] == 0)
                        r = (ny >= 0 && ny < TS && nx >= 0 && nx < TS) ? (uint16_t)(ny * TS + nx)
                                                                        : EXIT;
                }
            }
        }
        code[i] = (uint8_t)c;
        rl[i] = r;
        jump[0][i] = r >= EXIT ? (uint16_t)i : r;
        terms += terminal;
        if (COMPACT) {
            const unsigned long long m = __ballot(terminal);
            if ((tid & 63) == 0) wave_terms[i / 64] = (uint32_t)__popcll(m);
            // the rank inside the wave, kept in jump[1] until the doubling needs it
            jump[1][i] = terminal ? (uint16_t)__popcll(m & ((1ull << (tid & 63)) - 1)) : 0;
        }
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (terms) atomicAdd(&s_cnt[1], terms);
    __syncthreads();

    if (COMPACT) {
        // a terminal's own target word carries its rank in the tile
        for (int i = tid; i < TC; i += TNT) {
            const int ly = i / TS, lx = i % TS;
            if (ly >= th || lx >= tw || rl[i] != STOP) continue;
            uint32_t before = 0;
            for (int k = 0; k < i / 64; ++k) before += wave_terms[k];
            target[(size_t)blockIdx.x * TC + i] = T_RANK | (uint16_t)(before + jump[1][i]);
        }
        __syncthreads();
    }

    // pointer doubling: after round k a cell points 2^k steps down its in-tile path, or at
    // the stop / exit that ends it
    int cur = 0;
    for (int round = 0; round < DOUBLINGS; ++round) {
        int changed = 0;
        for (int i = tid; i < TC; i += TNT) {
            const uint16_t a = jump[cur][i];
            const uint16_t b = jump[cur][a];
            jump[cur ^ 1][i] = b;
            changed |= a != b;
        }
        cur ^= 1;
        if (!__syncthreads_or(changed)) break;
    }
    const uint16_t *jmp = jump[cur];

    // 2 B per cell for C: the stop (local index) or the exit (perimeter slot) it reaches
    unsigned int stuck = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= th || lx >= tw) continue;
        const uint16_t t = jmp[i];
        const uint16_t k = rl[t];
        if (k < EXIT) ++stuck;                       // still travelling: a cycle inside the tile
        if (COMPACT && t == i && k == STOP) continue;    // its rank is already there
        target[(size_t)blockIdx.x * TC + i] =
            k == EXIT ? (uint16_t)(T_EXIT | perim_pos(t / TS, t % TS)) : t;
    }
    if (stuck) atomicAdd(&s_cnt[3], stuck);

    // the perimeter slots
    if (tid < PER) {
        int ly, lx;
        perim_cell(tid, ly, lx);
        uint64_t w = RESOLVED;                       // outside the raster: never read
        if (ly < th && lx < tw) {
            const int i = ly * TS + lx;
            const int t = jmp[i];
            const uint16_t k = rl[t];
            const int t_ly = t / TS, t_lx = t % TS;
            if (k == STOP) {
                const size_t g = (size_t)(y0 + t_ly) * W + x0 + t_lx;
                w = RESOLVED | (seeds ? seeds[g] : (uint32_t)g + 1u);
            } else if (k == EXIT) {
                const int b = __builtin_ctz(code[t]);
                w = (uint64_t)slot_of(ty, tx, tiles_x, t_ly + code_dy(b), t_lx + code_dx(b));
            } else {
                w = (uint64_t)(base + tid);          // a cycle: points at itself, never resolves
            }
            if (rl[i] == EXIT) atomicAdd(&s_cnt[2], 1u);
        }
        word[base + tid] = w;
    }
    __syncthreads();
    if (tid == 0) {
        if (COMPACT) tile_count[blockIdx.x] = s_cnt[1];
        if (s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->terminals, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->exits, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[3]);
    }
}

// S: exclusive scan of the tiles' terminal counts, in place; one workgroup.
__global__ __launch_bounds__(SCAN_NT) void watershed_scan_kernel(uint32_t *__restrict__ count,
                                                                 int64_t tiles)
{
    __shared__ uint32_t part[SCAN_NT];
    const int tid = threadIdx.x;
    const int64_t chunk = (tiles + SCAN_NT - 1) / SCAN_NT;
    const int64_t lo = tid * chunk < tiles ? tid * chunk : tiles;
    const int64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
    uint32_t sum = 0;
    for (int64_t t = lo; t < hi; ++t) sum += count[t];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_NT; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (int64_t t = lo; t < hi; ++t) {
        const uint32_t n = count[t];
        count[t] = run;
        run += n;
    }
}

// B: one round of pointer jumping over the slot words.  Grid-stride.
__global__ __launch_bounds__(NT) void watershed_forest_kernel(int64_t nslots, int round,
                                                              uint64_t *__restrict__ word,
                                                              watershed_counters *__restrict__ cnt)
{
    if (round > 0 && __hip_atomic_load(&cnt->unresolved[round - 1], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT) == 0)
        return;
    __shared__ unsigned int s_left;
    if (threadIdx.x == 0) s_left = 0;
    __syncthreads();
    unsigned int left = 0;
    for (int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x; s < nslots;
         s += (int64_t)gridDim.x * NT) {
        uint64_t w = word_load(&word[s]);
        for (int j = 0; j < JUMPS && !(w & RESOLVED); ++j) {
            w = word_load(&word[(uint32_t)w]);       // my pointer's word: a label or an ancestor
            word_store(&word[s], w);
        }
        left += !(w & RESOLVED);
    }
    for (int m = 32; m >= 1; m >>= 1) left += __shfl_xor(left, m);
    if ((threadIdx.x & 63) == 0 && left) atomicAdd(&s_left, left);
    __syncthreads();
    if (threadIdx.x == 0 && s_left) atomicAdd(&cnt->unresolved[round], (unsigned long long)s_left);
}

// C.  MODE 0: outlet, 1: pour points, 2: compact.
template <int MODE>
__global__ __launch_bounds__(NT) void watershed_final_kernel(
    const uint32_t *__restrict__ seeds, int H, int W, int tiles_x,
    const uint16_t *__restrict__ target, const uint64_t *__restrict__ word,
    const uint32_t *__restrict__ tile_offset, uint32_t *__restrict__ out,
    uint32_t *__restrict__ outlets, watershed_counters *__restrict__ cnt)
{
    __shared__ uint32_t label[PER];
    __shared__ uint8_t known[PER];
    __shared__ unsigned int s_cnt[2];            // stuck cells, stuck slots

    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    const uint16_t *tg = target + (size_t)blockIdx.x * TC;

    if (tid < 2) s_cnt[tid] = 0;
    if (tid < PER) {
        const uint64_t w = word[(int64_t)blockIdx.x * PER + tid];
        uint32_t l = (uint32_t)w;
        const bool ok = (w & RESOLVED) != 0;
        if (MODE == 2 && ok) {
            // the outlet's flat index -> its tile and its rank there
            int ly, lx;
            perim_cell(tid, ly, lx);
            if (ly < th && lx < tw) {
                const uint32_t g = l - 1u;
                const int gy = (int)(g / (uint32_t)W), gx = (int)(g % (uint32_t)W);
                const size_t t = (size_t)(gy / TS) * tiles_x + gx / TS;
                l = tile_offset[t] + (target[t * TC + (gy % TS) * TS + gx % TS] & 0xFFF) + 1u;
            }
        }
        label[tid] = l;
        known[tid] = ok;
    }
    __syncthreads();
    if (tid < PER && !known[tid]) atomicAdd(&s_cnt[1], 1u);

    unsigned int stuck = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= th || lx >= tw) continue;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        uint16_t v = tg[i];
        uint32_t l;
        if (v & T_EXIT) {
            l = label[v & 0xFF];
            stuck += !known[v & 0xFF];
        } else if (MODE == 2) {
            const bool self = (v & T_RANK) != 0;
            if (!self) v = tg[v];                    // the terminal's own word: its rank
            const uint32_t k = tile_offset[blockIdx.x] + (v & 0xFFF);
            if (self) outlets[k] = (uint32_t)g;
            l = k + 1u;
        } else {
            const size_t s = (size_t)(y0 + v / TS) * W + x0 + v % TS;
            l = MODE == 1 ? seeds[s] : (uint32_t)s + 1u;
        }
        out[g] = l;
    }
    if (stuck) atomicAdd(&s_cnt[0], stuck);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->stuck_slots, (unsigned long long)s_cnt[1]);
    }
}

int check_args(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const uint32_t *seeds, int flags,
               uint32_t *out, uint32_t *outlets, hdem_watershed_stats *stats)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    if (int rc = hdem_check_raster(d8, out, H, W)) return rc;
    const int64_t cells = (int64_t)H * W;
    HDEM_REQUIRE(cells <= (int64_t)UINT32_MAX, HDEM_ERR_BAD_ARG,
                 "watershed labels are uint32: %d x %d = %lld cells is more than 2^32 - 1", H, W,
                 (long long)cells);
    HDEM_REQUIRE(!(flags & ~HDEM_WS_COMPACT), HDEM_ERR_BAD_ARG, "unknown watershed flags 0x%x",
                 flags);
    const bool compact = (flags & HDEM_WS_COMPACT) != 0;
    HDEM_REQUIRE(!(compact && seeds), HDEM_ERR_BAD_ARG,
                 "compact labels number the outlets: they cannot be combined with pour points");
    HDEM_REQUIRE(compact == (outlets != nullptr), HDEM_ERR_BAD_ARG,
                 "outlets must be given with HDEM_WS_COMPACT and only then");
    HDEM_REQUIRE(!stats || stats->struct_size >= sizeof(uint32_t), HDEM_ERR_BAD_ARG,
                 "hdem_watershed_stats.struct_size is %u: set it to sizeof(hdem_watershed_stats)",
                 stats ? stats->struct_size : 0u);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_watershed_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                     const uint32_t *seeds, int flags, uint32_t *out,
                                     uint32_t *outlets, hdem_watershed_stats *stats)
{
    if (int rc = check_args(ctx, d8, H, W, seeds, flags, out, outlets, stats)) return rc;
    const bool compact = (flags & HDEM_WS_COMPACT) != 0;
    const int tiles_y = (H + TS - 1) / TS, tiles_x = (W + TS - 1) / TS;
    const int64_t tiles = (int64_t)tiles_y * tiles_x;
    const int64_t nslots = tiles * PER;
    // (slots are 31-bit; only rasters a few cells wide and ~10^9 long get here)
    HDEM_REQUIRE(nslots <= INT32_MAX, HDEM_ERR_BAD_ARG,
                 "watersheds: %d x %d has %lld tiles of %d x %d, more than %d", H, W,
                 (long long)tiles, TS, TS, INT32_MAX / PER);
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));

    // what the caller's struct has room for is filled, and nothing beyond it
    hdem_watershed_stats st = {};
    const uint32_t st_size = stats ? std::min<uint32_t>(stats->struct_size, sizeof(st)) : 0;
    st.struct_size = st_size;
    auto publish = [&]() { if (stats) memcpy(stats, &st, st_size); };
    publish();

    // arena: counters | word u64 per slot | tile offsets u32 per tile | target u16 per cell
    const size_t head = 512;
    static_assert(sizeof(watershed_counters) <= head, "counters outgrew their block");
    const size_t bytes = head + (size_t)nslots * 8 + (size_t)tiles * 4 + (size_t)tiles * TC * 2;
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    watershed_counters *cnt = reinterpret_cast<watershed_counters *>(ws);
    uint64_t *word = reinterpret_cast<uint64_t *>(ws + head);
    uint32_t *tile_offset = reinterpret_cast<uint32_t *>(word + nslots);
    uint16_t *target = reinterpret_cast<uint16_t *>(tile_offset + tiles);

    hipEvent_t ev[4] = {};
    const bool phases = ctx->profiling && stats;
    for (int k = 0; phases && k < 4; ++k) HDEM_HIP_CHECK(hipEventCreate(&ev[k]));
    auto mark = [&](int k) { if (phases) (void)hipEventRecord(ev[k], ctx->stream); };

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(watershed_counters), ctx->stream));
    int rounds = 1;                               // ceil(log2 nslots) + 1
    while ((1ll << (rounds - 1)) < nslots) ++rounds;
    const int64_t forest_blocks = (nslots + NT - 1) / NT;
    const int forest_grid = (int)std::min<int64_t>(forest_blocks, (int64_t)ctx->num_cus * 8);
    const dim3 grid((unsigned)tiles);

    mark(0);
    if (compact) {
        hipLaunchKernelGGL(watershed_tile_kernel<true>, grid, dim3(TNT), 0, ctx->stream, d8, seeds,
                           H, W, tiles_x, target, word, tile_offset, cnt);
        hipLaunchKernelGGL(watershed_scan_kernel, dim3(1), dim3(SCAN_NT), 0, ctx->stream,
                           tile_offset, tiles);
    } else {
        hipLaunchKernelGGL(watershed_tile_kernel<false>, grid, dim3(TNT), 0, ctx->stream, d8,
                           seeds, H, W, tiles_x, target, word, tile_offset, cnt);
    }
    mark(1);
    for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(watershed_forest_kernel, dim3(forest_grid), dim3(NT), 0, ctx->stream,
                           nslots, r, word, cnt);
    mark(2);
    if (compact)
        hipLaunchKernelGGL(watershed_final_kernel<2>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    else if (seeds)
        hipLaunchKernelGGL(watershed_final_kernel<1>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    else
        hipLaunchKernelGGL(watershed_final_kernel<0>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    watershed_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.basins = (int64_t)host.terminals;
    st.exits = (int64_t)host.exits;
    st.forest_rounds = 1;
    while (st.forest_rounds < rounds && host.unresolved[st.forest_rounds - 1]) ++st.forest_rounds;
    st.tile_h = TS;
    st.tile_w = TS;
    if (phases) {
        (void)hipEventElapsedTime(&st.ms_tile, ev[0], ev[1]);
        (void)hipEventElapsedTime(&st.ms_forest, ev[1], ev[2]);
        (void)hipEventElapsedTime(&st.ms_final, ev[2], ev[3]);
    }
    publish();
    for (int k = 0; phases && k < 4; ++k) (void)hipEventDestroy(ev[k]);
    HDEM_REQUIRE(!host.bad, HDEM_ERR_BAD_ARG,
                 "invalid D8 code in %llu cells: a code is 0 or one of 1, 2, 4, ..., 128",
                 host.bad);
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_slots, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never resolve (and %llu tile "
                 "perimeter slots)",
                 host.stuck_cells, host.stuck_slots);
    return HDEM_OK;
}

extern "C" int hdem_watershed_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                 const uint32_t *seeds, int flags, uint32_t *out,
                                 uint32_t *outlets, hdem_watershed_stats *stats)
{
    if (int rc = check_args(ctx, d8, H, W, seeds, flags, out, outlets, stats)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dseeds, dout, doutlets;
    if (int rc = dd8.alloc(ctx, n)) return rc;
    if (int rc = dout.alloc(ctx, n * sizeof(uint32_t))) return rc;
    if (int rc = hdem_memcpy_h2d(ctx, dd8.p, d8, n)) return rc;
    if (seeds) {
        if (int rc = dseeds.alloc(ctx, n * sizeof(uint32_t))) return rc;
        if (int rc = hdem_memcpy_h2d(ctx, dseeds.p, seeds, n * sizeof(uint32_t))) return rc;
    }
    if (outlets)
        if (int rc = doutlets.alloc(ctx, n * sizeof(uint32_t))) return rc;
    // the basin count is needed here whether the caller asked for stats or not
    hdem_watershed_stats st = {};
    st.struct_size = sizeof(st);
    const int rc = hdem_watershed_u8_dev(ctx, (const uint8_t *)dd8.p, H, W,
                                         (const uint32_t *)dseeds.p, flags, (uint32_t *)dout.p,
                                         (uint32_t *)doutlets.p, &st);
    if (stats) {
        st.struct_size = std::min<uint32_t>(stats->struct_size, sizeof(st));
        memcpy(stats, &st, st.struct_size);
    }
    if (rc) return rc;
    if (outlets)
        if (int rc2 = hdem_memcpy_d2h(ctx, outlets, doutlets.p, (size_t)st.basins * sizeof(uint32_t)))
            return rc2;
    return hdem_memcpy_d2h(ctx, out, dout.p, n * sizeof(uint32_t));
}
