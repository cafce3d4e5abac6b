// D8 watershed labelling (new operator; Watersheds).
//
// label[c] = the label of the first *stop* on c's D8 path, c included.  A stop is a terminal
// cell (code 0 or pointing outside the raster) or, in pour-point mode, a seeded cell.
//   outlet mode      label of a terminal cell = 1 + its flat index
//   pour-point mode  label of a seeded cell = its seed, of an unseeded terminal cell = 0
//   compact mode     outlet mode renumbered 1 ... K (K terminal cells), outlets[k-1] = index
// The codes, what makes a cell terminal and the structure are those of hdem_d8tile.h: 64 x 64
// tiles, 252 perimeter slots per tile, a forest over the slots.  A label travels down -> up by
// pointer jumping: plain loads and stores, no arrival counting.
//   A  (watershed_tile_kernel)   per tile: every cell's in-tile receiver, then 16-bit pointer
//      doubling in LDS (<= 12 rounds, leaves when a round changes nothing) until every cell
//      points at a stop or at an *exit* (an unseeded cell whose receiver lies in a
//      neighbouring tile).  Writes 2 B per cell (which stop / which exit) and one forest
//      word per perimeter slot: "resolved, label L" when the frame cell's in-tile path ends
//      in a stop, else "next = the slot of the cell that its exit drains into".  A seeded
//      frame cell is a stop like any other, so the word of a seeded cell that an exit of the
//      neighbouring tile drains into is resolved by the tile that owns it: no tile looks at
//      the seeds of its halo.
//   S  (hdem_scan.h, its one workgroup)  compact mode only: exclusive scan of the tiles'
//      terminal counts; a terminal's label is 1 + offset of its tile + its rank inside the tile.
//   B  (watershed_forest_kernel) in-place pointer jumping over the slot words, up to 4 jumps
//      per node and launch.  A word is (resolved << 32 | label or next slot), read and written
//      whole, and a node only ever replaces its pointer by its pointer's pointer, so whatever
//      a racing reader sees is an ancestor and a round at least halves every chain.  The host
//      enqueues ceil(log2 slots) + 1 launches; a launch whose predecessor left nothing
//      unresolved returns at once (the count stays on the device), so a cycle costs the full
//      schedule and nothing more.
//   C  (watershed_final_kernel)  per tile, streaming: the tile's 252 resolved words in LDS,
//      2 B per cell in, 4 B per cell out.  Counts what never resolved (a cycle).
#include "hdem_d8tile.h"
#include "hdem_scan.h"

namespace {

constexpr int NT = 256;               // threads per forest / final workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each; A takes
                                      // 1.35x as long with 256 and 1.43x with 1024)
constexpr int JUMPS = 4;              // forest jumps per node and launch (B at 16384^2:
                                      // 0.47 ms with 1, 0.39 with 4, 0.49 with 16)
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile, cell not seeded
constexpr uint16_t STOP = 0xFFFF;     // rl[]: terminal, seeded, or outside the raster
constexpr uint16_t T_RANK = 0x4000;   // per-cell target, compact mode: a terminal's own rank
constexpr uint64_t RESOLVED = 1ull << 32;

struct watershed_counters : d8_forest_counters {
    unsigned long long terminals;     // terminal cells
};

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
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;

    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    // receivers; a stop or an exit points at itself
    unsigned int bad = 0, terms = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        uint16_t r = STOP;
        int c = 0;
        bool terminal = false;
        if (tile.inside(ly, lx)) {
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            c = d8[g];
            const d8_step s = d8_decode(c, ly, lx, tile, H, W);
            if (s.invalid) ++bad;
            terminal = s.terminal;
            if (!terminal && (!seeds || seeds[g] == 0))
                r = s.in_tile() ? (uint16_t)(s.ny * TS + s.nx) : EXIT;
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
            if (!tile.inside(ly, lx) || rl[i] != STOP) continue;
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
        if (!tile.inside(ly, lx)) continue;
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
        if (tile.inside(ly, lx)) {
            const int i = ly * TS + lx;
            const int t = jmp[i];
            const uint16_t k = rl[t];
            const int t_ly = t / TS, t_lx = t % TS;
            if (k == STOP) {
                const size_t g = (size_t)(y0 + t_ly) * W + x0 + t_lx;
                w = RESOLVED | (seeds ? seeds[g] : (uint32_t)g + 1u);
            } else if (k == EXIT) {
                const int b = __builtin_ctz(code[t]);
                w = (uint64_t)slot_of(tile, tiles_x, t_ly + code_dy(b), t_lx + code_dx(b));
            } else {
                w = (uint64_t)(tile.base + tid);     // a cycle: points at itself, never resolves
            }
            if (rl[i] == EXIT) atomicAdd(&s_cnt[2], 1u);
        }
        word[tile.base + tid] = w;
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

// B: one round of pointer jumping over the slot words.  Grid-stride.
__global__ __launch_bounds__(NT) void watershed_forest_kernel(int64_t nslots, int round,
                                                              uint64_t *__restrict__ word,
                                                              watershed_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_left;
    if (!d8_forest_begin(cnt, round, &s_left)) return;
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
    d8_forest_end(cnt, round, left, &s_left);
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
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const uint16_t *tg = target + (size_t)blockIdx.x * TC;

    if (tid < 2) s_cnt[tid] = 0;
    if (tid < PER) {
        const uint64_t w = word[tile.base + tid];
        uint32_t l = (uint32_t)w;
        const bool ok = (w & RESOLVED) != 0;
        if (MODE == 2 && ok) {
            // the outlet's flat index -> its tile and its rank there
            int ly, lx;
            perim_cell(tid, ly, lx);
            if (tile.inside(ly, lx)) {
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
        if (!tile.inside(ly, lx)) continue;
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

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const uint32_t *seeds, int flags,
               uint32_t *out, uint32_t *outlets, hdem_watershed_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, d8, out, H, W)) return rc;
    if (int rc = d8_grid_of("watersheds", H, W, g)) return rc;
    HDEM_REQUIRE(!(flags & ~HDEM_WS_COMPACT), HDEM_ERR_BAD_ARG, "unknown watershed flags 0x%x",
                 flags);
    const bool compact = (flags & HDEM_WS_COMPACT) != 0;
    HDEM_REQUIRE(!(compact && seeds), HDEM_ERR_BAD_ARG,
                 "compact labels number the outlets: they cannot be combined with pour points");
    HDEM_REQUIRE(compact == (outlets != nullptr), HDEM_ERR_BAD_ARG,
                 "outlets must be given with HDEM_WS_COMPACT and only then");
    return d8_check_stats(stats, "hdem_watershed_stats");
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_watershed_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                     const uint32_t *seeds, int flags, uint32_t *out,
                                     uint32_t *outlets, hdem_watershed_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, seeds, flags, out, outlets, stats, &g)) return rc;
    const bool compact = (flags & HDEM_WS_COMPACT) != 0;
    const int tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, nslots = g.nslots;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_watershed_stats st = {};
    d8_publish(stats, st);

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

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(watershed_counters), ctx->stream));
    const d8_forest_plan forest = d8_forest_plan_of(ctx, nslots, NT);
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    if (compact) {
        hipLaunchKernelGGL(watershed_tile_kernel<true>, grid, dim3(TNT), 0, ctx->stream, d8, seeds,
                           H, W, tiles_x, target, word, tile_offset, cnt);
        hdem_scan_exclusive_small(ctx->stream, tile_offset, tiles);
    } else {
        hipLaunchKernelGGL(watershed_tile_kernel<false>, grid, dim3(TNT), 0, ctx->stream, d8,
                           seeds, H, W, tiles_x, target, word, tile_offset, cnt);
    }
    phases.mark(1);
    for (int r = 0; r < forest.rounds; ++r)
        hipLaunchKernelGGL(watershed_forest_kernel, dim3(forest.grid), dim3(NT), 0, ctx->stream,
                           nslots, r, word, cnt);
    phases.mark(2);
    if (compact)
        hipLaunchKernelGGL(watershed_final_kernel<2>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    else if (seeds)
        hipLaunchKernelGGL(watershed_final_kernel<1>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    else
        hipLaunchKernelGGL(watershed_final_kernel<0>, grid, dim3(NT), 0, ctx->stream, seeds, H, W,
                           tiles_x, target, word, tile_offset, out, outlets, cnt);
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    watershed_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.basins = (int64_t)host.terminals;
    st.exits = (int64_t)host.exits;
    st.forest_rounds = d8_forest_rounds(forest, host);
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_tile, &st.ms_forest, &st.ms_final);
    d8_publish(stats, st);
    return d8_report_forest(host);
}

extern "C" int hdem_watershed_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                 const uint32_t *seeds, int flags, uint32_t *out,
                                 uint32_t *outlets, hdem_watershed_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, seeds, flags, out, outlets, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W, bytes = n * sizeof(uint32_t);
    hdem_dbuf dd8, dseeds, dout, doutlets;
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dseeds.upload(ctx, seeds, bytes)) return rc;
    if (int rc = dout.alloc(ctx, bytes)) return rc;
    if (outlets)
        if (int rc = doutlets.alloc(ctx, bytes)) return rc;
    // the basin count is needed here whether the caller asked for stats or not
    hdem_watershed_stats st = {};
    st.struct_size = sizeof(st);
    const int rc = hdem_watershed_u8_dev(ctx, dd8.as<const uint8_t>(), H, W,
                                         dseeds.as<const uint32_t>(), flags, dout.as<uint32_t>(),
                                         doutlets.as<uint32_t>(), &st);
    d8_publish(stats, st);
    if (rc) return rc;
    if (outlets)
        if (int rc2 = doutlets.download(outlets, (size_t)st.basins * sizeof(uint32_t))) return rc2;
    return dout.download(out, bytes);
}
