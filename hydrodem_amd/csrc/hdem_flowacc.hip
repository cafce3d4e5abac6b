// D8 flow accumulation (new operator; FlowAccumulation).
//
// acc[c] = number of cells whose D8 path passes through c, c itself included: the unique
// solution of acc[c] = 1 + sum acc[d] over the neighbours d whose code points at c.  The
// codes, what makes a cell terminal, the tiles and their perimeter slots are those of
// hdem_d8tile.h.  Integers: bit-exact whatever order the adds land in.
//
// A GPU form of Barnes' tiled accumulation (2017).  Four launches whatever the length of the
// longest path, and no workgroup ever waits on another:
//   A  (flowacc_tile_kernel<false>)  per 64 x 64 tile: in-tile accumulation by "last donor
//      continues" walks over one 64-bit LDS word per cell (arrivals << 32 | value), then the
//      tile's 252 perimeter slots: the local value of each exit cell (a cell whose receiver
//      lies in a neighbouring tile), the slot of the cell it drains into, and for every
//      perimeter cell the exit its in-tile path reaches (pointer jumping, 12 rounds).
//   B1 (flowacc_forest_degree_kernel) the exit forest: node = exit cell, next(e) = the exit
//      that the cell e drains into reaches in its own tile; in-degrees by global atomics.
//   B2 (flowacc_forest_walk_kernel)  the same last-donor walk over the forest, one returned
//      device-scope 64-bit atomic per hop (value and arrival in one word: no fences).
//   C  (flowacc_tile_kernel<true>)   A's walk again with seeds 1 + inflow, the inflow of a
//      perimeter cell being the final forest values of the halo exits that drain into it;
//      writes acc.  Also counts what never completed (a cycle).
// Every walk step completes one arrival on one node, so every loop is bounded by the
// nodes it completes (and, explicitly, by the node count).
#include "hdem_d8tile.h"

namespace {

constexpr int NT = 256;               // threads per forest workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each; 256: 1.6x
                                      // slower, the walks of a thread run one after another)
constexpr int HS = TS + 2;            // staged tile with its one-cell halo
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile
constexpr uint16_t TERM = 0xFFFF;     // rl[]: terminal (code 0, leaves the raster, invalid, outside)
constexpr uint8_t OUTSIDE = 0xFF;     // indeg[]: cell of a partial tile beyond the raster
constexpr uint64_t ARRIVAL = 1ull << 32;

struct flowacc_counters {
    unsigned long long exits;         // exit-forest nodes
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells whose in-tile donors never all arrived
    unsigned long long stuck_exits;   // forest nodes whose donors never all arrived
    int max_hops;                     // longest B2 walk
};

template <bool FINAL>
__global__ __launch_bounds__(TNT) void flowacc_tile_kernel(
    const uint8_t *__restrict__ d8, int H, int W, int tiles_x, uint32_t *__restrict__ out,
    uint64_t *__restrict__ word, uint32_t *__restrict__ indeg_b, int32_t *__restrict__ link,
    int32_t *__restrict__ tgt, flowacc_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[HS * HS];
    __shared__ uint16_t rl[TC];
    __shared__ uint8_t indeg[TC];
    __shared__ uint64_t acc[TC];            // A: reused by the pointer jumping afterwards
    __shared__ unsigned int s_cnt[3];       // invalid codes, stuck cells, stuck exits

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const int64_t base = tile.base;

    if (tid < 3) s_cnt[tid] = 0;
    for (int i = tid; i < HS * HS; i += TNT) {
        const int gy = y0 + i / HS - 1, gx = x0 + i % HS - 1;
        code[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? d8[(size_t)gy * W + gx] : 0;
    }
    __syncthreads();

    // receivers, in-tile in-degrees (gathered: the neighbours whose code points here) and
    // seeds: 1, plus in C the final forest values of the halo exits that drain here
    unsigned int bad = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) {
            rl[i] = TERM;
            indeg[i] = OUTSIDE;
            continue;
        }
        const d8_step s = d8_decode(code[(ly + 1) * HS + lx + 1], ly, lx, tile, H, W);
        if (s.invalid) ++bad;
        rl[i] = s.terminal ? TERM : s.in_tile() ? (uint16_t)(s.ny * TS + s.nx) : EXIT;
        int deg = 0;
        uint32_t seed = 1;
        for (int b = 0; b < 8; ++b) {
            const int ny = ly - code_dy(b), nx = lx - code_dx(b);   // a donor in direction b
            if (code[(ny + 1) * HS + nx + 1] != (1 << b)) continue;
            if (ny >= 0 && ny < TS && nx >= 0 && nx < TS) ++deg;
            else if (FINAL) seed += (uint32_t)word[slot_of(tile, tiles_x, ny, nx)];
        }
        indeg[i] = (uint8_t)deg;
        acc[i] = seed;
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    __syncthreads();

    // last donor continues: a walk starts at each cell without in-tile donors, adds its value
    // to its receiver with one returning 64-bit LDS atomic and goes on only if its arrival
    // completed the receiver.  Leaf status and completion come from indeg[] alone.
    for (int i = tid; i < TC; i += TNT) {
        if (indeg[i] != 0) continue;
        uint32_t v = (uint32_t)acc[i];
        uint16_t r = rl[i];
        for (int step = 0; step < TC && r < EXIT; ++step) {
            const uint64_t old = atomicAdd((unsigned long long *)&acc[r], ARRIVAL + v);
            // read while the atomic is in flight: one LDS latency per step
            const uint8_t need = indeg[r];
            const uint16_t next = rl[r];
            if ((uint32_t)(old >> 32) + 1 != need) break;
            v += (uint32_t)old;
            r = next;
        }
    }
    __syncthreads();

    if (FINAL) {
        unsigned int stuck = 0;
        for (int i = tid; i < TC; i += TNT) {
            const int ly = i / TS, lx = i % TS;
            if (indeg[i] == OUTSIDE) continue;
            const uint64_t a = acc[i];
            if ((uint32_t)(a >> 32) != indeg[i]) ++stuck;
            out[(size_t)(y0 + ly) * W + x0 + lx] = (uint32_t)a;
        }
        unsigned int stuck_b = 0;
        if (tid < PER && tgt[base + tid] >= 0 &&
            (uint32_t)(word[base + tid] >> 32) != indeg_b[base + tid])
            ++stuck_b;
        if (stuck) atomicAdd(&s_cnt[1], stuck);
        if (stuck_b) atomicAdd(&s_cnt[2], stuck_b);
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[1]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[1]);
            if (s_cnt[2]) atomicAdd(&cnt->stuck_exits, (unsigned long long)s_cnt[2]);
        }
        return;
    }

    // A: the perimeter slots -- each exit's local value and the slot it drains into
    int p_ly = 0, p_lx = 0, p_cell = 0;
    bool p_in = false;
    if (tid < PER) {
        perim_cell(tid, p_ly, p_lx);
        p_cell = p_ly * TS + p_lx;
        p_in = tile.inside(p_ly, p_lx);
        const bool is_exit = p_in && rl[p_cell] == EXIT;
        int32_t to = -1;
        if (is_exit) {
            const int b = __builtin_ctz(code[(p_ly + 1) * HS + p_lx + 1]);
            to = (int32_t)slot_of(tile, tiles_x, p_ly + code_dy(b), p_lx + code_dx(b));
        }
        word[base + tid] = is_exit ? (uint32_t)acc[p_cell] : 0u;
        indeg_b[base + tid] = 0;
        tgt[base + tid] = to;
    }
    __syncthreads();

    // pointer jumping: jmp[c] -> the exit c's in-tile path reaches (an exit points at
    // itself), TERM when it ends in the tile.  Paths are shorter than 2^12 cells.
    uint16_t *jmp = reinterpret_cast<uint16_t *>(acc);
    uint16_t *jnx = jmp + TC;
    for (int i = tid; i < TC; i += TNT) {
        const uint16_t r = rl[i];
        jmp[i] = r == EXIT ? (uint16_t)i : r;
    }
    __syncthreads();
    for (int round = 0; round < 12; ++round) {
        for (int i = tid; i < TC; i += TNT) {
            const uint16_t a = jmp[i];
            jnx[i] = a == TERM ? TERM : jmp[a];
        }
        __syncthreads();
        uint16_t *t = jmp; jmp = jnx; jnx = t;
    }
    if (tid < PER) {
        int32_t l = -1;
        if (p_in) {
            const uint16_t e = jmp[p_cell];
            if (e != TERM && rl[e] == EXIT) l = (int32_t)(base + perim_pos(e / TS, e % TS));
        }
        link[base + tid] = l;
    }
    if (tid == 0 && s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
}

// B1: next(e) of every exit node (the exit its receiver's in-tile path reaches, -1 when that
// path ends in a terminal cell) and the forest in-degrees.  Grid-stride, so that the node
// count costs one global atomic per workgroup.
__global__ __launch_bounds__(NT) void flowacc_forest_degree_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ link,
    int32_t *__restrict__ next, uint32_t *__restrict__ indeg_b, flowacc_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_exits;
    if (threadIdx.x == 0) s_exits = 0;
    __syncthreads();
    unsigned int exits = 0;
    for (int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x; s < nslots;
         s += (int64_t)gridDim.x * NT) {
        const int32_t to = tgt[s];
        int32_t n = -1;
        if (to >= 0) {
            ++exits;
            n = link[to];
            if (n >= 0) atomicAdd(&indeg_b[n], 1u);
        }
        next[s] = n;
    }
    if (exits) atomicAdd(&s_exits, exits);
    __syncthreads();
    if (threadIdx.x == 0 && s_exits) atomicAdd(&cnt->exits, (unsigned long long)s_exits);
}

// B2: last-donor walks over the exit forest.  A node's final value is the low half of its
// word once its arrivals (high half) equal its in-degree.
__global__ __launch_bounds__(NT) void flowacc_forest_walk_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ next,
    const uint32_t *__restrict__ indeg_b, uint64_t *__restrict__ word,
    flowacc_counters *__restrict__ cnt)
{
    __shared__ int s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    int hops = 0;
    if (s < nslots && tgt[s] >= 0 && indeg_b[s] == 0) {
        int64_t e = s;
        uint32_t v = (uint32_t)word[e];
        for (int64_t step = 0; step < nslots; ++step) {
            const int32_t t = next[e];
            if (t < 0) break;
            const uint64_t old = __hip_atomic_fetch_add(&word[t], ARRIVAL + v, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            ++hops;
            if ((uint32_t)(old >> 32) + 1 != indeg_b[t]) break;
            v += (uint32_t)old;
            e = t;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) hops = max(hops, __shfl_xor(hops, m));
    if ((threadIdx.x & 63) == 0 && hops) atomicMax(&s_max, hops);
    __syncthreads();
    // most workgroups see a larger figure already there and skip the atomic
    if (threadIdx.x == 0 && s_max > __hip_atomic_load(&cnt->max_hops, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&cnt->max_hops, s_max);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_flowacc_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, uint32_t *out,
                                   hdem_flowacc_stats *stats)
{
    if (int rc = hdem_check_call(ctx, d8, out, H, W)) return rc;
    d8_grid g;
    if (int rc = d8_grid_of("flow accumulation", H, W, &g)) return rc;
    const int64_t cells = (int64_t)H * W, tiles = g.tiles, nslots = g.nslots;
    const int tiles_x = g.tiles_x;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    if (stats) *stats = hdem_flowacc_stats{};

    // arena: counters | word u64 | indeg_b u32 | link i32 | tgt i32 | next i32  (per slot)
    const size_t head = 256;
    const size_t bytes = head + (size_t)nslots * (8 + 4 * 4);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    flowacc_counters *cnt = reinterpret_cast<flowacc_counters *>(ws);
    uint64_t *word = reinterpret_cast<uint64_t *>(ws + head);
    uint32_t *indeg_b = reinterpret_cast<uint32_t *>(word + nslots);
    int32_t *link = reinterpret_cast<int32_t *>(indeg_b + nslots);
    int32_t *tgt = link + nslots;
    int32_t *next = tgt + nslots;

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(flowacc_counters), ctx->stream));
    const int64_t forest_blocks = (nslots + NT - 1) / NT;
    const int degree_blocks = (int)std::min<int64_t>(forest_blocks, (int64_t)ctx->num_cus * 8);
    {
        hdem_scoped_timer tm(ctx, HDEM_K_FLOWACC, cells);
        phases.mark(0);
        hipLaunchKernelGGL(flowacc_tile_kernel<false>, dim3((unsigned)tiles), dim3(TNT), 0,
                           ctx->stream, d8, H, W, tiles_x, out, word, indeg_b, link, tgt, cnt);
        phases.mark(1);
        hipLaunchKernelGGL(flowacc_forest_degree_kernel, dim3(degree_blocks), dim3(NT), 0,
                           ctx->stream, nslots, tgt, link, next, indeg_b, cnt);
        hipLaunchKernelGGL(flowacc_forest_walk_kernel, dim3((unsigned)forest_blocks), dim3(NT), 0,
                           ctx->stream, nslots, tgt, next, indeg_b, word, cnt);
        phases.mark(2);
        hipLaunchKernelGGL(flowacc_tile_kernel<true>, dim3((unsigned)tiles), dim3(TNT), 0,
                           ctx->stream, d8, H, W, tiles_x, out, word, indeg_b, link, tgt, cnt);
        phases.mark(3);
    }
    HDEM_HIP_CHECK(hipGetLastError());
    flowacc_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (stats) {
        stats->exits = (int64_t)host.exits;
        stats->max_hops = host.max_hops;
        stats->tile_h = TS;
        stats->tile_w = TS;
        phases.read(&stats->ms_tile, &stats->ms_forest, &stats->ms_final);
    }
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_exits, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never drain (%llu of them inside "
                 "tiles, %llu tile exits)",
                 host.stuck_cells + host.stuck_exits, host.stuck_cells, host.stuck_exits);
    return HDEM_OK;
}

extern "C" int hdem_flowacc_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, uint32_t *out,
                               hdem_flowacc_stats *stats)
{
    if (int rc = hdem_check_call(ctx, d8, out, H, W)) return rc;
    d8_grid g;
    if (int rc = d8_grid_of("flow accumulation", H, W, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W, bytes = n * sizeof(uint32_t);
    hdem_dbuf dd8, dout;
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dout.alloc(ctx, bytes)) return rc;
    if (int rc = hdem_flowacc_u8_dev(ctx, dd8.as<const uint8_t>(), H, W, dout.as<uint32_t>(),
                                     stats))
        return rc;
    return dout.download(out, bytes);
}
