// D8 flow trace (new operators; FlowDistance, HeightAboveDrainage, DemToHAND).
//
// For every cell c: s(c), the first *stop* on c's D8 path (c included), and ncard(c) /
// ndiag(c), the cardinal and diagonal steps taken to get there.  A stop is a terminal cell
// (code 0 or pointing outside the raster) or, when streams are given, a stream cell
// (mask != 0, or acc >= threshold).  With streams, a terminal cell that is no stream cell is
// *dry*: it and everything that ends in it are unreached (stop 0, distance and HAND NaN, the
// counts still those to the terminal).  "First stop downstream" and "steps to it" compose
// along a path, (stop, n) o (stop', n') = (stop', n + n'), so the scheme is that of
// hdem_watershed.hip with a payload on every pointer: the codes, 64 x 64 tiles, 252 perimeter
// slots per tile and a forest over the slots of hdem_d8tile.h, pointer jumping, no atomics on
// the data path.
//   A  (flowtrace_tile_kernel)   per tile: every cell's in-tile receiver, then Jacobi pointer
//      doubling in LDS on 64-bit words (pointer | ncard << 16 | ndiag << 32; a path inside a
//      tile has at most 4095 steps) until every cell points at a stop or at an *exit* (a
//      cell that is no stop and whose receiver lies in a neighbouring tile).  Writes 6 B per
//      cell (2 B: which stop / which exit; 4 B: the in-tile counts and the dry bit) and one
//      16-byte forest node per perimeter slot: "resolved, stop S, counts" when the frame
//      cell's in-tile path ends in a stop, else "next = the slot of the cell its exit drains
//      into, counts up to and including the crossing step".  The stream test reads the
//      cell's own value: no tile looks at the streams of its halo.
//   B  (flowtrace_forest_kernel) pointer jumping with payload over the slot nodes,
//      node <- (next(next), n + n').  A node is 16 bytes, wider than any single naturally
//      atomic word, so nothing is done in place: there are two node arrays, launch r reads
//      only array r & 1 and writes only array (r + 1) & 1, every node every launch, and the
//      launches are ordered by the stream.  No reader can see a half-written node because no
//      launch reads what it writes.  The host enqueues ceil(log2 slots) + 1 launches; a
//      launch whose predecessor left nothing unresolved returns at once (the count stays on
//      the device), so a cycle costs the full schedule and nothing more.  C works out from
//      the same counts which array holds the result.
//   C  (flowtrace_final_kernel)  per tile, streaming: the tile's 252 resolved nodes in LDS,
//      6 B per cell in, 4 B per cell and wanted output out.  HAND gathers dem[s(c)].
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per forest / final workgroup
constexpr int TNT = 1024;             // threads per tile workgroup (4 cells each; the LDS
                                      // allows two workgroups per CU whatever their size: A at
                                      // 16384^2 takes 3.48 ms with 256, 2.17 with 512, 1.72
                                      // with 1024)
constexpr int JUMPS = 4;              // forest jumps per node and launch, all in the source
                                      // array (B at 16384^2, distance to the outlet: 1.01 ms
                                      // with 1, 0.71 with 2, 0.54 with 4)
constexpr uint32_t C_DRY = 1u << 31;  // per-cell counts word: the stop reached is a dry terminal
constexpr uint32_t RESOLVED = 1u;     // node.y

// kind[] of a cell
constexpr uint8_t K_TRAVEL = 0;       // has an in-tile receiver
constexpr uint8_t K_EXIT = 1;         // receiver in a neighbouring tile, cell no stop
constexpr uint8_t K_STOP = 2;         // terminal or stream cell (outside the raster too)
constexpr uint8_t K_DRY = 3;          // terminal, streams given, no stream cell

// node: x = stop (1 + flat index, 0 = dry) when resolved, else the next slot; y = RESOLVED or
// 0; z = ncard; w = ndiag
typedef uint4 node_t;

struct flowtrace_counters : d8_forest_counters {
    unsigned long long stops;         // stop cells (stream cells and terminal cells)
    unsigned long long unreached;     // cells whose path ends in a dry terminal
};
constexpr size_t FT_HEAD = 512;      // the counters' block at the head of the arena
static_assert(sizeof(flowtrace_counters) <= FT_HEAD, "counters outgrew their block");

// LDS word of A: pointer in bits 0-15, ncard in 16-31, ndiag in 32-47.  A stop or an exit
// holds (itself, 0, 0), so composing "a then b" is one addition of b to a's counts.
__device__ __forceinline__ uint32_t w_ptr(uint64_t w) { return (uint32_t)w & 0xFFFFu; }
__device__ __forceinline__ uint32_t w_nc(uint64_t w) { return (uint32_t)(w >> 16) & 0xFFFFu; }
__device__ __forceinline__ uint32_t w_nd(uint64_t w) { return (uint32_t)(w >> 32) & 0xFFFFu; }

// A.  STREAMS 0: none, 1: uint8 mask, 2: uint32 raster against a threshold.
template <int STREAMS>
__global__ __launch_bounds__(TNT) void flowtrace_tile_kernel(
    const uint8_t *__restrict__ d8, const void *__restrict__ streams, uint32_t threshold, int H,
    int W, int tiles_x, uint16_t *__restrict__ target, uint32_t *__restrict__ counts,
    node_t *__restrict__ node, flowtrace_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[TC];
    __shared__ uint8_t kind[TC];
    __shared__ uint64_t jump[2][TC];
    __shared__ unsigned int s_cnt[4];            // invalid codes, stops, exits, stuck cells

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;

    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    // receivers; a stop or an exit points at itself with no steps taken
    unsigned int bad = 0, stops = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        uint8_t k = K_STOP;
        uint64_t w = (uint64_t)i;
        int c = 0;
        if (tile.inside(ly, lx)) {
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            c = d8[g];
            bool stream = false;
            if (STREAMS == 1) stream = static_cast<const uint8_t *>(streams)[g] != 0;
            if (STREAMS == 2) stream = static_cast<const uint32_t *>(streams)[g] >= threshold;
            const d8_step s = d8_decode(c, ly, lx, tile, H, W);
            if (s.invalid) ++bad;
            if (stream || s.terminal) {
                k = (STREAMS == 0 || stream) ? K_STOP : K_DRY;
                ++stops;
            } else if (s.in_tile()) {
                k = K_TRAVEL;
                w = (uint64_t)(s.ny * TS + s.nx) | ((s.b & 1) ? 1ull << 32 : 1ull << 16);
            } else {
                k = K_EXIT;
            }
        }
        code[i] = (uint8_t)c;
        kind[i] = k;
        jump[0][i] = w;
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (stops) atomicAdd(&s_cnt[1], stops);
    __syncthreads();

    // pointer doubling: after round k a cell points 2^k steps down its in-tile path, or at
    // the stop / exit that ends it, and carries the steps to where it points
    int cur = 0;
    for (int round = 0; round < DOUBLINGS; ++round) {
        int changed = 0;
        for (int i = tid; i < TC; i += TNT) {
            const uint64_t a = jump[cur][i];
            const uint64_t b = jump[cur][w_ptr(a)];
            jump[cur ^ 1][i] = (a & ~0xFFFFull) + b;     // a's counts + b's counts, b's pointer
            changed |= w_ptr(a) != w_ptr(b);
        }
        cur ^= 1;
        if (!__syncthreads_or(changed)) break;
    }
    const uint64_t *jmp = jump[cur];

    // 6 B per cell for C: the stop (local index) or the exit (perimeter slot) it reaches,
    // and the steps to it
    unsigned int stuck = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const uint64_t w = jmp[i];
        const uint32_t t = w_ptr(w);
        const uint8_t k = kind[t];
        if (k == K_TRAVEL) ++stuck;                      // a cycle inside the tile
        target[(size_t)blockIdx.x * TC + i] =
            k == K_EXIT ? (uint16_t)(T_EXIT | perim_pos(t / TS, t % TS)) : (uint16_t)t;
        counts[(size_t)blockIdx.x * TC + i] =
            (w_nc(w) & 0xFFFu) | ((w_nd(w) & 0xFFFu) << 12) | (k == K_DRY ? C_DRY : 0u);
    }
    if (stuck) atomicAdd(&s_cnt[3], stuck);

    // the perimeter slots
    if (tid < PER) {
        int ly, lx;
        perim_cell(tid, ly, lx);
        node_t n = make_uint4(0u, RESOLVED, 0u, 0u);     // outside the raster: never read
        if (tile.inside(ly, lx)) {
            const int i = ly * TS + lx;
            const uint64_t w = jmp[i];
            const int t = (int)w_ptr(w);
            const uint8_t k = kind[t];
            const int t_ly = t / TS, t_lx = t % TS;
            n.z = w_nc(w);
            n.w = w_nd(w);
            if (k == K_STOP) {
                n.x = (uint32_t)((size_t)(y0 + t_ly) * W + x0 + t_lx) + 1u;
            } else if (k == K_DRY) {
                n.x = 0u;
            } else if (k == K_EXIT) {
                const int b = __builtin_ctz(code[t]);
                n.x = (uint32_t)slot_of(tile, tiles_x, t_ly + code_dy(b), t_lx + code_dx(b));
                n.y = 0u;
                if (b & 1) ++n.w; else ++n.z;            // the crossing step
            } else {
                n = make_uint4((uint32_t)(tile.base + tid), 0u, 0u, 0u);   // a cycle: unresolved
            }
            if (kind[i] == K_EXIT) atomicAdd(&s_cnt[2], 1u);
        }
        node[tile.base + tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->stops, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->exits, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[3]);
    }
}

// B: one round of pointer jumping with payload, src -> dst.  Grid-stride.
__global__ __launch_bounds__(NT) void flowtrace_forest_kernel(int64_t nslots, int round,
                                                              const node_t *__restrict__ src,
                                                              node_t *__restrict__ dst,
                                                              flowtrace_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_left;
    if (!d8_forest_begin(cnt, round, &s_left)) return;
    unsigned int left = 0;
    for (int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x; s < nslots;
         s += (int64_t)gridDim.x * NT) {
        node_t n = src[s];
        for (int j = 0; j < JUMPS && !(n.y & RESOLVED); ++j) {
            const node_t t = src[n.x];                   // my pointer's node, as the last launch left it
            n = make_uint4(t.x, t.y, n.z + t.z, n.w + t.w);
        }
        dst[s] = n;
        left += !(n.y & RESOLVED);
    }
    d8_forest_end(cnt, round, left, &s_left);
}

// C.  Every output pointer may be null (not wanted).  cs2 = cellsize * sqrt(2), in double.
__global__ __launch_bounds__(NT) void flowtrace_final_kernel(
    int H, int W, int tiles_x, int rounds, const uint16_t *__restrict__ target,
    const uint32_t *__restrict__ counts, const node_t *__restrict__ node0,
    const node_t *__restrict__ node1, const float *__restrict__ dem, double cs, double cs2,
    uint32_t *__restrict__ out_stop, uint32_t *__restrict__ out_nc, uint32_t *__restrict__ out_nd,
    float *__restrict__ out_dist, float *__restrict__ out_hand,
    flowtrace_counters *__restrict__ cnt)
{
    __shared__ uint32_t n_stop[PER], n_nc[PER], n_nd[PER];
    __shared__ uint8_t known[PER];
    __shared__ unsigned int s_cnt[3];            // stuck cells, stuck slots, unreached cells

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const uint16_t *tg = target + (size_t)blockIdx.x * TC;
    const uint32_t *ct = counts + (size_t)blockIdx.x * TC;

    if (tid < 3) s_cnt[tid] = 0;
    if (tid < PER) {
        // launch r of B wrote array (r + 1) & 1; the first that left nothing unresolved wrote
        // the result, and every later one returned at once
        int r = 0;
        while (r < rounds - 1 && cnt->unresolved[r]) ++r;
        const node_t n = (((r + 1) & 1) ? node1 : node0)[tile.base + tid];
        const bool ok = (n.y & RESOLVED) != 0;
        n_stop[tid] = ok ? n.x : 0u;                     // a slot number is no cell to gather from
        n_nc[tid] = n.z;
        n_nd[tid] = n.w;
        known[tid] = ok;
    }
    __syncthreads();
    if (tid < PER && !known[tid]) atomicAdd(&s_cnt[1], 1u);

    const float nan = __builtin_nanf("");
    unsigned int stuck = 0, unreached = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        const uint16_t v = tg[i];
        const uint32_t c = ct[i];
        uint32_t nc = c & 0xFFFu, nd = (c >> 12) & 0xFFFu, stop;
        if (v & T_EXIT) {
            const int p = v & 0xFF;
            stop = n_stop[p];
            nc += n_nc[p];
            nd += n_nd[p];
            stuck += !known[p];
        } else {
            stop = (c & C_DRY) ? 0u : (uint32_t)((size_t)(y0 + v / TS) * W + x0 + v % TS) + 1u;
        }
        unreached += stop == 0u;
        if (out_stop) out_stop[g] = stop;
        if (out_nc) out_nc[g] = nc;
        if (out_nd) out_nd[g] = nd;
        if (out_dist)
            out_dist[g] = stop ? __double2float_rn(__dadd_rn(__dmul_rn((double)nc, cs),
                                                             __dmul_rn((double)nd, cs2)))
                               : nan;
        if (out_hand) out_hand[g] = stop ? __fsub_rn(dem[g], dem[stop - 1u]) : nan;
    }
    if (stuck) atomicAdd(&s_cnt[0], stuck);
    if (unreached) atomicAdd(&s_cnt[2], unreached);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->stuck_slots, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->unreached, (unsigned long long)s_cnt[2]);
    }
}

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
               int stream_kind, uint32_t threshold, const float *dem, double cellsize,
               const uint32_t *stop, const uint32_t *ncard, const uint32_t *ndiag,
               const float *distance, const float *hand, int flags,
               const hdem_flowtrace_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, d8, d8, H, W)) return rc;
    if (int rc = d8_grid_of("flow trace", H, W, g)) return rc;
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "unknown flow trace flags 0x%x", flags);
    HDEM_REQUIRE(stop || ncard || ndiag || distance || hand, HDEM_ERR_BAD_ARG,
                 "no output wanted: give at least one of stop, ncard, ndiag, distance, hand");
    HDEM_REQUIRE(!hand || dem, HDEM_ERR_BAD_ARG, "hand needs the dem it is measured on");
    if (int rc = d8_check_streams(streams, stream_kind, threshold)) return rc;
    HDEM_REQUIRE(std::isfinite(cellsize) && cellsize > 0.0, HDEM_ERR_BAD_ARG,
                 "cellsize must be finite and positive, got %g", cellsize);
    return d8_check_stats(stats, "hdem_flowtrace_stats");
}

}  // namespace

// The arena the trace takes for a raster of `tiles` tiles: an operator that calls it and keeps
// views of its own in the arena puts them behind these bytes (hdem_d8tile.h).
size_t hdem_flowtrace_arena_bytes(int64_t tiles, int64_t nslots)
{
    return FT_HEAD + (size_t)nslots * 32 + (size_t)tiles * TC * 6;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_flowtrace_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                     const void *streams, int stream_kind, uint32_t threshold,
                                     const float *dem, double cellsize, uint32_t *stop,
                                     uint32_t *ncard, uint32_t *ndiag, float *distance,
                                     float *hand, int flags, hdem_flowtrace_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, streams, stream_kind, threshold, dem, cellsize, stop,
                            ncard, ndiag, distance, hand, flags, stats, &g))
        return rc;
    const int tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, nslots = g.nslots;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_flowtrace_stats st = {};
    d8_publish(stats, st);

    // arena: counters | two node arrays, 16 B per slot each | counts u32 per cell | target
    // u16 per cell
    const size_t head = FT_HEAD;
    const size_t bytes = hdem_flowtrace_arena_bytes(tiles, nslots);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    flowtrace_counters *cnt = reinterpret_cast<flowtrace_counters *>(ws);
    node_t *node[2] = {reinterpret_cast<node_t *>(ws + head),
                       reinterpret_cast<node_t *>(ws + head) + nslots};
    uint32_t *counts = reinterpret_cast<uint32_t *>(node[1] + nslots);
    uint16_t *target = reinterpret_cast<uint16_t *>(counts + (size_t)tiles * TC);

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(flowtrace_counters), ctx->stream));
    const d8_forest_plan forest = d8_forest_plan_of(ctx, nslots, NT);
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    if (stream_kind == HDEM_FT_STREAMS_NONE)
        hipLaunchKernelGGL(flowtrace_tile_kernel<0>, grid, dim3(TNT), 0, ctx->stream, d8, streams,
                           threshold, H, W, tiles_x, target, counts, node[0], cnt);
    else if (stream_kind == HDEM_FT_STREAMS_MASK_U8)
        hipLaunchKernelGGL(flowtrace_tile_kernel<1>, grid, dim3(TNT), 0, ctx->stream, d8, streams,
                           threshold, H, W, tiles_x, target, counts, node[0], cnt);
    else
        hipLaunchKernelGGL(flowtrace_tile_kernel<2>, grid, dim3(TNT), 0, ctx->stream, d8, streams,
                           threshold, H, W, tiles_x, target, counts, node[0], cnt);
    phases.mark(1);
    for (int r = 0; r < forest.rounds; ++r)
        hipLaunchKernelGGL(flowtrace_forest_kernel, dim3(forest.grid), dim3(NT), 0, ctx->stream,
                           nslots, r, node[r & 1], node[(r + 1) & 1], cnt);
    phases.mark(2);
    const double cs2 = cellsize * std::sqrt(2.0);
    hipLaunchKernelGGL(flowtrace_final_kernel, grid, dim3(NT), 0, ctx->stream, H, W, tiles_x,
                       forest.rounds, target, counts, node[0], node[1], dem, cellsize, cs2, stop,
                       ncard, ndiag, distance, hand, cnt);
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    flowtrace_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.stops = (int64_t)host.stops;
    st.unreached = (int64_t)host.unreached;
    st.exits = (int64_t)host.exits;
    st.forest_rounds = d8_forest_rounds(forest, host);
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_tile, &st.ms_forest, &st.ms_final);
    d8_publish(stats, st);
    return d8_report_forest(host);
}

extern "C" int hdem_flowtrace_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                 const void *streams, int stream_kind, uint32_t threshold,
                                 const float *dem, double cellsize, uint32_t *stop,
                                 uint32_t *ncard, uint32_t *ndiag, float *distance, float *hand,
                                 int flags, hdem_flowtrace_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, streams, stream_kind, threshold, dem, cellsize, stop,
                            ncard, ndiag, distance, hand, flags, stats, &g))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dstreams, ddem, dout[5];
    const size_t sb = n * (stream_kind == HDEM_FT_STREAMS_ACC_U32 ? sizeof(uint32_t) : 1);
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dstreams.upload(ctx, streams, sb)) return rc;
    if (int rc = ddem.upload(ctx, dem, n * sizeof(float))) return rc;
    void *const host_out[5] = {stop, ncard, ndiag, distance, hand};
    for (int k = 0; k < 5; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, n * 4)) return rc;
    const int rc = hdem_flowtrace_u8_dev(
        ctx, dd8.as<const uint8_t>(), H, W, dstreams.p, stream_kind, threshold,
        ddem.as<const float>(), cellsize, dout[0].as<uint32_t>(), dout[1].as<uint32_t>(),
        dout[2].as<uint32_t>(), dout[3].as<float>(), dout[4].as<float>(), flags, stats);
    if (rc) return rc;
    for (int k = 0; k < 5; ++k)
        if (host_out[k])
            if (int rc2 = dout[k].download(host_out[k], n * 4)) return rc2;
    return HDEM_OK;
}
