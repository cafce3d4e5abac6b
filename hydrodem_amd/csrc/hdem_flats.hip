// D8 flat resolution (new operator; ResolveFlats).
//
// D8 routes strictly downhill, so every cell of a flat keeps code 0.  This operator gives the
// flat cells a direction towards the nearest way out of their flat.  Definitions (all exact;
// "equal" is float ==, so -0.0 equals 0.0 and NaN equals nothing):
//   S  (drains)  non-NaN cells with a code != 0, or on the one-cell raster ring, or with a NaN
//                8-neighbour.
//   F  (flat)    the other non-NaN cells.
//   dist[c], c in F: the length k >= 1 of the shortest 8-connected path c = p0 ... pk of cells
//                of c's elevation with p0 ... p(k-1) in F and pk in S; infinite (0xFFFFFFFF)
//                when there is none -- a pit of an unfilled DEM.
//   out[c]       for c in F with finite dist the code of the first neighbour n in D8 window
//                order (NW, N, NE, W, E, SW, S, SE) with dem[n] == dem[c] and
//                dist[n] == dist[c] - 1, S counting as 0; codes[c] everywhere else.
// dist is the unique solution of dist[c] = 1 + min over equal neighbours (0 in S, else dist),
// infinite where no equal neighbour is finite; it strictly decreases along the new pointers.
//
// The working raster is dist itself, uint32 per cell: 0 outside F (NaN cells too: no equality
// ever looks at them), and in F an upper bound that only ever is the length of a real path.
//   classify  (flats_classify_kernel)  per tile: dist = 0 / infinite, flat cells and invalid
//             bytes counted, the tiles that hold a flat cell marked and listed for round 0.
//   relax     (flats_relax_kernel)  one workgroup per listed tile: dem and dist of the tile and
//             its one-cell halo in LDS, then dist[c] <- min(dist[c], 1 + dist[n]) over equal
//             neighbours until the tile stops changing.  One iteration is four directional
//             sweeps, one wave each, all four at once: down the rows, up the rows, along the
//             columns to the right and to the left, 64 steps with the three neighbours of the
//             previous line each.  A sweep carries a distance along a whole straight or
//             diagonal run in one pass, so a spiral of 2 000 steps takes about as many
//             iterations as it has legs, not 2 000.  The waves race on the same cells through
//             LDS atomic min, so a cell never goes up.  The tile is written back where it
//             changed; if a frame cell changed, the tile stamps the round.
//   schedule  (flats_schedule_kernel)  between rounds: a tile with flat cells runs again when one
//             of its eight neighbours stamped the last round.  The host reads the length of
//             the list (one word per round) and launches that many workgroups; an empty list
//             ends the relaxation.
//   final     (flats_final_kernel)  streaming: the code of every flat cell, unresolved cells
//             and the largest distance counted -- and the local equation above checked at
//             every flat cell, so the result is certified, not assumed: a violation is
//             HDEM_ERR_NOT_CONVERGED.
// Schedule freedom: every value a cell ever holds is the length of a real path (min-plus in
// place of the minimax of the sink fill), the halo a tile reads is what a neighbour wrote in
// some earlier or the same round, and a neighbour that lowers a frame cell afterwards stamps
// its round, which puts the tile on the next list.  So stale reads only cost rounds, no
// workgroup waits for another, and there are no fences.  Bounds: an iteration that changes
// the tile makes at least one more cell final, so at most 4096 iterations; a round that
// changes anything makes final every cell whose shortest path crosses one more tile seam, so
// at most H * W rounds (a path may cross the same seam many times: the bound is not the
// tile count).
#include "hdem_d8tile.h"

namespace {

constexpr int NT = 256;               // threads per workgroup, every kernel here
constexpr int LH = TS + 2;            // LDS rows: the tile and its halo
constexpr int LW = TS + 3;            // LDS row pitch: odd, so a column sweep (one lane per
                                      // row) hits 64 different banks
constexpr uint32_t INF = 0xFFFFFFFFu;

struct flats_counters {
    unsigned long long flat_cells;
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long unresolved;
    unsigned long long violations;    // flat cells at which the local equation fails
    unsigned int max_distance;
    unsigned int active_tiles;        // tiles holding a flat cell
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
};

// D8 window order (oracle/hdem_oracle_np.py D8_OFFSETS / D8_CODES): the ESRI bit of window
// position j, 4 bits each
__device__ __forceinline__ int window_bit(int j) { return (0x12304765u >> (4 * j)) & 7; }

__global__ __launch_bounds__(NT) void flats_classify_kernel(
    const uint8_t *__restrict__ d8, const float *__restrict__ dem, int H, int W, int tiles_x,
    uint32_t *__restrict__ dist, uint32_t *__restrict__ active, uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ list, flats_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[2];            // flat cells, invalid bytes
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int flat = 0, bad = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const int gy = tile.y0 + ly, gx = tile.x0 + lx;
        const size_t g = (size_t)gy * W + gx;
        const uint8_t c = d8[g];
        const float z = dem[g];
        bad += (c & (c - 1)) != 0;
        uint32_t v = 0;
        if (c == 0 && z == z && gy > 0 && gy < H - 1 && gx > 0 && gx < W - 1) {
            bool nodata = false;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const float n = dem[g + (ptrdiff_t)dy * W + dx];
                    nodata |= n != n;
                }
            if (!nodata) {
                v = INF;
                ++flat;
            }
        }
        dist[g] = v;
    }
    if (flat) atomicAdd(&s_cnt[0], flat);
    if (bad) atomicAdd(&s_cnt[1], bad);
    __syncthreads();
    if (tid == 0) {
        active[blockIdx.x] = s_cnt[0] != 0;
        stamp[blockIdx.x] = 0;
        if (s_cnt[0]) {
            atomicAdd(&cnt->flat_cells, (unsigned long long)s_cnt[0]);
            atomicAdd(&cnt->active_tiles, 1u);
            list[atomicAdd(&cnt->listed, 1u)] = blockIdx.x;
        }
        if (s_cnt[1]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[1]);
    }
}

// The list of round `round` >= 1: the tiles with flat cells next to a tile whose frame changed
// in round - 1.  One thread per tile; the order of the list is whatever the atomics give and
// changes no result.
__global__ __launch_bounds__(NT) void flats_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ active,
    const uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    flats_counters *__restrict__ cnt)
{
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= (int64_t)tiles_y * tiles_x || !active[t]) return;
    const int ty = (int)(t / tiles_x), tx = (int)(t % tiles_x);
    bool run = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int ny = ty + dy, nx = tx + dx;
            if ((dy || dx) && ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
                run |= stamp[(int64_t)ny * tiles_x + nx] == round;
        }
    if (run) list[atomicAdd(&cnt->listed, 1u)] = (uint32_t)t;
}

__global__ __launch_bounds__(NT) void flats_relax_kernel(
    const float *__restrict__ dem, uint32_t *dist, int H, int W, int tiles_x,
    const uint32_t *__restrict__ list, uint32_t round, uint32_t *__restrict__ stamp)
{
    __shared__ float z[LH * LW];
    __shared__ uint32_t d[LH * LW];
    __shared__ unsigned int s_edge;

    const int tid = threadIdx.x;
    const uint32_t t = list[blockIdx.x];
    const int y0 = (int)(t / tiles_x) * TS, x0 = (int)(t % tiles_x) * TS;
    if (tid == 0) s_edge = 0;

    // the tile and its halo; outside the raster: NaN, which equals nothing
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = (size_t)gy * W + gx;
        z[hy * LW + hx] = in ? dem[g] : __builtin_nanf("");
        d[hy * LW + hx] = in ? dist[g] : 0u;
    }
    __syncthreads();

    // wave 0 sweeps down the rows, 1 up, 2 along the columns to the right, 3 to the left; the
    // lane is the position in the line.  c0: the cell of step 0, step: to the next line,
    // side: to the neighbour in the line (LDS indices, halo included).
    const int wave = tid >> 6, lane = tid & 63;
    const int step = wave == 0 ? LW : wave == 1 ? -LW : wave == 2 ? 1 : -1;
    const int side = wave < 2 ? 1 : LW;
    const int c0 = wave == 0   ? LW + lane + 1
                   : wave == 1 ? TS * LW + lane + 1
                   : wave == 2 ? (lane + 1) * LW + 1
                               : (lane + 1) * LW + TS;
    bool any = false;
    for (int iter = 0; iter < TC; ++iter) {
        int changed = 0;
        for (int s = 0, c = c0; s < TS; ++s, c += step) {
            const uint32_t dc = d[c];
            if (dc) {                                    // a flat cell
                const float zc = z[c];
                const int p = c - step;
                uint32_t best = dc;
                for (int k = -1; k <= 1; ++k) {
                    const int n = p + k * side;
                    const uint32_t dn = d[n];
                    if (z[n] == zc && dn != INF && dn + 1 < best) best = dn + 1;
                }
                if (best < dc) {
                    atomicMin(&d[c], best);
                    changed = 1;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(changed)) break;
        any = true;
    }
    if (!any) return;

    unsigned int edge = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const size_t g = (size_t)gy * W + gx;
        const uint32_t v = d[(ly + 1) * LW + lx + 1];
        if (v != dist[g]) {                              // only this workgroup writes these cells
            dist[g] = v;
            edge |= ly == 0 || ly == TS - 1 || lx == 0 || lx == TS - 1;
        }
    }
    if (edge) atomicOr(&s_edge, 1u);
    __syncthreads();
    if (tid == 0 && s_edge) stamp[t] = round + 1;
}

__global__ __launch_bounds__(NT) void flats_final_kernel(
    const uint8_t *d8, const float *__restrict__ dem, const uint32_t *__restrict__ dist, int H,
    int W, int tiles_x, uint8_t *out, flats_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[3];            // unresolved, violations, largest distance
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int unresolved = 0, violations = 0, far = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        uint8_t code = d8[g];
        const uint32_t k = dist[g];
        if (k) {                                         // a flat cell: interior, 8 neighbours
            const float zc = dem[g];
            uint32_t nearest = INF;
            int pick = -1;
            for (int j = 0; j < 8; ++j) {
                const int b = window_bit(j);
                const size_t n = g + (ptrdiff_t)code_dy(b) * W + code_dx(b);
                if (dem[n] != zc) continue;
                const uint32_t dn = dist[n];
                nearest = min(nearest, dn);
                if (pick < 0 && dn == k - 1) pick = b;
            }
            violations += k != (nearest == INF ? INF : nearest + 1);
            if (k == INF) {
                ++unresolved;
            } else {
                code = pick < 0 ? 0 : (uint8_t)(1u << pick);
                far = max(far, k);
            }
        }
        out[g] = code;
    }
    if (unresolved) atomicAdd(&s_cnt[0], unresolved);
    if (violations) atomicAdd(&s_cnt[1], violations);
    if (far) atomicMax(&s_cnt[2], far);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->unresolved, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->violations, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicMax(&cnt->max_distance, s_cnt[2]);
    }
}

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const uint8_t *d8, const float *dem, int H, int W,
               const uint8_t *out, int flags, const hdem_resolve_flats_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, d8, out, H, W)) return rc;
    HDEM_REQUIRE(dem, HDEM_ERR_BAD_ARG, "flat resolution needs the dem the codes were made on");
    if (int rc = d8_grid_of("flat resolution", H, W, g)) return rc;
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "unknown flat resolution flags 0x%x", flags);
    return d8_check_stats(stats, "hdem_resolve_flats_stats");
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_resolve_flats_u8_dev(hdem_ctx *ctx, const uint8_t *d8, const float *dem,
                                         int H, int W, uint8_t *out, uint32_t *dist, int flags,
                                         hdem_resolve_flats_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, dem, H, W, out, flags, stats, &g)) return rc;
    const int tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_resolve_flats_stats st = {};
    d8_publish(stats, st);

    // arena: counters | active, stamp, list: u32 per tile each | the working raster, u32 per
    // cell, unless the caller's dist serves
    const size_t head = 512;
    static_assert(sizeof(flats_counters) <= head, "counters outgrew their block");
    const size_t bytes = head + (size_t)tiles * 12 + (dist ? 0 : (size_t)cells * 4);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    flats_counters *cnt = reinterpret_cast<flats_counters *>(ws);
    uint32_t *active = reinterpret_cast<uint32_t *>(ws + head);
    uint32_t *stamp = active + tiles, *list = stamp + tiles;
    uint32_t *work = dist ? dist : list + tiles;

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(flats_counters), ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    hipLaunchKernelGGL(flats_classify_kernel, grid, dim3(NT), 0, ctx->stream, d8, dem, H, W,
                       tiles_x, work, active, stamp, list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    flats_counters host = {};
    int64_t rounds = 0, visits = 0;
    for (;; ++rounds) {
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
        HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (host.bad || !host.listed || rounds > cells) break;
        visits += host.listed;
        hipLaunchKernelGGL(flats_relax_kernel, dim3(host.listed), dim3(NT), 0, ctx->stream, dem,
                           work, H, W, tiles_x, list, (uint32_t)rounds, stamp);
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(flats_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           active, stamp, list, cnt);
    }
    phases.mark(2);
    if (!host.bad) {
        hipLaunchKernelGGL(flats_final_kernel, grid, dim3(NT), 0, ctx->stream, d8, dem, work, H,
                           W, tiles_x, out, cnt);
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (int rc = d8_report_invalid(host.bad)) return rc;

    st.rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
    st.flat_cells = (int64_t)host.flat_cells;
    st.unresolved = (int64_t)host.unresolved;
    st.tile_visits = visits;
    st.max_distance = host.max_distance;
    st.active_tiles = (int32_t)host.active_tiles;
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_classify, &st.ms_relax, &st.ms_final);
    d8_publish(stats, st);
    HDEM_REQUIRE(!host.listed && !host.violations, HDEM_ERR_NOT_CONVERGED,
                 "flat resolution is not certified after %lld rounds: the distance of %llu flat "
                 "cells is not 1 + that of their nearest equal neighbour",
                 (long long)rounds, host.violations);
    return HDEM_OK;
}

extern "C" int hdem_resolve_flats_u8(hdem_ctx *ctx, const uint8_t *d8, const float *dem, int H,
                                     int W, uint8_t *out, uint32_t *dist, int flags,
                                     hdem_resolve_flats_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, dem, H, W, out, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, ddem, ddist;
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = ddem.upload(ctx, dem, n * sizeof(float))) return rc;
    if (dist)
        if (int rc = ddist.alloc(ctx, n * sizeof(uint32_t))) return rc;
    // the codes are resolved in place on the device
    if (int rc = hdem_resolve_flats_u8_dev(ctx, dd8.as<const uint8_t>(), ddem.as<const float>(), H,
                                           W, dd8.as<uint8_t>(), ddist.as<uint32_t>(), flags,
                                           stats))
        return rc;
    if (int rc = dd8.download(out, n)) return rc;
    return dist ? ddist.download(dist, n * sizeof(uint32_t)) : HDEM_OK;
}
