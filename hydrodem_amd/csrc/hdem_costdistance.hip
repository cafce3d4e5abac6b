// Cost distance, back link and allocation (new operator; CostDistance, CostAllocation).
//
// The least accumulated cost from every cell to a source set S when crossing a cell has a
// price; include/hydrodem_hip.h (A28) has the contract.  In short, all in integers:
//   q(c)      (int64)rint((double)cost[c] * 2^frac_bits), 1 ... 2^28 - 1; a NaN cost is a barrier,
//             a cell outside the graph
//   w(a, b)   s = q(a) + q(b) for a cardinal step, (s * 3037000500 + 2^30) >> 31 for a diagonal
//   D[c]      0 in S, else the least sum of w over the 8-connected paths from c to S; infinite
//             (2^64 - 1) where there is none
//   backlink  the code of the first neighbour n in D8 window order (NW, N, NE, W, E, SW, S, SE)
//             with D[n] + w(c, n) == D[c]
// D is the unique solution of D[S] = 0, D[c] = min over neighbours n of D[n] + w(c, n): every
// weight is >= 1, so D strictly decreases along the minimising neighbours and they end in S.
//
// The working raster is D itself, uint64 per cell, an upper bound that only ever is the weight
// of a real path.  The phases are those of hdem_flats.hip:
//   classify  (cost_classify_kernel)  per tile: costs validated, barriers, invalid costs and
//             sources counted, D = 0 / infinite, the tiles that hold a source listed for round 0.
//             Unlike the flats, a tile without a source has nothing to do until a neighbour's
//             frame changes: tiles become active as the front arrives.  A source on a tile's
//             frame is such a change, made here: the tile stamps round 0, so that its
//             neighbours run in round 1 whether or not its own visit moves the frame.
//   relax     (cost_relax_kernel)  one workgroup per listed tile: q and D of the tile and its
//             one-cell halo in LDS, then D[c] <- min(D[c], D[n] + w(c, n)) until the tile stops
//             changing.  One iteration is four directional sweeps, one wave each, all four at
//             once, 64 steps with the three neighbours of the previous line each; the waves race
//             on the same cells through 64-bit LDS atomic min, so a cell never goes up.  Barriers
//             (q = 0, also outside the raster) are never relaxed and never offered.  The tile is
//             written back where it changed; if a frame cell changed, the tile stamps the round.
//   schedule  (cost_schedule_kernel)  between rounds: a tile runs again when one of its eight
//             neighbours stamped the last round.  The host reads the length of the list (one
//             word per round) and launches that many workgroups; an empty list ends it.
//   final     (cost_final_kernel)  streaming: back link, units and distance of every cell, ties,
//             cells out of reach and the largest D counted, the limit applied -- and the local
//             equation above checked at every non-barrier cell, so the result is certified, not
//             assumed: a violation is HDEM_ERR_NOT_CONVERGED.
//   trace     only when nearest or label is wanted: hdem_flowtrace_u8_dev over the back links
//             with S as its streams, then cost_nearest_kernel turns its stop into nearest and
//             label and blanks the cells out of reach.
// q is worked out from cost again on every visit, not kept: a 4-byte q raster would be read in
// place of the 4-byte cost, the same traffic, and cost 4 B per cell of arena and one more
// streaming write; the conversion is four instructions on 17 cells per thread and visit.
// Schedule freedom: every value a cell ever holds is the weight of a real path, the halo a tile
// reads is what a neighbour wrote in some earlier or the same round (whole 64-bit words), and a
// neighbour that lowers a frame cell afterwards stamps its round, which puts the tile on the
// next list.  So stale reads only cost rounds, no workgroup waits for another, and there are no
// fences.  Bounds: an iteration that changes the tile makes at least one more cell final
// (Bellman-Ford from fixed halo values), so at most 4096 iterations; a round that changes
// anything makes final every cell whose least path crosses one more tile seam, so at most H * W
// rounds.
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per workgroup, every kernel here
constexpr int LH = TS + 2;            // LDS rows: the tile and its halo
constexpr int LW = TS + 3;            // LDS row pitch, odd.  A column sweep has one lane per row:
                                      // D (8 B, read as one b64, bank (a/4) % 64, 32 lanes a
                                      // pass) starts at dword 2 * 67 * l = 6 l (mod 64), 32
                                      // different even banks and their odd successors; q (4 B,
                                      // bank (a/4) % 32) at 67 l = 3 l (mod 32), 32 different
                                      // banks.  Two conflict-free passes each.
constexpr uint64_t INF = ~0ull;
constexpr uint32_t Q_MAX = (1u << 28) - 1;
constexpr uint32_t Q_BAD = 0xFFFFFFFFu;   // a cost out of range
constexpr uint64_t SQRT2_Q31 = 3037000500ull;   // round(sqrt(2) * 2^31)

struct cost_counters {
    unsigned long long sources;       // non-barrier cells of S
    unsigned long long barriers;
    unsigned long long bad;           // costs out of range
    unsigned long long unreached;
    unsigned long long ties;
    unsigned long long violations;    // non-barrier cells at which the local equation fails
    unsigned long long max_units;
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
};

// D8 window order (oracle/hdem_oracle_np.py D8_OFFSETS / D8_CODES): the ESRI bit of window
// position j, 4 bits each
__device__ __forceinline__ int window_bit(int j) { return (0x12304765u >> (4 * j)) & 7; }

__device__ __forceinline__ bool in_set(const void *src, int kind, uint32_t threshold, size_t at)
{
    if (kind == HDEM_FT_STREAMS_MASK_U8) return static_cast<const uint8_t *>(src)[at] != 0;
    const uint32_t v = static_cast<const uint32_t *>(src)[at];
    return kind == HDEM_FT_STREAMS_ACC_U32 ? v >= threshold : v != 0;
}

// 0: a barrier; Q_BAD: out of range; else q
__device__ __forceinline__ uint32_t quantise(float c, double scale)
{
    if (c != c) return 0;
    const double v = rint((double)c * scale);
    return c >= 0.f && v >= 1.0 && v <= (double)Q_MAX ? (uint32_t)v : Q_BAD;
}

__device__ __forceinline__ uint64_t step_weight(uint32_t qa, uint32_t qb, bool diagonal)
{
    const uint64_t s = (uint64_t)qa + qb;
    return diagonal ? (s * SQRT2_Q31 + (1ull << 30)) >> 31 : s;
}

// a tile reads its halo while the neighbour writes it: whole words
__device__ __forceinline__ uint64_t work_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void work_store(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t lds_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(NT) void cost_classify_kernel(
    const float *__restrict__ cost, const void *__restrict__ sources, int kind,
    uint32_t threshold, double scale, int H, int W, int tiles_x, uint64_t *__restrict__ work,
    uint32_t *__restrict__ stamp, uint32_t *__restrict__ list, cost_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[4];            // sources, barriers, costs out of range, and
                                                 // whether a source lies on the frame
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int src = 0, barrier = 0, bad = 0, edge = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        const uint32_t q = quantise(cost[g], scale);
        const bool s = q != 0 && in_set(sources, kind, threshold, g);
        barrier += q == 0;
        bad += q == Q_BAD;
        src += s;
        edge |= s && (ly == 0 || ly == TS - 1 || lx == 0 || lx == TS - 1);
        work[g] = s ? 0ull : INF;
    }
    if (src) atomicAdd(&s_cnt[0], src);
    if (edge) atomicOr(&s_cnt[3], 1u);
    if (barrier) atomicAdd(&s_cnt[1], barrier);
    if (bad) atomicAdd(&s_cnt[2], bad);
    __syncthreads();
    if (tid == 0) {
        stamp[blockIdx.x] = s_cnt[3];                // 1: what a visit of round 0 would stamp
        if (s_cnt[0]) {
            atomicAdd(&cnt->sources, (unsigned long long)s_cnt[0]);
            list[atomicAdd(&cnt->listed, 1u)] = blockIdx.x;
        }
        if (s_cnt[1]) atomicAdd(&cnt->barriers, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[2]);
    }
}

// The list of round `round` >= 1: the tiles next to a tile whose frame changed in round - 1.
// One thread per tile; the order of the list is whatever the atomics give and changes no result.
__global__ __launch_bounds__(NT) void cost_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ list, cost_counters *__restrict__ cnt)
{
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= (int64_t)tiles_y * tiles_x) return;
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

__global__ __launch_bounds__(NT) void cost_relax_kernel(
    const float *__restrict__ cost, uint64_t *work, double scale, int H, int W, int tiles_x,
    const uint32_t *__restrict__ list, uint32_t round, uint32_t *__restrict__ stamp)
{
    __shared__ uint64_t d[LH * LW];
    __shared__ uint32_t q[LH * LW];
    __shared__ unsigned int s_edge;

    const int tid = threadIdx.x;
    const uint32_t t = list[blockIdx.x];
    const int y0 = (int)(t / tiles_x) * TS, x0 = (int)(t % tiles_x) * TS;
    if (tid == 0) s_edge = 0;

    // the tile and its halo; outside the raster: a barrier
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = (size_t)gy * W + gx;
        q[hy * LW + hx] = in ? quantise(cost[g], scale) : 0u;
        d[hy * LW + hx] = in ? work_load(work + g) : INF;
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
            const uint32_t qc = q[c];
            if (qc) {                                    // a cell of the graph
                const uint64_t dc = lds_load(&d[c]);
                const int p = c - step;
                uint64_t best = dc;
                for (int k = -1; k <= 1; ++k) {
                    const int n = p + k * side;
                    const uint32_t qn = q[n];
                    const uint64_t dn = lds_load(&d[n]);
                    if (!qn || dn == INF) continue;
                    best = min(best, dn + step_weight(qc, qn, k != 0));
                }
                if (best < dc) {
                    atomicMin(reinterpret_cast<unsigned long long *>(&d[c]),
                              (unsigned long long)best);
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
        const uint64_t v = d[(ly + 1) * LW + lx + 1];
        if (v != work[g]) {                              // only this workgroup writes these cells
            work_store(work + g, v);
            edge |= ly == 0 || ly == TS - 1 || lx == 0 || lx == TS - 1;
        }
    }
    if (edge) atomicOr(&s_edge, 1u);
    __syncthreads();
    if (tid == 0 && s_edge) stamp[t] = round + 1;
}

__global__ __launch_bounds__(NT) void cost_final_kernel(
    const float *__restrict__ cost, const void *__restrict__ sources, int kind,
    uint32_t threshold, double scale, double unit, uint64_t limit,
    const uint64_t *__restrict__ work, int H, int W, int tiles_x, int64_t *__restrict__ units,
    float *__restrict__ distance, uint8_t *__restrict__ backlink, cost_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[3];            // out of reach, ties, violations
    __shared__ unsigned long long s_far;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 3) s_cnt[tid] = 0;
    if (tid == 0) s_far = 0;
    __syncthreads();

    unsigned int unreached = 0, ties = 0, violations = 0;
    uint64_t far = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const int gy = tile.y0 + ly, gx = tile.x0 + lx;
        const size_t g = (size_t)gy * W + gx;
        const uint32_t qc = quantise(cost[g], scale);
        const uint64_t D = work[g];
        uint8_t code = 0;
        bool reached = false;
        if (qc) {
            const bool src = in_set(sources, kind, threshold, g);
            uint64_t least = INF;
            int pick = -1, attain = 0;
            for (int j = 0; j < 8; ++j) {
                const int b = window_bit(j);
                const int ny = gy + code_dy(b), nx = gx + code_dx(b);
                if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                const size_t n = (size_t)ny * W + nx;
                const uint32_t qn = quantise(cost[n], scale);
                const uint64_t dn = work[n];
                if (!qn || dn == INF) continue;
                const uint64_t a = dn + step_weight(qc, qn, b & 1);
                least = min(least, a);
                if (a == D) {
                    if (pick < 0) pick = b;
                    ++attain;
                }
            }
            violations += D != (src ? 0ull : least);
            reached = D != INF && (!limit || D <= limit);
            if (reached) {
                far = max(far, D);
                if (!src) {
                    code = pick < 0 ? 0 : (uint8_t)(1u << pick);
                    ties += attain > 1;
                }
            } else {
                ++unreached;
            }
        }
        if (units) units[g] = reached ? (int64_t)D : -1;
        if (distance)
            distance[g] = reached ? (float)((double)D * unit) : __uint_as_float(0x7FC00000u);
        if (backlink) backlink[g] = code;
    }
    if (unreached) atomicAdd(&s_cnt[0], unreached);
    if (ties) atomicAdd(&s_cnt[1], ties);
    if (violations) atomicAdd(&s_cnt[2], violations);
    if (far) atomicMax(&s_far, (unsigned long long)far);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->unreached, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->ties, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->violations, (unsigned long long)s_cnt[2]);
        if (s_far) atomicMax(&cnt->max_units, s_far);
    }
}

// stop (1 + the flat index of the source a cell's back links end in, as the trace wrote it, in
// `nearest` itself when that is wanted) -> nearest and label; out of reach: 0xFFFFFFFF and 0
__global__ __launch_bounds__(NT) void cost_nearest_kernel(
    int64_t cells, const uint64_t *__restrict__ work, uint64_t limit, const uint32_t *stop,
    const uint32_t *__restrict__ sources, uint32_t *nearest, uint32_t *__restrict__ label)
{
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c >= cells) return;
    const uint64_t D = work[c];
    const uint32_t s = stop[c];
    const bool reached = D != INF && (!limit || D <= limit) && s != 0;
    if (nearest) nearest[c] = reached ? s - 1 : 0xFFFFFFFFu;
    if (label) label[c] = reached ? sources[s - 1] : 0u;
}

// What a call is given.
struct cost_call {
    const float *cost;
    int H, W;
    const void *sources;
    int kind;
    uint32_t threshold;
    int frac_bits;
    double cellsize;
    int64_t max_units;
    int64_t *units;
    float *distance;
    uint8_t *backlink;
    uint32_t *nearest, *label;
};

// also the tile grid: nothing is allocated for a raster that is refused
int cost_check(const hdem_ctx *ctx, const cost_call &a, int flags,
               const hdem_costdistance_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.cost && a.sources, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(a.H > 0 && a.W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", a.H, a.W);
    if (int rc = d8_check_stats(stats, "hdem_costdistance_stats")) return rc;
    HDEM_REQUIRE(a.kind != HDEM_FT_STREAMS_NONE, HDEM_ERR_BAD_ARG,
                 "cost distance needs a source set: HDEM_FT_STREAMS_NONE is not a kind here");
    if (a.kind == HDEM_PX_SOURCES_LABELS_U32)
        HDEM_REQUIRE(!a.threshold, HDEM_ERR_BAD_ARG,
                     "a label raster takes no threshold (got %u)", a.threshold);
    else if (int rc = d8_check_streams(a.sources, a.kind, a.threshold))
        return rc;
    HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 16, HDEM_ERR_BAD_ARG,
                 "frac_bits is 0 ... 16, got %d", a.frac_bits);
    HDEM_REQUIRE(a.max_units >= 0, HDEM_ERR_BAD_ARG,
                 "max_units is >= 0 (0: no limit), got %lld", (long long)a.max_units);
    HDEM_REQUIRE(a.units || a.distance || a.backlink || a.nearest || a.label, HDEM_ERR_BAD_ARG,
                 "cost distance: no output wanted");
    HDEM_REQUIRE(!a.label || a.kind == HDEM_PX_SOURCES_LABELS_U32, HDEM_ERR_BAD_ARG,
                 "label needs label sources (HDEM_PX_SOURCES_LABELS_U32)");
    HDEM_REQUIRE(!a.distance || (std::isfinite(a.cellsize) && a.cellsize > 0.0),
                 HDEM_ERR_BAD_ARG, "cellsize must be finite and positive, got %g", a.cellsize);
    HDEM_REQUIRE(!(flags & ~HDEM_ON_DEVICE), HDEM_ERR_BAD_ARG,
                 "cost distance: unknown flags 0x%x", flags);
    if (int rc = d8_grid_of("cost distance", a.H, a.W, g)) return rc;

    // inputs first; an output overlaps neither an input nor an earlier output
    const uintptr_t n = (uintptr_t)a.H * a.W;
    const struct { const char *name; uintptr_t at, bytes; } r[] = {
        {"cost", (uintptr_t)a.cost, n * 4},
        {"sources", (uintptr_t)a.sources, a.kind == HDEM_FT_STREAMS_MASK_U8 ? n : n * 4},
        {"units", (uintptr_t)a.units, n * 8},
        {"distance", (uintptr_t)a.distance, n * 4},
        {"backlink", (uintptr_t)a.backlink, n},
        {"nearest", (uintptr_t)a.nearest, n * 4},
        {"label", (uintptr_t)a.label, n * 4},
    };
    for (int i = 2; i < 7; ++i)
        for (int j = 0; r[i].at && j < i; ++j)
            HDEM_REQUIRE(!r[j].at || r[i].at + r[i].bytes <= r[j].at ||
                             r[j].at + r[j].bytes <= r[i].at,
                         HDEM_ERR_BAD_ARG, "cost distance: %s overlaps %s", r[i].name, r[j].name);
    return HDEM_OK;
}

// The operator on device pointers, after cost_check.  *st is filled when the launches ran,
// whatever is returned; the caller publishes it.
int cost_dev(hdem_ctx *ctx, const cost_call &a, const d8_grid &g, bool want_stats,
             hdem_costdistance_stats *st)
{
    const int H = a.H, W = a.W, tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;
    const bool trace = a.nearest || a.label;

    // arena: the flow trace's bytes (when it runs) | counters | stamp, list: u32 per tile each |
    // the working raster, u64 per cell | for the trace: the codes, u8 per cell, and its stop,
    // u32 per cell, where the caller's backlink and nearest do not hold them
    const size_t trace_bytes =
        trace ? hdem_round16(hdem_flowtrace_arena_bytes(g.tiles, g.nslots)) : 0;
    const size_t head = 512;
    static_assert(sizeof(cost_counters) <= head, "counters outgrew their block");
    const size_t per_tile = hdem_round16((size_t)tiles * 8);
    const size_t code_bytes = trace && !a.backlink ? hdem_round16((size_t)cells) : 0;
    const size_t stop_bytes = trace && !a.nearest ? (size_t)cells * 4 : 0;
    char *ws = static_cast<char *>(hdem_arena(
        ctx, trace_bytes + head + per_tile + (size_t)cells * 8 + code_bytes + stop_bytes));
    if (!ws) return HDEM_ERR_OOM;
    ws += trace_bytes;
    cost_counters *cnt = reinterpret_cast<cost_counters *>(ws);
    uint32_t *stamp = reinterpret_cast<uint32_t *>(ws + head), *list = stamp + tiles;
    uint64_t *work = reinterpret_cast<uint64_t *>(ws + head + per_tile);
    char *behind = reinterpret_cast<char *>(work + cells);
    uint8_t *codes = a.backlink ? a.backlink : reinterpret_cast<uint8_t *>(behind);
    uint32_t *stop = a.nearest ? a.nearest : reinterpret_cast<uint32_t *>(behind + code_bytes);

    const double scale = std::ldexp(1.0, a.frac_bits);
    const double unit = a.distance ? std::ldexp(a.cellsize, -(a.frac_bits + 1)) : 0.0;
    const uint64_t limit = (uint64_t)a.max_units;

    hdem_event_timer<5> phases(ctx, want_stats);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(cost_counters), ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    hipLaunchKernelGGL(cost_classify_kernel, grid, dim3(NT), 0, ctx->stream, a.cost, a.sources,
                       a.kind, a.threshold, scale, H, W, tiles_x, work, stamp, list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    cost_counters host = {};
    int64_t rounds = 0, visits = 0;
    for (;; ++rounds) {
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
        HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (host.bad || !host.listed || rounds > cells) break;
        visits += host.listed;
        hipLaunchKernelGGL(cost_relax_kernel, dim3(host.listed), dim3(NT), 0, ctx->stream, a.cost,
                           work, scale, H, W, tiles_x, list, (uint32_t)rounds, stamp);
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(cost_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           stamp, list, cnt);
    }
    phases.mark(2);
    if (!host.bad) {
        hipLaunchKernelGGL(cost_final_kernel, grid, dim3(NT), 0, ctx->stream, a.cost, a.sources,
                           a.kind, a.threshold, scale, unit, limit, work, H, W, tiles_x, a.units,
                           a.distance, trace ? codes : a.backlink, cnt);
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
    st->tile_visits = visits;
    st->sources = (int64_t)host.sources;
    st->barriers = (int64_t)host.barriers;
    st->unreached = (int64_t)host.unreached;
    st->tie_cells = (int64_t)host.ties;
    st->invalid = (int64_t)host.bad;
    st->max_units = (int64_t)host.max_units;
    st->tile_h = TS;
    st->tile_w = TS;
    HDEM_REQUIRE(!host.bad, HDEM_ERR_BAD_ARG,
                 "cost out of range in %llu cells: a cost is NaN (a barrier) or finite with "
                 "1 <= rint(cost * 2^frac_bits) <= 2^28 - 1",
                 host.bad);
    HDEM_REQUIRE(!host.listed && !host.violations, HDEM_ERR_NOT_CONVERGED,
                 "cost distance is not certified after %lld rounds: the distance of %llu cells "
                 "is not the least of their neighbours' plus the step",
                 (long long)rounds, host.violations);
    if (trace) {
        // the source every back-link path ends in; the trace takes the head of the arena,
        // synchronises, and finds nothing to refuse in codes that strictly decrease D
        const bool labels = a.kind == HDEM_PX_SOURCES_LABELS_U32;
        if (int rc = hdem_flowtrace_u8_dev(
                ctx, codes, H, W, a.sources, labels ? HDEM_FT_STREAMS_ACC_U32 : a.kind,
                labels ? 1u : a.threshold, nullptr, 1.0, stop, nullptr, nullptr, nullptr, nullptr,
                0, nullptr))
            return rc;
        hipLaunchKernelGGL(cost_nearest_kernel, dim3((unsigned)((cells + NT - 1) / NT)), dim3(NT),
                           0, ctx->stream, cells, work, limit, stop,
                           static_cast<const uint32_t *>(a.sources), a.nearest, a.label);
        HDEM_HIP_CHECK(hipGetLastError());
    }
    phases.mark(4);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    phases.read(&st->ms_classify, &st->ms_relax, &st->ms_final);
    if (trace) st->ms_trace = phases.ms(3, 4);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: one symbol; HDEM_ON_DEVICE in flags says the pointers are device pointers
// ---------------------------------------------------------------------------
extern "C" int hdem_costdistance_f32(hdem_ctx *ctx, const float *cost, int H, int W,
                                     const void *sources, int source_kind, uint32_t threshold,
                                     int frac_bits, double cellsize, int64_t max_units,
                                     int64_t *units, float *distance, uint8_t *backlink,
                                     uint32_t *nearest, uint32_t *label, int flags,
                                     hdem_costdistance_stats *stats)
{
    cost_call a = {cost, H, W, sources, source_kind, threshold, frac_bits, cellsize, max_units,
                   units, distance, backlink, nearest, label};
    d8_grid g;
    if (int rc = cost_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_costdistance_stats st = {};
    d8_publish(stats, st);

    const size_t n = (size_t)H * W;
    hdem_dbuf dcost, dsources, dunits, ddistance, dbacklink, dnearest, dlabel;
    if (!(flags & HDEM_ON_DEVICE)) {
        if (int rc = dcost.upload(ctx, cost, n * 4)) return rc;
        if (int rc = dsources.upload(ctx, sources,
                                     source_kind == HDEM_FT_STREAMS_MASK_U8 ? n : n * 4))
            return rc;
        if (units)
            if (int rc = dunits.alloc(ctx, n * 8)) return rc;
        if (distance)
            if (int rc = ddistance.alloc(ctx, n * 4)) return rc;
        if (backlink)
            if (int rc = dbacklink.alloc(ctx, n)) return rc;
        if (nearest)
            if (int rc = dnearest.alloc(ctx, n * 4)) return rc;
        if (label)
            if (int rc = dlabel.alloc(ctx, n * 4)) return rc;
        a.cost = dcost.as<const float>(), a.sources = dsources.p;
        a.units = dunits.as<int64_t>(), a.distance = ddistance.as<float>();
        a.backlink = dbacklink.as<uint8_t>();
        a.nearest = dnearest.as<uint32_t>(), a.label = dlabel.as<uint32_t>();
    }
    const int rc = cost_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, st);
    if (rc || (flags & HDEM_ON_DEVICE)) return rc;
    if (units)
        if (int rc2 = dunits.download(units, n * 8)) return rc2;
    if (distance)
        if (int rc2 = ddistance.download(distance, n * 4)) return rc2;
    if (backlink)
        if (int rc2 = dbacklink.download(backlink, n)) return rc2;
    if (nearest)
        if (int rc2 = dnearest.download(nearest, n * 4)) return rc2;
    return label ? dlabel.download(label, n * 4) : HDEM_OK;
}
