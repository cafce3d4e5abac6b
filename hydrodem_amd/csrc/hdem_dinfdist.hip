// A26  D-infinity distance down: horizontal, vertical or surface distance along the D-infinity
// paths to a stop set, as average, minimum or maximum over the flow proportions (TauDEM's
// dinfdistdown; new operator; include/hydrodem_hip.h has the contract, DESIGN 3.27 the argument).
//
// The word of a cell is hdem_dinf.hip's: q in bits 0-15, the facet in bits 16-19, directions
// counted counter-clockwise from east.  The decode below is this file's own short copy:
// hdem_dinf.hip is left as it is.
//
// The distance is a pull over RECEIVERS on the DAG that A21 pulls over donors, in A21's structure:
//   classify  (dinfdist_classify_kernel)  per tile: words validated and counted as A21 counts
//             them, the working raster (uint64 per cell: the bits of the float64 D, or the one
//             reserved NaN pattern NOT_FINAL) set -- a stop cell to 0, a cell with facet 0
//             outside the stop set to NaN, every other cell to NOT_FINAL -- and every tile listed
//             for round 0.  It writes every word that is read later.
//   visit     (dinfdist_visit_kernel)  one workgroup per listed tile: words, values and, for the
//             vertical and surface kinds, elevations of the tile and its one-cell halo in LDS; a
//             cell that is not final and whose receivers with a share are all final becomes final
//             with the value the contract gives, until the tile stops changing.  One iteration is
//             four directional sweeps, one wave each, as in A21; the waves do not wait for each
//             other inside an iteration: a cell only ever goes from NOT_FINAL to one final value,
//             the value is one 64-bit LDS word, and two waves that finalise the same cell store
//             the same word.  Halo cells are read-only.  The cells that became final are written
//             back; if one of them is on the tile's frame the tile stamps the round.  No donor
//             mask: a cell finds its receivers in its own word.
//   schedule  (dinfdist_schedule_kernel)  a tile that still has cells to finalise runs again
//             when one of its eight neighbours stamped the round just run.  The host reads the
//             length of the list, one word per round; an empty list ends the loop.
//   final     (dinfdist_final_kernel)  streaming: (float)D written, the NaN results and the
//             cells that never became final counted: any of the latter is a cycle.
// Schedule freedom: the final word of a cell is a function of its receivers' final words alone
// -- float64 operations in a fixed order, every NaN canonicalised -- so a cell has one possible
// final word whoever computes it and whenever.  NOT_FINAL is a NaN pattern that no store of a
// result can produce.  A halo word is read with one relaxed 64-bit load: it is NOT_FINAL or the
// final word, never half of each; a stale NOT_FINAL costs a round, because the neighbour that
// finalises the cell afterwards stamps its round and that puts this tile on the next list.
// Visibility between tiles comes from the kernel boundaries alone (the per-XCD L2s are not
// coherent inside a launch): no fences, and no workgroup waits for another.  Bounds: an
// iteration that changes the tile makes at least one cell final, so at most 4096 of them; a
// round with a non-empty list follows a round that made a frame cell final, so at most
// H * W + 1 rounds.
#include "hdem_d8tile.h"
#include "hdem_stencil_tile.h"

#include <cmath>

namespace {

constexpr uint32_t Q_ONE = 32768;                        // q of "everything to the diagonal"
constexpr uint64_t QNAN = 0x7FF8000000000000ull;         // the one NaN a result is stored as
constexpr uint64_t NOT_FINAL = 0x7FF8000000000001ull;    // never the bits of a stored result
constexpr int LH = TS + 2;                    // LDS rows: the tile and its halo
constexpr int LW = TS + 3;                    // LDS row pitch: odd (hdem_dinf.hip)

// direction d -> (dy, dx), packed (d + 1) in 4 bits per entry
__device__ __forceinline__ int dir_dy(int d) { return ((0x22210001u >> (4 * d)) & 3) - 1; }
__device__ __forceinline__ int dir_dx(int d) { return ((0x21000122u >> (4 * d)) & 3) - 1; }
__device__ __forceinline__ int facet_card(uint32_t f) { return 2 * ((f >> 1) & 3); }
__device__ __forceinline__ int facet_diag(uint32_t f) { return 2 * ((f - 1) >> 1) + 1; }

__device__ __forceinline__ bool word_valid(uint32_t w)
{
    const uint32_t f = (w >> 16) & 15, q = w & 0xFFFFu;
    return (w >> 20) == 0 && f <= 8 && q <= Q_ONE && (f != 0 || q == 0);
}

struct dinfdist_counters {
    unsigned long long split;         // cells with two receivers
    unsigned long long terminal;      // cells with facet 0
    unsigned long long stop;          // cells of the stop set
    unsigned long long bad;           // invalid words
    unsigned long long outside;       // cells with a receiver outside the raster
    unsigned long long unreached;     // NaN results
    unsigned long long unresolved;    // cells that never became final
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
};

// the horizontal step by direction: dx for E / W, dy for N / S, the diagonal; and their squares
struct dinfdist_steps {
    double dx, dy, diag;
    double dx2, dy2, diag2;
};

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
__device__ __forceinline__ void lds_store(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(NT) void dinfdist_classify_kernel(
    const uint32_t *__restrict__ words, const void *__restrict__ streams, int stream_kind,
    uint32_t threshold, int H, int W, int tiles_x, uint64_t *__restrict__ work,
    uint32_t *__restrict__ left, uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    dinfdist_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_cnt[6];            // split, terminal, stop, bad, outside, pending
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();

    unsigned int n[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const int gy = tile.y0 + ly, gx = tile.x0 + lx;
        const size_t g = (size_t)gy * W + gx;
        const uint32_t w = words[g];
        const bool valid = word_valid(w);
        const uint32_t f = w >> 16, q = w & 0xFFFFu;
        if (!valid) {
            ++n[3];
        } else {
            n[0] += q != 0 && q != Q_ONE;
            n[1] += f == 0;
            bool out = false;
            if (f && q != Q_ONE) {
                const int d = facet_card(f), ny = gy + dir_dy(d), nx = gx + dir_dx(d);
                out |= ny < 0 || ny >= H || nx < 0 || nx >= W;
            }
            if (f && q != 0) {
                const int d = facet_diag(f), ny = gy + dir_dy(d), nx = gx + dir_dx(d);
                out |= ny < 0 || ny >= H || nx < 0 || nx >= W;
            }
            n[4] += out;
        }
        bool stop;
        if (stream_kind == HDEM_FT_STREAMS_MASK_U8)
            stop = static_cast<const uint8_t *>(streams)[g] != 0;
        else if (stream_kind == HDEM_FT_STREAMS_ACC_U32)
            stop = static_cast<const uint32_t *>(streams)[g] >= threshold;
        else
            stop = valid && f == 0;
        n[2] += stop;
        const uint64_t init = stop ? 0ull : (valid && f == 0) ? QNAN : NOT_FINAL;
        n[5] += init == NOT_FINAL;
        work[g] = init;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (n[j]) atomicAdd(&s_cnt[j], n[j]);
    __syncthreads();
    if (tid == 0) {
        left[blockIdx.x] = s_cnt[5];
        stamp[blockIdx.x] = 0;
        list[atomicAdd(&cnt->listed, 1u)] = blockIdx.x;
        if (s_cnt[0]) atomicAdd(&cnt->split, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->terminal, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->stop, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[3]);
        if (s_cnt[4]) atomicAdd(&cnt->outside, (unsigned long long)s_cnt[4]);
    }
}

// The list of round `round` >= 1: the tiles with cells left next to a tile that made a frame
// cell final in round - 1.  One thread per tile; the order of the list changes no result.
__global__ __launch_bounds__(NT) void dinfdist_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ left,
    const uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    dinfdist_counters *__restrict__ cnt)
{
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= (int64_t)tiles_y * tiles_x || !left[t]) return;
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

// a = s + D[r] for the receiver of LDS cell c in direction d; false while r is not final
template <int KIND>
__device__ __forceinline__ bool dinfdist_arrive(const uint64_t *v, const float *z, int c, int d,
                                                const dinfdist_steps &s, double *a)
{
    const int n = c + dir_dy(d) * LW + dir_dx(d);
    const uint64_t vn = lds_load(&v[n]);
    if (vn == NOT_FINAL) return false;
    const double down = __longlong_as_double((long long)vn);
    double cost;
    if (KIND == HDEM_DD_HORIZONTAL) {
        cost = (d & 1) ? s.diag : (d & 2) ? s.dy : s.dx;
    } else {
        const double drop = (double)z[c] - (double)z[n];
        if (KIND == HDEM_DD_VERTICAL) {
            cost = drop;
        } else {
            const double h2 = (d & 1) ? s.diag2 : (d & 2) ? s.dy2 : s.dx2;
            cost = sqrt(h2 + drop * drop);
        }
    }
    *a = cost + down;
    return true;
}

// D of a cell with two receivers, shares 32768 - q and q
__device__ __forceinline__ double dinfdist_combine(int statistic, uint32_t q, double a1, double a2)
{
    if (statistic == HDEM_DD_AVERAGE)
        return ((double)(Q_ONE - q) * a1 + (double)q * a2) * 0x1p-15;
    const bool n1 = a1 != a1, n2 = a2 != a2;
    if (statistic == HDEM_DD_MAXIMUM)
        return (n1 || n2) ? __longlong_as_double((long long)QNAN) : a2 > a1 ? a2 : a1;
    return n1 ? a2 : n2 ? a1 : a2 < a1 ? a2 : a1;
}

// KIND: HDEM_DD_*; the horizontal form holds no elevations
template <int KIND>
__global__ __launch_bounds__(NT) void dinfdist_visit_kernel(
    const uint32_t *__restrict__ words, const float *__restrict__ dem, uint64_t *work, int H,
    int W, int tiles_x, const uint32_t *__restrict__ list, uint32_t round,
    const dinfdist_steps steps, int statistic, uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ left)
{
    __shared__ uint64_t v[LH * LW];              // the bits of D, or NOT_FINAL
    __shared__ uint32_t w[LH * LW];              // the word
    __shared__ float z[KIND == HDEM_DD_HORIZONTAL ? 1 : LH * LW];
    __shared__ unsigned int s_edge, s_left;

    const int tid = threadIdx.x;
    const uint32_t t = list[blockIdx.x];
    if (!left[t]) return;                        // round 0 lists every tile
    const int y0 = (int)(t / tiles_x) * TS, x0 = (int)(t % tiles_x) * TS;
    if (tid == 0) s_edge = 0, s_left = 0;

    // the tile and its halo; outside the raster: final, and no cell's receiver
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = (size_t)gy * W + gx;
        w[hy * LW + hx] = in ? words[g] : 0u;
        if (KIND != HDEM_DD_HORIZONTAL) z[hy * LW + hx] = in ? dem[g] : 0.0f;
        lds_store(&v[hy * LW + hx], in ? work_load(work + g) : QNAN);
    }
    __syncthreads();

    // which of the thread's 16 cells are not final yet: the ones it may have to write back
    uint32_t pending = 0;
#pragma unroll
    for (int k = 0; k < TC / NT; ++k) {
        const int i = tid + k * NT;
        if (lds_load(&v[(i / TS + 1) * LW + i % TS + 1]) == NOT_FINAL) pending |= 1u << k;
    }

    // wave 0 sweeps down the rows, 1 up, 2 along the columns to the right, 3 to the left; the
    // lane is the position in the line.  c0: the cell of step 0, step: to the next line.
    const int wave = tid >> 6, lane = tid & 63;
    const int step = wave == 0 ? LW : wave == 1 ? -LW : wave == 2 ? 1 : -1;
    const int c0 = wave == 0   ? LW + lane + 1
                   : wave == 1 ? TS * LW + lane + 1
                   : wave == 2 ? (lane + 1) * LW + 1
                               : (lane + 1) * LW + TS;
    bool any = false;
    for (int iter = 0; iter < TC; ++iter) {
        int changed = 0;
        for (int s = 0, c = c0; s < TS; ++s, c += step) {
            if (lds_load(&v[c]) != NOT_FINAL) continue;
            const uint32_t f = w[c] >> 16, q = w[c] & 0xFFFFu;   // valid, and f is 1 ... 8
            double a1 = 0.0, a2 = 0.0;
            if (q != Q_ONE && !dinfdist_arrive<KIND>(v, z, c, facet_card(f), steps, &a1)) continue;
            if (q != 0 && !dinfdist_arrive<KIND>(v, z, c, facet_diag(f), steps, &a2)) continue;
            const double D = q == 0       ? a1
                             : q == Q_ONE ? a2
                                          : dinfdist_combine(statistic, q, a1, a2);
            lds_store(&v[c], D != D ? QNAN : (uint64_t)__double_as_longlong(D));
            changed = 1;
        }
        if (!__syncthreads_or(changed)) break;
        any = true;
    }
    if (!any) return;

    unsigned int edge = 0, still = 0;
#pragma unroll
    for (int k = 0; k < TC / NT; ++k) {
        if (!((pending >> k) & 1)) continue;
        const int i = tid + k * NT;
        const int ly = i / TS, lx = i % TS;
        const uint64_t vc = lds_load(&v[(ly + 1) * LW + lx + 1]);
        if (vc != NOT_FINAL) {                           // only this workgroup writes these cells
            work_store(work + (size_t)(y0 + ly) * W + x0 + lx, vc);
            edge |= ly == 0 || ly == TS - 1 || lx == 0 || lx == TS - 1;
        } else {
            ++still;
        }
    }
    if (edge) atomicOr(&s_edge, 1u);
    if (still) atomicAdd(&s_left, still);
    __syncthreads();
    if (tid == 0) {
        left[t] = s_left;
        if (s_edge) stamp[t] = round + 1;
    }
}

__global__ __launch_bounds__(NT) void dinfdist_final_kernel(
    const uint64_t *__restrict__ work, int H, int W, int tiles_x, float *__restrict__ distance,
    dinfdist_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_unreached, s_unresolved;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid == 0) s_unreached = 0, s_unresolved = 0;
    __syncthreads();

    unsigned int unreached = 0, unresolved = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        const uint64_t vc = work[g];
        const double D = __longlong_as_double((long long)vc);
        unresolved += vc == NOT_FINAL;
        unreached += vc == QNAN;
        distance[g] = D != D ? __uint_as_float(0x7FC00000u) : (float)D;
    }
    if (unreached) atomicAdd(&s_unreached, unreached);
    if (unresolved) atomicAdd(&s_unresolved, unresolved);
    __syncthreads();
    if (tid == 0) {
        if (s_unreached) atomicAdd(&cnt->unreached, (unsigned long long)s_unreached);
        if (s_unresolved) atomicAdd(&cnt->unresolved, (unsigned long long)s_unresolved);
    }
}

// What a call is given.
struct dinfdist_call {
    const uint32_t *words;
    int H, W;
    const void *streams;
    int stream_kind;
    uint32_t threshold;
    const float *dem;
    double dx, dy;
    int kind, statistic;
    float *distance;
};

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

inline size_t stream_bytes(int stream_kind)
{
    return stream_kind == HDEM_FT_STREAMS_MASK_U8 ? 1 : 4;
}

// also the tile grid: nothing is allocated for a raster that is refused
int dinfdist_check(const hdem_ctx *ctx, const dinfdist_call &a, int flags,
                   const hdem_dinfdist_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.words && a.distance, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(a.H > 0 && a.W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", a.H, a.W);
    if (int rc = d8_check_stats(stats, "hdem_dinfdist_stats")) return rc;
    HDEM_REQUIRE(a.kind >= HDEM_DD_HORIZONTAL && a.kind <= HDEM_DD_SURFACE, HDEM_ERR_BAD_ARG,
                 "unknown distance kind %d", a.kind);
    HDEM_REQUIRE(a.statistic >= HDEM_DD_AVERAGE && a.statistic <= HDEM_DD_MAXIMUM,
                 HDEM_ERR_BAD_ARG, "unknown distance statistic %d", a.statistic);
    if (int rc = d8_check_streams(a.streams, a.stream_kind, a.threshold)) return rc;
    if (a.kind == HDEM_DD_HORIZONTAL)
        HDEM_REQUIRE(!a.dem, HDEM_ERR_BAD_ARG, "the horizontal distance takes no dem");
    else
        HDEM_REQUIRE(a.dem, HDEM_ERR_BAD_ARG,
                     "the vertical and surface distances need the dem they are measured on");
    HDEM_REQUIRE(positive(a.dx) && positive(a.dy), HDEM_ERR_BAD_ARG,
                 "dx and dy must be finite and positive, got %g and %g", a.dx, a.dy);
    HDEM_REQUIRE(!(flags & ~HDEM_ON_DEVICE), HDEM_ERR_BAD_ARG,
                 "D-infinity distance down: unknown flags 0x%x", flags);
    return d8_grid_of("D-infinity distance down", a.H, a.W, g);
}

// The distance on device pointers, after dinfdist_check.  *st is filled when the launches ran,
// whatever is returned; the caller publishes it.
int dinfdist_dev(hdem_ctx *ctx, const dinfdist_call &a, const d8_grid &g, bool want_stats,
                 hdem_dinfdist_stats *st)
{
    const int H = a.H, W = a.W, tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;

    // arena: counters | left, stamp, list: u32 per tile each | the working raster, u64 per cell
    const size_t head = 512;
    static_assert(sizeof(dinfdist_counters) <= head, "counters outgrew their block");
    const size_t per_tile = hdem_round16((size_t)tiles * 12);
    char *ws = static_cast<char *>(hdem_arena(ctx, head + per_tile + (size_t)cells * 8));
    if (!ws) return HDEM_ERR_OOM;
    dinfdist_counters *cnt = reinterpret_cast<dinfdist_counters *>(ws);
    uint32_t *left = reinterpret_cast<uint32_t *>(ws + head);
    uint32_t *stamp = left + tiles, *list = stamp + tiles;
    uint64_t *work = reinterpret_cast<uint64_t *>(ws + head + per_tile);

    dinfdist_steps steps;
    steps.dx = a.dx, steps.dy = a.dy, steps.diag = std::sqrt(a.dx * a.dx + a.dy * a.dy);
    steps.dx2 = steps.dx * steps.dx, steps.dy2 = steps.dy * steps.dy;
    steps.diag2 = steps.diag * steps.diag;

    hdem_event_timer<4> phases(ctx, want_stats);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(dinfdist_counters), ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    hipLaunchKernelGGL(dinfdist_classify_kernel, grid, dim3(NT), 0, ctx->stream, a.words,
                       a.streams, a.stream_kind, a.threshold, H, W, tiles_x, work, left, stamp,
                       list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    dinfdist_counters host = {};
    int64_t rounds = 0, visits = 0;
    bool refused = false;
    for (;; ++rounds) {
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
        HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        refused = host.bad || host.outside;
        if (refused || !host.listed || rounds > cells) break;
        visits += host.listed;
#define HDEM_DINFDIST_VISIT(KIND)                                                                 \
    hipLaunchKernelGGL(dinfdist_visit_kernel<KIND>, dim3(host.listed), dim3(NT), 0, ctx->stream,  \
                       a.words, a.dem, work, H, W, tiles_x, list, (uint32_t)rounds, steps,        \
                       a.statistic, stamp, left)
        if (a.kind == HDEM_DD_HORIZONTAL) HDEM_DINFDIST_VISIT(HDEM_DD_HORIZONTAL);
        else if (a.kind == HDEM_DD_VERTICAL) HDEM_DINFDIST_VISIT(HDEM_DD_VERTICAL);
        else HDEM_DINFDIST_VISIT(HDEM_DD_SURFACE);
#undef HDEM_DINFDIST_VISIT
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(dinfdist_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           left, stamp, list, cnt);
    }
    phases.mark(2);
    if (!refused) {
        hipLaunchKernelGGL(dinfdist_final_kernel, grid, dim3(NT), 0, ctx->stream, work, H, W,
                           tiles_x, a.distance, cnt);
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
    st->tile_visits = visits;
    st->split_cells = (int64_t)host.split;
    st->terminal_cells = (int64_t)host.terminal;
    st->stop_cells = (int64_t)host.stop;
    st->unreached_cells = (int64_t)host.unreached;
    st->invalid = (int64_t)host.bad;
    st->outside = (int64_t)host.outside;
    st->unresolved = (int64_t)host.unresolved;
    st->tile_h = TS;
    st->tile_w = TS;
    phases.read(&st->ms_classify, &st->ms_relax, &st->ms_final);
    HDEM_REQUIRE(!host.bad, HDEM_ERR_BAD_ARG,
                 "invalid D-infinity word in %llu cells: the facet is 0 ... 8 in bits 16-19, q is "
                 "0 ... 32768 in bits 0-15 (0 with facet 0), every other bit is 0",
                 host.bad);
    HDEM_REQUIRE(!host.outside, HDEM_ERR_BAD_ARG,
                 "D-infinity words send flow outside the raster in %llu cells", host.outside);
    HDEM_REQUIRE(!host.unresolved, HDEM_ERR_BAD_ARG,
                 "D-infinity words form a cycle without a stop cell: %llu cells never resolve",
                 host.unresolved);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: one symbol; HDEM_ON_DEVICE in flags says the pointers are device pointers
// ---------------------------------------------------------------------------
extern "C" int hdem_dinfdist_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W,
                                 const void *streams, int stream_kind, uint32_t threshold,
                                 const float *dem, double dx, double dy, int kind, int statistic,
                                 float *distance, int flags, hdem_dinfdist_stats *stats)
{
    dinfdist_call a = {words, H, W, streams, stream_kind, threshold, dem, dx, dy, kind, statistic,
                       distance};
    d8_grid g;
    if (int rc = dinfdist_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dinfdist_stats st = {};
    d8_publish(stats, st);

    const size_t n = (size_t)H * W;
    hdem_dbuf dwords, dstreams, ddem, ddistance;
    if (!(flags & HDEM_ON_DEVICE)) {
        if (int rc = dwords.upload(ctx, words, n * 4)) return rc;
        if (int rc = dstreams.upload(ctx, streams, n * stream_bytes(stream_kind))) return rc;
        if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
        if (int rc = ddistance.alloc(ctx, n * 4)) return rc;
        a.words = dwords.as<const uint32_t>(), a.streams = dstreams.p;
        a.dem = ddem.as<const float>(), a.distance = ddistance.as<float>();
    }
    const int rc = dinfdist_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, st);
    if (rc || (flags & HDEM_ON_DEVICE)) return rc;
    return ddistance.download(distance, n * 4);
}
