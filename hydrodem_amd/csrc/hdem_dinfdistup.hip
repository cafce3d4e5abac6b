// A27  D-infinity distance up: horizontal, vertical or surface distance from every cell up its
// D-infinity paths to the ridge, as average, minimum or maximum over the entering flow
// proportions (TauDEM's dinfdistup; new operator; include/hydrodem_hip.h has the contract,
// DESIGN 3.28 the argument).
//
// The word of a cell is hdem_dinf.hip's: q in bits 0-15, the facet in bits 16-19, directions
// counted counter-clockwise from east.  The decode below is this file's own short copy, and the
// skeleton restates hdem_dinfdist.hip's: the shared header is still open.
//
// The distance is a pull over DONORS, A21's dependency, on A26's value representation:
//   classify  (dinfdistup_classify_kernel)  per tile: the words of the tile and its halo in LDS,
//             validated and counted as A21 counts them; the links that enter each cell counted
//             (counted: share >= min_share; ignored: below it), the ridge cells (no counted
//             donor) and the merge cells (more than one); every word of the working raster
//             (uint64 per cell: the bits of the float64 D, or the one reserved NaN pattern
//             NOT_FINAL) written as NOT_FINAL and every tile listed for round 0.
//   visit     (dinfdistup_visit_kernel)  one workgroup per listed tile: words, values and, for
//             the vertical and surface kinds, elevations of the tile and its one-cell halo in LDS.
//             First the mask of each cell's counted donors goes into the top byte of the LDS copy
//             of its word (where A21 keeps its donor mask): the one place where a share meets
//             min_share.  A cell with an empty mask becomes final with 0.  Then a cell that is
//             not final and whose counted donors are all final becomes final with the value the
//             contract gives, until the tile stops changing.  One iteration is four directional
//             sweeps, one wave each, as in A21; the waves do not wait for each other inside an
//             iteration: a cell only ever goes from NOT_FINAL to one final value, the value is
//             one 64-bit LDS word, and two waves that finalise the same cell store the same word.
//             Halo cells are read-only.  The cells that became final are written back; if one of
//             them is on the tile's frame the tile stamps the round.
//   schedule  (dinfdistup_schedule_kernel)  a tile that still has cells to finalise runs again
//             when one of its eight neighbours stamped the round just run.  The host reads the
//             length of the list, one word per round; an empty list ends the loop.
//   final     (dinfdistup_final_kernel)  one workgroup per tile: (float)D written, the NaN
//             results and the cells that never became final counted: any of the latter waits on
//             a cycle of counted links.
// Schedule freedom: the final word of a cell is a function of its counted donors' final words
// alone -- the mask comes from the immutable words and min_share, the donors are taken in the
// order of their position around the cell, the float64 operations are in a fixed order and every
// NaN is canonicalised -- so a cell has one possible final word whoever computes it and whenever.
// NOT_FINAL is a NaN pattern that no store of a result can produce.  A halo word is read with one
// relaxed 64-bit load: it is NOT_FINAL or the final word, never half of each; a stale NOT_FINAL
// costs a round, because the neighbour that finalises the cell afterwards stamps its round and
// that puts this tile on the next list.  Visibility between tiles comes from the kernel
// boundaries alone (the per-XCD L2s are not coherent inside a launch): no fences, and no
// workgroup waits for another.  Bounds: an iteration that changes the tile makes at least one
// cell final, so at most 4096 of them; a round with a non-empty list follows a round that made a
// frame cell final, so at most H * W + 1 rounds.
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

// the share, in units of 2^-15, that the cell of the valid word w sends in direction `to`;
// 0: no link.  Bits 24-31 of w are ignored: the visit keeps a mask there.
__device__ __forceinline__ uint32_t word_share(uint32_t w, int to)
{
    const uint32_t f = (w >> 16) & 15, q = w & 0xFFFFu;
    if (!f) return 0;
    return (to & 1) ? (facet_diag(f) == to ? q : 0u) : (facet_card(f) == to ? Q_ONE - q : 0u);
}

struct dinfdistup_counters {
    unsigned long long ridge;         // cells without a counted donor
    unsigned long long counted;       // links with share >= min_share
    unsigned long long ignored;       // links with share 1 ... min_share - 1
    unsigned long long merge;         // cells with more than one counted donor
    unsigned long long bad;           // invalid words
    unsigned long long outside;       // cells with a receiver outside the raster
    unsigned long long nan;           // NaN results
    unsigned long long unresolved;    // cells that never became final
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
};

// the horizontal step by direction: dx for E / W, dy for N / S, the diagonal; and their squares
struct dinfdistup_steps {
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

__global__ __launch_bounds__(NT) void dinfdistup_classify_kernel(
    const uint32_t *__restrict__ words, uint32_t min_share, int H, int W, int tiles_x,
    uint64_t *__restrict__ work, uint32_t *__restrict__ left, uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ list, dinfdistup_counters *__restrict__ cnt)
{
    __shared__ uint32_t w[LH * LW];              // the words of the tile and its halo
    __shared__ unsigned int s_cnt[6];            // ridge, counted, ignored, merge, bad, outside
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 6) s_cnt[tid] = 0;
    // outside the raster: word 0, no cell's donor
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = tile.y0 + hy - 1, gx = tile.x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        w[hy * LW + hx] = in ? words[(size_t)gy * W + gx] : 0u;
    }
    __syncthreads();

    unsigned int n[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const int gy = tile.y0 + ly, gx = tile.x0 + lx;
        const int c = (ly + 1) * LW + lx + 1;
        const uint32_t wc = w[c];
        if (!word_valid(wc)) {
            ++n[4];
        } else {
            const uint32_t f = wc >> 16, q = wc & 0xFFFFu;
            bool out = false;
            if (f && q != Q_ONE) {
                const int d = facet_card(f), ny = gy + dir_dy(d), nx = gx + dir_dx(d);
                out |= ny < 0 || ny >= H || nx < 0 || nx >= W;
            }
            if (f && q != 0) {
                const int d = facet_diag(f), ny = gy + dir_dy(d), nx = gx + dir_dx(d);
                out |= ny < 0 || ny >= H || nx < 0 || nx >= W;
            }
            n[5] += out;
        }
        // the links that enter the cell; an invalid neighbour is counted above, as itself
        unsigned int counted = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const uint32_t wn = w[c + dir_dy(d) * LW + dir_dx(d)];
            if (!word_valid(wn)) continue;
            const uint32_t p = word_share(wn, (d + 4) & 7);
            counted += p >= min_share;
            n[2] += p != 0 && p < min_share;
        }
        n[0] += counted == 0;
        n[1] += counted;
        n[3] += counted > 1;
        work[(size_t)gy * W + gx] = NOT_FINAL;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (n[j]) atomicAdd(&s_cnt[j], n[j]);
    __syncthreads();
    if (tid == 0) {
        left[blockIdx.x] = (unsigned)(tile.th * tile.tw);
        stamp[blockIdx.x] = 0;
        list[atomicAdd(&cnt->listed, 1u)] = blockIdx.x;
        if (s_cnt[0]) atomicAdd(&cnt->ridge, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->counted, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->ignored, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->merge, (unsigned long long)s_cnt[3]);
        if (s_cnt[4]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[4]);
        if (s_cnt[5]) atomicAdd(&cnt->outside, (unsigned long long)s_cnt[5]);
    }
}

// The list of round `round` >= 1: the tiles with cells left next to a tile that made a frame
// cell final in round - 1.  One thread per tile; the order of the list changes no result.
__global__ __launch_bounds__(NT) void dinfdistup_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ left,
    const uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    dinfdistup_counters *__restrict__ cnt)
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

// the cost of the step from the donor at LDS cell n, position d around LDS cell c, down to c
template <int KIND>
__device__ __forceinline__ double dinfdistup_cost(const float *z, int c, int n, int d,
                                                  const dinfdistup_steps &s)
{
    if (KIND == HDEM_DD_HORIZONTAL) return (d & 1) ? s.diag : (d & 2) ? s.dy : s.dx;
    const double rise = (double)z[n] - (double)z[c];
    if (KIND == HDEM_DD_VERTICAL) return rise;
    const double h2 = (d & 1) ? s.diag2 : (d & 2) ? s.dy2 : s.dx2;
    return sqrt(h2 + rise * rise);
}

// KIND: HDEM_DD_*; the horizontal form holds no elevations
template <int KIND>
__global__ __launch_bounds__(NT) void dinfdistup_visit_kernel(
    const uint32_t *__restrict__ words, const float *__restrict__ dem, uint64_t *work, int H,
    int W, int tiles_x, const uint32_t *__restrict__ list, uint32_t round,
    const dinfdistup_steps steps, int statistic, uint32_t min_share,
    uint32_t *__restrict__ stamp, uint32_t *__restrict__ left)
{
    __shared__ uint64_t v[LH * LW];              // the bits of D, or NOT_FINAL
    __shared__ uint32_t w[LH * LW];              // the word; bits 24-31: the counted donors
    __shared__ float z[KIND == HDEM_DD_HORIZONTAL ? 1 : LH * LW];
    __shared__ unsigned int s_edge, s_left;

    const int tid = threadIdx.x;
    const uint32_t t = list[blockIdx.x];
    if (!left[t]) return;
    const int y0 = (int)(t / tiles_x) * TS, x0 = (int)(t % tiles_x) * TS;
    if (tid == 0) s_edge = 0, s_left = 0;

    // the tile and its halo; outside the raster: final, and no cell's donor
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = (size_t)gy * W + gx;
        w[hy * LW + hx] = in ? words[g] : 0u;
        if (KIND != HDEM_DD_HORIZONTAL) z[hy * LW + hx] = in ? dem[g] : 0.0f;
        lds_store(&v[hy * LW + hx], in ? work_load(work + g) : 0ull);
    }
    __syncthreads();

    // the counted donors of the thread's 16 cells that are not final yet (`pending`: which of
    // them); a cell without one is a ridge cell, final at once.  Only bits 24-31 of a word
    // change here, and the share test reads the bits below: the pass needs no barrier of its own.
    uint32_t pending = 0;
    int changed = 0;
#pragma unroll
    for (int k = 0; k < TC / NT; ++k) {
        const int i = tid + k * NT;
        const int c = (i / TS + 1) * LW + i % TS + 1;
        if (lds_load(&v[c]) != NOT_FINAL) continue;
        pending |= 1u << k;
        uint32_t donors = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (word_share(w[c + dir_dy(d) * LW + dir_dx(d)], (d + 4) & 7) >= min_share)
                donors |= 1u << d;
        w[c] = (w[c] & 0xFFFFFFu) | (donors << 24);
        if (!donors) {
            lds_store(&v[c], 0ull);
            changed = 1;
        }
    }
    bool any = __syncthreads_or(changed);

    // wave 0 sweeps down the rows, 1 up, 2 along the columns to the right, 3 to the left; the
    // lane is the position in the line.  c0: the cell of step 0, step: to the next line.
    const int wave = tid >> 6, lane = tid & 63;
    const int step = wave == 0 ? LW : wave == 1 ? -LW : wave == 2 ? 1 : -1;
    const int c0 = wave == 0   ? LW + lane + 1
                   : wave == 1 ? TS * LW + lane + 1
                   : wave == 2 ? (lane + 1) * LW + 1
                               : (lane + 1) * LW + TS;
    const double qnan = __longlong_as_double((long long)QNAN);
    for (int iter = 0; iter < TC; ++iter) {
        changed = 0;
        for (int s = 0, c = c0; s < TS; ++s, c += step) {
            if (lds_load(&v[c]) != NOT_FINAL) continue;
            uint32_t donors = w[c] >> 24;                    // not empty: the cell is not final
            const bool single = (donors & (donors - 1)) == 0;
            // the donors in the order of their position.  m: a_d of a single donor, the
            // numerator of the average, or the running extreme; den: the shares; first: nothing
            // went into m yet; nan: a NaN a_d was left out of the extreme
            double m = 0.0;
            uint32_t den = 0;
            bool ready = true, first = true, nan = false;
            while (donors) {
                const int d = __builtin_ctz(donors);
                donors &= donors - 1;
                const int n = c + dir_dy(d) * LW + dir_dx(d);
                const uint64_t vn = lds_load(&v[n]);
                if (vn == NOT_FINAL) {
                    ready = false;
                    break;
                }
                const double a = dinfdistup_cost<KIND>(z, c, n, d, steps) +
                                 __longlong_as_double((long long)vn);
                if (single) {
                    m = a;
                } else if (statistic == HDEM_DD_AVERAGE) {
                    const uint32_t p = word_share(w[n], (d + 4) & 7);
                    const double term = (double)p * a;
                    m = first ? term : m + term;
                    den += p;
                    first = false;
                } else if (a != a) {
                    nan = true;
                } else {
                    if (first) m = a;
                    else if (statistic == HDEM_DD_MAXIMUM) m = a > m ? a : m;
                    else m = a < m ? a : m;
                    first = false;
                }
            }
            if (!ready) continue;
            double D = m;
            if (!single) {
                if (statistic == HDEM_DD_AVERAGE) D = m / (double)den;
                else if (statistic == HDEM_DD_MAXIMUM) D = nan ? qnan : m;
                else D = first ? qnan : m;
            }
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

__global__ __launch_bounds__(NT) void dinfdistup_final_kernel(
    const uint64_t *__restrict__ work, int H, int W, int tiles_x, float *__restrict__ distance,
    dinfdistup_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_nan, s_unresolved;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid == 0) s_nan = 0, s_unresolved = 0;
    __syncthreads();

    unsigned int nan = 0, unresolved = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        const uint64_t vc = work[g];
        const double D = __longlong_as_double((long long)vc);
        unresolved += vc == NOT_FINAL;
        nan += vc == QNAN;
        distance[g] = D != D ? __uint_as_float(0x7FC00000u) : (float)D;
    }
    if (nan) atomicAdd(&s_nan, nan);
    if (unresolved) atomicAdd(&s_unresolved, unresolved);
    __syncthreads();
    if (tid == 0) {
        if (s_nan) atomicAdd(&cnt->nan, (unsigned long long)s_nan);
        if (s_unresolved) atomicAdd(&cnt->unresolved, (unsigned long long)s_unresolved);
    }
}

// What a call is given.
struct dinfdistup_call {
    const uint32_t *words;
    int H, W;
    const float *dem;
    double dx, dy;
    int kind, statistic;
    uint32_t min_share;
    float *distance;
};

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// also the tile grid: nothing is allocated for a raster that is refused
int dinfdistup_check(const hdem_ctx *ctx, const dinfdistup_call &a, int flags,
                     const hdem_dinfdistup_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.words && a.distance, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(a.H > 0 && a.W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", a.H, a.W);
    if (int rc = d8_check_stats(stats, "hdem_dinfdistup_stats")) return rc;
    HDEM_REQUIRE(a.kind >= HDEM_DD_HORIZONTAL && a.kind <= HDEM_DD_SURFACE, HDEM_ERR_BAD_ARG,
                 "unknown distance kind %d", a.kind);
    HDEM_REQUIRE(a.statistic >= HDEM_DD_AVERAGE && a.statistic <= HDEM_DD_MAXIMUM,
                 HDEM_ERR_BAD_ARG, "unknown distance statistic %d", a.statistic);
    HDEM_REQUIRE(a.min_share >= 1 && a.min_share <= Q_ONE, HDEM_ERR_BAD_ARG,
                 "min_share is 1 ... 32768 (units of 2^-15), got %u", a.min_share);
    if (a.kind == HDEM_DD_HORIZONTAL)
        HDEM_REQUIRE(!a.dem, HDEM_ERR_BAD_ARG, "the horizontal distance takes no dem");
    else
        HDEM_REQUIRE(a.dem, HDEM_ERR_BAD_ARG,
                     "the vertical and surface distances need the dem they are measured on");
    HDEM_REQUIRE(positive(a.dx) && positive(a.dy), HDEM_ERR_BAD_ARG,
                 "dx and dy must be finite and positive, got %g and %g", a.dx, a.dy);
    HDEM_REQUIRE(!(flags & ~HDEM_ON_DEVICE), HDEM_ERR_BAD_ARG,
                 "D-infinity distance up: unknown flags 0x%x", flags);
    if (int rc = d8_grid_of("D-infinity distance up", a.H, a.W, g)) return rc;
    const uintptr_t n4 = (uintptr_t)a.H * a.W * 4, out = (uintptr_t)a.distance;
    const uintptr_t in_w = (uintptr_t)a.words, in_z = (uintptr_t)a.dem;
    HDEM_REQUIRE(out + n4 <= in_w || in_w + n4 <= out, HDEM_ERR_BAD_ARG,
                 "D-infinity distance up: distance overlaps words");
    HDEM_REQUIRE(!a.dem || out + n4 <= in_z || in_z + n4 <= out, HDEM_ERR_BAD_ARG,
                 "D-infinity distance up: distance overlaps dem");
    return HDEM_OK;
}

// The distance on device pointers, after dinfdistup_check.  *st is filled when the launches ran,
// whatever is returned; the caller publishes it.
int dinfdistup_dev(hdem_ctx *ctx, const dinfdistup_call &a, const d8_grid &g, bool want_stats,
                   hdem_dinfdistup_stats *st)
{
    const int H = a.H, W = a.W, tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;

    // arena: counters | left, stamp, list: u32 per tile each | the working raster, u64 per cell
    const size_t head = 512;
    static_assert(sizeof(dinfdistup_counters) <= head, "counters outgrew their block");
    const size_t per_tile = hdem_round16((size_t)tiles * 12);
    char *ws = static_cast<char *>(hdem_arena(ctx, head + per_tile + (size_t)cells * 8));
    if (!ws) return HDEM_ERR_OOM;
    dinfdistup_counters *cnt = reinterpret_cast<dinfdistup_counters *>(ws);
    uint32_t *left = reinterpret_cast<uint32_t *>(ws + head);
    uint32_t *stamp = left + tiles, *list = stamp + tiles;
    uint64_t *work = reinterpret_cast<uint64_t *>(ws + head + per_tile);

    dinfdistup_steps steps;
    steps.dx = a.dx, steps.dy = a.dy, steps.diag = std::sqrt(a.dx * a.dx + a.dy * a.dy);
    steps.dx2 = steps.dx * steps.dx, steps.dy2 = steps.dy * steps.dy;
    steps.diag2 = steps.diag * steps.diag;

    hdem_event_timer<4> phases(ctx, want_stats);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(dinfdistup_counters), ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    hipLaunchKernelGGL(dinfdistup_classify_kernel, grid, dim3(NT), 0, ctx->stream, a.words,
                       a.min_share, H, W, tiles_x, work, left, stamp, list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    dinfdistup_counters host = {};
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
#define HDEM_DINFDISTUP_VISIT(KIND)                                                               \
    hipLaunchKernelGGL(dinfdistup_visit_kernel<KIND>, dim3(host.listed), dim3(NT), 0,             \
                       ctx->stream, a.words, a.dem, work, H, W, tiles_x, list, (uint32_t)rounds,  \
                       steps, a.statistic, a.min_share, stamp, left)
        if (a.kind == HDEM_DD_HORIZONTAL) HDEM_DINFDISTUP_VISIT(HDEM_DD_HORIZONTAL);
        else if (a.kind == HDEM_DD_VERTICAL) HDEM_DINFDISTUP_VISIT(HDEM_DD_VERTICAL);
        else HDEM_DINFDISTUP_VISIT(HDEM_DD_SURFACE);
#undef HDEM_DINFDISTUP_VISIT
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(dinfdistup_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           left, stamp, list, cnt);
    }
    phases.mark(2);
    if (!refused) {
        hipLaunchKernelGGL(dinfdistup_final_kernel, grid, dim3(NT), 0, ctx->stream, work, H, W,
                           tiles_x, a.distance, cnt);
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
    st->tile_visits = visits;
    st->ridge_cells = (int64_t)host.ridge;
    st->counted_links = (int64_t)host.counted;
    st->ignored_links = (int64_t)host.ignored;
    st->merge_cells = (int64_t)host.merge;
    st->nan_cells = (int64_t)host.nan;
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
                 "D-infinity words form a cycle of counted links: %llu cells never resolve",
                 host.unresolved);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: one symbol; HDEM_ON_DEVICE in flags says the pointers are device pointers
// ---------------------------------------------------------------------------
extern "C" int hdem_dinfdistup_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W,
                                   const float *dem, double dx, double dy, int kind,
                                   int statistic, uint32_t min_share, float *distance, int flags,
                                   hdem_dinfdistup_stats *stats)
{
    dinfdistup_call a = {words, H, W, dem, dx, dy, kind, statistic, min_share, distance};
    d8_grid g;
    if (int rc = dinfdistup_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dinfdistup_stats st = {};
    d8_publish(stats, st);

    const size_t n = (size_t)H * W;
    hdem_dbuf dwords, ddem, ddistance;
    if (!(flags & HDEM_ON_DEVICE)) {
        if (int rc = dwords.upload(ctx, words, n * 4)) return rc;
        if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
        if (int rc = ddistance.alloc(ctx, n * 4)) return rc;
        a.words = dwords.as<const uint32_t>();
        a.dem = ddem.as<const float>(), a.distance = ddistance.as<float>();
    }
    const int rc = dinfdistup_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, st);
    if (rc || (flags & HDEM_ON_DEVICE)) return rc;
    return ddistance.download(distance, n * 4);
}
