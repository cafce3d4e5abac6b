// A20 / A21 / A22  D-infinity flow direction, accumulation and weighted accumulation (Tarboton
// 1997; new operators; include/hydrodem_hip.h has the contract, DESIGN 3.24 and 3.25 the argument).
//
// The word of a cell: q in bits 0-15 (the share of the diagonal receiver in units of 2^-15),
// the facet in bits 16-19.  Directions are numbered counter-clockwise from east, 0 = E,
// 1 = NE, 2 = N ... 7 = SE, so that facet k has its cardinal receiver in direction
// 2 * ((k >> 1) & 3) and its diagonal one in direction 2 * ((k - 1) >> 1) + 1, and bit b
// of an ESRI D8 code is direction (8 - b) & 7.
//
// Direction (dinf_kernel): one launch on the staging of hdem_stencil_tile.h, a thread per
// column of the 256 x 32 tile, eight facets per cell in float64, one atan2 for the winner.
//
// Accumulation is a pull over donors on a DAG, in the structure of hdem_flats.hip:
//   classify  (dinfacc_classify_kernel)  per tile: words validated and counted, the working
//             raster (uint64 per cell, bit 63 = final, the low bits A) set to "not final",
//             every tile listed for round 0.  It writes every word that is read later.  The
//             weighted form (A22) quantises the cell's weight here and leaves q(w) in the low
//             bits of the "not final" word: the cell's own term, at no extra raster.
//   visit     (dinfacc_visit_kernel)  one workgroup per listed tile: words and values of the
//             tile and its one-cell halo in LDS; the donors of every cell as a bit mask beside
//             its word; then a cell that is not final and whose donors are all final becomes
//             final with U (weighted: the q(w) its own not-yet-final word holds; a donor's word
//             is only read once its FINAL bit has been seen, so the two uses never meet) + the
//             sum of their shares, until the tile stops changing.  One
//             iteration is four directional sweeps, one wave each (down the rows, up, along the
//             columns to the right, to the left), so that a straight reach resolves in one
//             iteration.  The waves do not wait for each other inside an iteration: a cell only
//             ever goes from "not final" to one final value, flag and value are one 64-bit LDS
//             word, and two waves that finalise the same cell store the same word.  Halo cells
//             are read-only.  The cells that became final are written back; if one of them is
//             on the tile's frame the tile stamps the round.
//   schedule  (dinfacc_schedule_kernel)  a tile that still has cells to finalise runs again
//             when one of its eight neighbours stamped the round just run.  The host reads the
//             length of the list, one word per round; an empty list ends the loop.
//   final     (dinfacc_final_kernel)  streaming: the flag stripped, sum and value written,
//             the cells that never became final counted: any at all is a cycle.
// Schedule freedom: the final value of a cell is a function of its donors' final values alone
// and integer addition has no order, so a cell has one possible final word whoever computes it
// and whenever.  A halo word is read with one relaxed 64-bit load: it is "not final" or the
// final word, never half of each; a stale "not final" costs a round, because the neighbour
// that finalises the cell afterwards stamps its round and that puts this tile on the next
// list.  Visibility between tiles comes from the kernel boundaries alone (the per-XCD L2s are
// not coherent inside a launch): no fences, and no workgroup waits for another.  Bounds: an
// iteration that changes the tile makes at least one cell final, so at most 4096 of them; a
// round with a non-empty list follows a round that made a frame cell final, so at most
// H * W + 1 rounds.
#include "hdem_d8tile.h"
#include "hdem_stencil_tile.h"

#include <cmath>

namespace {

constexpr uint32_t Q_ONE = 32768;             // q of "everything to the diagonal receiver"
constexpr uint64_t FINAL = 1ull << 63;
constexpr int LH = TS + 2;                    // LDS rows: the tile and its halo
constexpr int LW = TS + 3;                    // LDS row pitch: odd, so a column sweep (one lane
                                              // per row) is free of bank conflicts
constexpr double HALF_PI = 1.57079632679489661923;

// direction d -> (dy, dx), packed (d + 1) in 4 bits per entry
__host__ __device__ __forceinline__ int dir_dy(int d) { return ((0x22210001u >> (4 * d)) & 3) - 1; }
__host__ __device__ __forceinline__ int dir_dx(int d) { return ((0x21000122u >> (4 * d)) & 3) - 1; }
__device__ __forceinline__ int facet_card(uint32_t f) { return 2 * ((f >> 1) & 3); }
__device__ __forceinline__ int facet_diag(uint32_t f) { return 2 * ((f - 1) >> 1) + 1; }

__device__ __forceinline__ bool word_valid(uint32_t w)
{
    const uint32_t f = (w >> 16) & 15, q = w & 0xFFFFu;
    return (w >> 20) == 0 && f <= 8 && q <= Q_ONE && (f != 0 || q == 0);
}
// does the (valid) word w send a non-zero share in direction `toward`?
__device__ __forceinline__ bool word_gives(uint32_t w, int toward)
{
    const uint32_t f = (w >> 16) & 15, q = w & 0xFFFFu;
    if (!f) return false;
    return (toward & 1) ? q != 0 && facet_diag(f) == toward : q != Q_ONE && facet_card(f) == toward;
}
// what a donor with word w and area a sends in direction `toward` (word_gives holds)
__device__ __forceinline__ uint64_t word_share(uint32_t w, uint64_t a, int toward)
{
    const uint64_t diag = (a * (uint64_t)(w & 0xFFFFu)) >> 15;
    return (toward & 1) ? diag : a - diag;
}
// the canonical word of the ESRI D8 code c (one bit set)
__device__ __forceinline__ uint32_t word_of_code(uint32_t c, int *dir)
{
    const int d = (8 - __builtin_ctz(c)) & 7;
    *dir = d;
    return ((uint32_t)max(d, 1) << 16) | ((d & 1) ? Q_ONE : 0u);
}

// ---------------------------------------------------------------------------
// A20  direction
// ---------------------------------------------------------------------------
enum { D_NOFLOW, D_FALLBACK, D_INVALID, D_COUNT };

struct dinf_args {
    const float *z;
    const uint8_t *fallback;
    uint32_t *words;
    float *angle, *slope;
    int H, W, tiles_x;
    double dx, dy, diag;            // diag = sqrt(dx^2 + dy^2)
    double t_ew, t_ns;              // atan2(d2, d1) of the facets on E / W and on N / S
    unsigned long long *cnt;        // D_COUNT counters, zeroed by the caller
};

__global__ __launch_bounds__(NT) void dinf_kernel(const dinf_args p)
{
    __shared__ __attribute__((aligned(16))) float t[(TH + 2) * LS];
    __shared__ unsigned int s_cnt[D_COUNT];
    const int H = p.H, W = p.W;
    const int bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int x0 = bx * TW, y0 = by * TH;
    if (threadIdx.x < D_COUNT) s_cnt[threadIdx.x] = 0;
    stage_tile<float, false, true>(p.z, H, W, y0, x0, t);
    __syncthreads();

    const int x = x0 + (int)threadIdx.x;
    unsigned int n[D_COUNT] = {0, 0, 0};
    if (x < W) {
#pragma unroll 1
        for (int lr = 0; lr < TH; ++lr) {
            const int y = y0 + lr;
            if (y >= H) break;
            // the window by direction: LDS row lr + 1 is the centre's
            const float *c = t + (lr + 1) * LS + 4 + threadIdx.x;
            const float centre = c[0];
            const double e0 = centre;
            const double nb[8] = {c[1], c[1 - LS], c[-LS], c[-1 - LS],
                                  c[-1], c[-1 + LS], c[LS], c[1 + LS]};
            double best = 0.0, s1w = 0.0, s2w = 0.0;
            int facet = 0, how = 0;
            if (centre == centre && y > 0 && y < H - 1 && x > 0 && x < W - 1) {
#pragma unroll
                for (int k = 1; k <= 8; ++k) {
                    const int dc = 2 * ((k >> 1) & 3), dd = 2 * ((k - 1) >> 1) + 1;
                    const double e1 = nb[dc], e2 = nb[dd];
                    if (e1 != e1 || e2 != e2) continue;
                    const bool ew = dc == 0 || dc == 4;
                    const double d1 = ew ? p.dx : p.dy, d2 = ew ? p.dy : p.dx;
                    const double s1 = (e0 - e1) / d1, s2 = (e1 - e2) / d2;
                    double s;
                    int h;
                    if (s2 <= 0.0) {
                        s = s1, h = 0;
                    } else if (s2 * d1 >= s1 * d2) {
                        s = (e0 - e2) / p.diag, h = 1;
                    } else {
                        s = sqrt(s1 * s1 + s2 * s2), h = 2;
                    }
                    if (s > best) best = s, facet = k, how = h, s1w = s1, s2w = s2;
                }
            }
            uint32_t word = 0;
            float ang = -1.0f;
            if (facet) {
                const int dc = facet_card(facet);
                const double theta = (dc == 0 || dc == 4) ? p.t_ew : p.t_ns;
                const double r = how == 0 ? 0.0 : how == 1 ? theta : atan2(s2w, s1w);
                const uint32_t q = how == 0   ? 0u
                                   : how == 1 ? Q_ONE
                                              : (uint32_t)rint(r / theta * 32768.0);
                word = ((uint32_t)facet << 16) | q;
                if (p.angle) {
                    const double af = (facet & 1) ? 1.0 : -1.0;
                    const double a = af * r + (double)(facet >> 1) * HALF_PI;
                    ang = a >= 4.0 * HALF_PI ? 0.0f : (float)a;
                }
            } else if (p.fallback) {
                const uint32_t code = p.fallback[(size_t)y * W + x];
                if (code & (code - 1)) {
                    ++n[D_INVALID];
                } else if (code) {
                    int d;
                    word = word_of_code(code, &d);
                    ang = (float)((double)d * (HALF_PI / 2.0));
                    ++n[D_FALLBACK];
                }
            }
            n[D_NOFLOW] += word == 0;
            const size_t at = (size_t)y * W + x;
            p.words[at] = word;
            if (p.angle) p.angle[at] = ang;
            if (p.slope) p.slope[at] = centre == centre ? (float)best : __builtin_nanf("");
        }
    }
    // lane -> wave -> workgroup -> one global atomic per counter
#pragma unroll
    for (int j = 0; j < D_COUNT; ++j) {
        unsigned int v = n[j];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[j], v);
    }
    __syncthreads();
    if (threadIdx.x < D_COUNT && s_cnt[threadIdx.x])
        atomicAdd(&p.cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

int dinf_check(const hdem_ctx *ctx, const float *dem, int H, int W, double dx, double dy,
               const uint32_t *words, int flags, const hdem_dinf_stats *stats, int *tiles_x,
               int64_t *tiles)
{
    if (int rc = hdem_check_call(ctx, dem, words, H, W)) return rc;
    if (int rc = d8_check_stats(stats, "hdem_dinf_stats")) return rc;
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "D-infinity flow direction: unknown flags 0x%x", flags);
    HDEM_REQUIRE(positive(dx) && positive(dy), HDEM_ERR_BAD_ARG,
                 "dx and dy must be finite and positive, got %g and %g", dx, dy);
    *tiles_x = (W + TW - 1) / TW;
    *tiles = (int64_t)*tiles_x * ((H + TH - 1) / TH);
    HDEM_REQUIRE(*tiles <= INT32_MAX, HDEM_ERR_BAD_ARG,
                 "D-infinity flow direction: %d x %d has %lld tiles of %d x %d, more than %d", H,
                 W, (long long)*tiles, TH, TW, INT32_MAX);
    return HDEM_OK;
}

// ---------------------------------------------------------------------------
// A21  accumulation
// ---------------------------------------------------------------------------
struct dinfacc_counters {
    unsigned long long split;         // cells with two receivers
    unsigned long long terminal;      // cells with facet 0
    unsigned long long bad;           // invalid words
    unsigned long long outside;       // cells with a receiver outside the raster
    unsigned long long unresolved;    // cells that never became final
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
    // the weighted form (A22) alone, behind what the unweighted one reads
    unsigned long long nan;           // NaN weights (they contribute 0)
    unsigned long long negative;      // weights below 0 (-inf among them)
    unsigned long long infinite;      // +inf
    unsigned long long over;          // q(w) > 2^31 - 1
    unsigned long long total;         // the sum of q(w) over the raster
};
constexpr size_t COUNTERS_UNWEIGHTED = offsetof(dinfacc_counters, nan);
constexpr double Q_MAX = 2147483647.0;
constexpr unsigned long long TOTAL_LIMIT = 1ull << 48;

// q(w) of cell g (hdem_flowsum.hip's rule; integer weights shifted by frac_bits); a weight that
// is refused counts 0.  n[]: what the weight is counted as (nan, negative, infinite, over).
template <int WT>
__device__ __forceinline__ uint64_t dinf_weight_of(const void *__restrict__ weights, size_t g,
                                                   double scale, int frac_bits,
                                                   unsigned int (&n)[4])
{
    if (WT == HDEM_FLOWSUM_F32) {
        const float f = static_cast<const float *>(weights)[g];
        if (f != f) { ++n[0]; return 0; }
        if (f < 0.0f) { ++n[1]; return 0; }                    // -0.0 is not: it counts as 0
        if (f == __builtin_inff()) { ++n[2]; return 0; }
        const double d = rint((double)f * scale);   // exact product, one rounding to nearest even
        if (d > Q_MAX) { ++n[3]; return 0; }
        return (uint64_t)(long long)d;
    }
    const uint64_t v = (uint64_t)(WT == HDEM_FLOWSUM_U32 ? static_cast<const uint32_t *>(weights)[g]
                                                          : static_cast<const uint8_t *>(weights)[g])
                       << frac_bits;
    if (v > 0x7FFFFFFFull) { ++n[3]; return 0; }
    return v;
}

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

// WT: 0 for the unweighted form, else the HDEM_FLOWSUM_* type of the weights
template <int WT>
__global__ __launch_bounds__(NT) void dinfacc_classify_kernel(
    const uint32_t *__restrict__ words, int H, int W, int tiles_x, uint64_t *__restrict__ work,
    uint32_t *__restrict__ left, uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    dinfacc_counters *__restrict__ cnt, const void *__restrict__ weights, double scale,
    int frac_bits)
{
    __shared__ unsigned int s_cnt[4];            // split, terminal, bad, outside
    __shared__ unsigned int s_wcnt[4];           // weights: nan, negative, infinite, over
    __shared__ unsigned long long s_total;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid < 4) s_cnt[tid] = 0;
    if (WT) {
        if (tid < 4) s_wcnt[tid] = 0;
        if (tid == 0) s_total = 0;
    }
    __syncthreads();

    unsigned int n[4] = {0, 0, 0, 0};
    unsigned int nw[4] = {0, 0, 0, 0};
    unsigned long long total = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const int gy = tile.y0 + ly, gx = tile.x0 + lx;
        const size_t g = (size_t)gy * W + gx;
        const uint32_t w = words[g];
        if (!word_valid(w)) {
            ++n[2];
        } else {
            const uint32_t f = w >> 16, q = w & 0xFFFFu;
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
            n[3] += out;
        }
        if (WT) {                                // not final, the own term in the low bits
            const uint64_t q = dinf_weight_of<WT>(weights, g, scale, frac_bits, nw);
            total += q;
            work[g] = q;
        } else {
            work[g] = 0;                         // not final
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (n[j]) atomicAdd(&s_cnt[j], n[j]);
    if (WT) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (nw[j]) atomicAdd(&s_wcnt[j], nw[j]);
        if (total) atomicAdd(&s_total, total);
    }
    __syncthreads();
    if (tid == 0) {
        left[blockIdx.x] = (uint32_t)(tile.th * tile.tw);
        stamp[blockIdx.x] = 0;
        list[atomicAdd(&cnt->listed, 1u)] = blockIdx.x;
        if (s_cnt[0]) atomicAdd(&cnt->split, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->terminal, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->outside, (unsigned long long)s_cnt[3]);
        if (WT) {
            if (s_wcnt[0]) atomicAdd(&cnt->nan, (unsigned long long)s_wcnt[0]);
            if (s_wcnt[1]) atomicAdd(&cnt->negative, (unsigned long long)s_wcnt[1]);
            if (s_wcnt[2]) atomicAdd(&cnt->infinite, (unsigned long long)s_wcnt[2]);
            if (s_wcnt[3]) atomicAdd(&cnt->over, (unsigned long long)s_wcnt[3]);
            if (s_total) atomicAdd(&cnt->total, s_total);
        }
    }
}

// The list of round `round` >= 1: the tiles with cells left next to a tile that made a frame
// cell final in round - 1.  One thread per tile; the order of the list changes no result.
__global__ __launch_bounds__(NT) void dinfacc_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ left,
    const uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    dinfacc_counters *__restrict__ cnt)
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

// WEIGHTED: a cell's sum starts from the q(w) in its own not-yet-final word, not from `unit`
template <bool WEIGHTED>
__global__ __launch_bounds__(NT) void dinfacc_visit_kernel(
    const uint32_t *__restrict__ words, uint64_t *work, int H, int W, int tiles_x,
    const uint32_t *__restrict__ list, uint32_t round, uint64_t unit, uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ left)
{
    __shared__ uint64_t v[LH * LW];              // bit 63: final; the low bits: A
    __shared__ uint32_t w[LH * LW];              // the word; bits 24-31: the cell's donors
    __shared__ unsigned int s_edge, s_left;

    const int tid = threadIdx.x;
    const uint32_t t = list[blockIdx.x];
    const int y0 = (int)(t / tiles_x) * TS, x0 = (int)(t % tiles_x) * TS;
    if (tid == 0) s_edge = 0, s_left = 0;

    // the tile and its halo; outside the raster: final and giving nothing
    for (int i = tid; i < LH * LH; i += NT) {
        const int hy = i / LH, hx = i % LH;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = (size_t)gy * W + gx;
        w[hy * LW + hx] = in ? words[g] : 0u;
        lds_store(&v[hy * LW + hx], in ? work_load(work + g) : FINAL);
    }
    __syncthreads();

    // the donors of the thread's 16 cells that are not final yet (`pending`: which of them);
    // a cell without donors is final at once.  Only bits 24-31 of a word change here, and the
    // donor test reads the bits below: the pass needs no barrier of its own.
    uint32_t pending = 0;
    int changed = 0;
#pragma unroll
    for (int k = 0; k < TC / NT; ++k) {
        const int i = tid + k * NT;
        const int c = (i / TS + 1) * LW + i % TS + 1;
        const uint64_t own = lds_load(&v[c]);
        if (own & FINAL) continue;
        pending |= 1u << k;
        uint32_t donors = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (word_gives(w[c + dir_dy(d) * LW + dir_dx(d)], (d + 4) & 7)) donors |= 1u << d;
        w[c] = (w[c] & 0xFFFFFFu) | (donors << 24);
        if (!donors) {
            lds_store(&v[c], FINAL | (WEIGHTED ? own : unit));
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
    for (int iter = 0; iter < TC; ++iter) {
        changed = 0;
        for (int s = 0, c = c0; s < TS; ++s, c += step) {
            const uint64_t own = lds_load(&v[c]);
            if (own & FINAL) continue;
            uint32_t donors = w[c] >> 24;
            uint64_t sum = WEIGHTED ? own : unit;
            bool ready = true;
            while (donors) {
                const int d = __builtin_ctz(donors);
                donors &= donors - 1;
                const int n = c + dir_dy(d) * LW + dir_dx(d);
                const uint64_t vn = lds_load(&v[n]);
                if (!(vn & FINAL)) {
                    ready = false;
                    break;
                }
                sum += word_share(w[n], vn & ~FINAL, (d + 4) & 7);
            }
            if (ready) {
                lds_store(&v[c], FINAL | sum);
                changed = 1;
            }
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
        if (vc & FINAL) {                                // only this workgroup writes these cells
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

__global__ __launch_bounds__(NT) void dinfacc_final_kernel(
    const uint64_t *work, int H, int W, int tiles_x, double scale, int64_t *sum,
    float *__restrict__ value, dinfacc_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_unresolved;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid == 0) s_unresolved = 0;
    __syncthreads();

    unsigned int unresolved = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
        const uint64_t vc = work[g];
        unresolved += !(vc & FINAL);
        const uint64_t a = vc & ~FINAL;
        if (sum) sum[g] = (int64_t)a;                    // may be the working raster itself
        if (value) value[g] = (float)((double)a * scale);
    }
    if (unresolved) atomicAdd(&s_unresolved, unresolved);
    __syncthreads();
    if (tid == 0 && s_unresolved)
        atomicAdd(&cnt->unresolved, (unsigned long long)s_unresolved);
}

// What a call of the accumulation is given: A21 (weights null) or A22.
struct dinfacc_call {
    const uint32_t *words;
    int H, W;
    const void *weights;              // null: every cell counts 2^frac_bits
    int weight_type, frac_bits;
    int64_t *sum;
    float *value;
};

struct span {
    const char *name;
    uintptr_t lo, hi;
};

inline size_t weight_bytes(int weight_type) { return weight_type == HDEM_FLOWSUM_U8 ? 1 : 4; }

// also the tile grid: nothing is allocated for a raster that is refused
int dinfacc_check(const hdem_ctx *ctx, const uint32_t *words, int H, int W, int frac_bits,
                  const int64_t *sum, const float *value, int flags,
                  const hdem_dinfacc_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(words, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(H > 0 && W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", H, W);
    if (int rc = d8_check_stats(stats, "hdem_dinfacc_stats")) return rc;
    HDEM_REQUIRE(sum || value, HDEM_ERR_BAD_ARG, "D-infinity flow accumulation: no output wanted");
    HDEM_REQUIRE(frac_bits >= 0 && frac_bits <= 16, HDEM_ERR_BAD_ARG,
                 "frac_bits is 0 ... 16, got %d", frac_bits);
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "D-infinity flow accumulation: unknown flags 0x%x",
                 flags);
    return d8_grid_of("D-infinity flow accumulation", H, W, g);
}

int dinfsum_check(const hdem_ctx *ctx, const dinfacc_call &a, int flags,
                  const hdem_dinfsum_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.words, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(a.H > 0 && a.W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", a.H, a.W);
    if (int rc = d8_check_stats(stats, "hdem_dinfsum_stats")) return rc;
    HDEM_REQUIRE(a.sum || a.value, HDEM_ERR_BAD_ARG,
                 "weighted D-infinity flow accumulation: no output wanted");
    HDEM_REQUIRE(a.weights, HDEM_ERR_BAD_ARG, "the weight raster is null");
    HDEM_REQUIRE(a.weight_type >= HDEM_FLOWSUM_F32 && a.weight_type <= HDEM_FLOWSUM_U8,
                 HDEM_ERR_BAD_ARG, "unknown weight type %d", a.weight_type);
    if (a.weight_type == HDEM_FLOWSUM_F32)
        HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 30, HDEM_ERR_BAD_ARG,
                     "frac_bits is 0 ... 30, got %d", a.frac_bits);
    else
        HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 16, HDEM_ERR_BAD_ARG,
                     "integer weights take frac_bits 0 ... 16, got %d", a.frac_bits);
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG,
                 "weighted D-infinity flow accumulation: unknown flags 0x%x", flags);
    if (int rc = d8_grid_of("weighted D-infinity flow accumulation", a.H, a.W, g)) return rc;
    const size_t n = (size_t)a.H * a.W;
    span s[4];
    int ns = 0;
    s[ns++] = {"words", (uintptr_t)a.words, (uintptr_t)a.words + 4 * n};
    s[ns++] = {"weights", (uintptr_t)a.weights,
               (uintptr_t)a.weights + n * weight_bytes(a.weight_type)};
    const span outs[2] = {{"sum", (uintptr_t)a.sum, (uintptr_t)a.sum + 8 * n},
                          {"value", (uintptr_t)a.value, (uintptr_t)a.value + 4 * n}};
    for (const span &o : outs) {
        if (!o.lo) continue;
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "weighted D-infinity flow accumulation: %s overlaps %s", o.name,
                         s[j].name);
        s[ns++] = o;
    }
    return HDEM_OK;
}

void launch_classify(hdem_ctx *ctx, const dinfacc_call &a, const d8_grid &g, uint64_t *work,
                     uint32_t *left, uint32_t *stamp, uint32_t *list, dinfacc_counters *cnt)
{
    const dim3 grid((unsigned)g.tiles), block(NT);
    const double scale = (double)(1ll << a.frac_bits);
#define HDEM_DINF_CLASSIFY(WT)                                                                    \
    hipLaunchKernelGGL((dinfacc_classify_kernel<WT>), grid, block, 0, ctx->stream, a.words, a.H,  \
                       a.W, g.tiles_x, work, left, stamp, list, cnt, a.weights, scale, a.frac_bits)
    if (!a.weights) HDEM_DINF_CLASSIFY(0);
    else if (a.weight_type == HDEM_FLOWSUM_F32) HDEM_DINF_CLASSIFY(HDEM_FLOWSUM_F32);
    else if (a.weight_type == HDEM_FLOWSUM_U32) HDEM_DINF_CLASSIFY(HDEM_FLOWSUM_U32);
    else HDEM_DINF_CLASSIFY(HDEM_FLOWSUM_U8);
#undef HDEM_DINF_CLASSIFY
}

// The accumulation of both forms on device pointers.  *st is filled when the launches ran, whatever
// is returned; the caller publishes it.
int dinfacc_dev(hdem_ctx *ctx, const dinfacc_call &a, const d8_grid &g, bool want_stats,
                hdem_dinfsum_stats *st)
{
    const bool weighted = a.weights != nullptr;
    const int H = a.H, W = a.W, tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;

    // arena: counters | left, stamp, list: u32 per tile each | the working raster, u64 per
    // cell, unless the caller's sum serves
    const size_t head = 512;
    static_assert(sizeof(dinfacc_counters) <= head, "counters outgrew their block");
    const size_t per_tile = hdem_round16((size_t)tiles * 12);
    const size_t bytes = head + per_tile + (a.sum ? 0 : (size_t)cells * 8);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    dinfacc_counters *cnt = reinterpret_cast<dinfacc_counters *>(ws);
    uint32_t *left = reinterpret_cast<uint32_t *>(ws + head);
    uint32_t *stamp = left + tiles, *list = stamp + tiles;
    uint64_t *work = a.sum ? reinterpret_cast<uint64_t *>(a.sum)
                           : reinterpret_cast<uint64_t *>(ws + head + per_tile);
    const uint64_t unit = 1ull << (weighted ? 0 : a.frac_bits);
    // the unweighted form neither zeroes nor reads the counters of the weights
    const size_t cnt_bytes = weighted ? sizeof(dinfacc_counters) : COUNTERS_UNWEIGHTED;

    hdem_event_timer<4> phases(ctx, want_stats);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, cnt_bytes, ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    launch_classify(ctx, a, g, work, left, stamp, list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    dinfacc_counters host = {};
    int64_t rounds = 0, visits = 0;
    bool refused = false;
    for (;; ++rounds) {
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        refused = host.bad || host.outside || host.negative || host.infinite || host.over ||
                  host.total >= TOTAL_LIMIT;
        if (refused || !host.listed || rounds > cells) break;
        visits += host.listed;
        if (weighted)
            hipLaunchKernelGGL(dinfacc_visit_kernel<true>, dim3(host.listed), dim3(NT), 0,
                               ctx->stream, a.words, work, H, W, tiles_x, list, (uint32_t)rounds,
                               unit, stamp, left);
        else
            hipLaunchKernelGGL(dinfacc_visit_kernel<false>, dim3(host.listed), dim3(NT), 0,
                               ctx->stream, a.words, work, H, W, tiles_x, list, (uint32_t)rounds,
                               unit, stamp, left);
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(dinfacc_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           left, stamp, list, cnt);
    }
    phases.mark(2);
    if (!refused) {
        hipLaunchKernelGGL(dinfacc_final_kernel, grid, dim3(NT), 0, ctx->stream, work, H, W,
                           tiles_x, std::ldexp(1.0, -a.frac_bits), a.sum, a.value, cnt);
        HDEM_HIP_CHECK(hipGetLastError());
        HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    phases.mark(3);
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
    st->tile_visits = visits;
    st->split_cells = (int64_t)host.split;
    st->terminal_cells = (int64_t)host.terminal;
    st->invalid = (int64_t)host.bad;
    st->outside = (int64_t)host.outside;
    st->unresolved = (int64_t)host.unresolved;
    st->tile_h = TS;
    st->tile_w = TS;
    phases.read(&st->ms_classify, &st->ms_relax, &st->ms_final);
    st->nan_weights = (int64_t)host.nan;
    st->bad_weights = (int64_t)(host.negative + host.infinite + host.over);
    st->total = host.total;
    HDEM_REQUIRE(!host.bad, HDEM_ERR_BAD_ARG,
                 "invalid D-infinity word in %llu cells: the facet is 0 ... 8 in bits 16-19, q is "
                 "0 ... 32768 in bits 0-15 (0 with facet 0), every other bit is 0",
                 host.bad);
    HDEM_REQUIRE(!host.outside, HDEM_ERR_BAD_ARG,
                 "D-infinity words send flow outside the raster in %llu cells", host.outside);
    HDEM_REQUIRE(!host.negative && !host.infinite && !host.over, HDEM_ERR_BAD_ARG,
                 "weights out of range in %llu cells: %llu negative, %llu infinite, %llu above "
                 "2^31 - 1 once quantised (frac_bits %d)",
                 host.negative + host.infinite + host.over, host.negative, host.infinite,
                 host.over, a.frac_bits);
    HDEM_REQUIRE(host.total < TOTAL_LIMIT, HDEM_ERR_BAD_ARG,
                 "the quantised weights sum to %llu: the total must stay below 2^48 (frac_bits %d)",
                 host.total, a.frac_bits);
    HDEM_REQUIRE(!host.unresolved, HDEM_ERR_BAD_ARG,
                 "D-infinity words form a cycle: %llu cells never resolve", host.unresolved);
    return HDEM_OK;
}

// hdem_dinfsum_stats opens with the fields of hdem_dinfacc_stats
static_assert(offsetof(hdem_dinfsum_stats, reserved) == offsetof(hdem_dinfacc_stats, reserved) &&
                  offsetof(hdem_dinfsum_stats, nan_weights) == sizeof(hdem_dinfacc_stats),
              "the weighted stats no longer open with the unweighted ones");
inline hdem_dinfacc_stats unweighted_stats(const hdem_dinfsum_stats &st)
{
    hdem_dinfacc_stats out;
    memcpy(&out, &st, sizeof(out));
    return out;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_dinf_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W,
                                 const uint8_t *fallback, double dx, double dy, uint32_t *words,
                                 float *angle, float *slope, int flags, hdem_dinf_stats *stats)
{
    int tiles_x;
    int64_t tiles;
    if (int rc = dinf_check(ctx, dem, H, W, dx, dy, words, flags, stats, &tiles_x, &tiles))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dinf_stats st = {};
    d8_publish(stats, st);
    unsigned long long *cnt =
        static_cast<unsigned long long *>(hdem_arena(ctx, D_COUNT * sizeof(unsigned long long)));
    if (!cnt) return HDEM_ERR_OOM;

    dinf_args p = {};
    p.z = dem, p.fallback = fallback, p.words = words, p.angle = angle, p.slope = slope;
    p.H = H, p.W = W, p.tiles_x = tiles_x;
    p.dx = dx, p.dy = dy, p.diag = std::sqrt(dx * dx + dy * dy);
    p.t_ew = std::atan2(dy, dx), p.t_ns = std::atan2(dx, dy);
    p.cnt = cnt;

    hdem_event_timer<2> timer(ctx, stats != nullptr);   // around the launch
    if (int rc = timer.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, D_COUNT * sizeof(unsigned long long), ctx->stream));
    timer.mark(0);
    hipLaunchKernelGGL(dinf_kernel, dim3((unsigned)tiles), dim3(NT), 0, ctx->stream, p);
    timer.mark(1);
    HDEM_HIP_CHECK(hipGetLastError());
    unsigned long long host[D_COUNT] = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.no_flow = (int64_t)host[D_NOFLOW];
    st.fallback_cells = (int64_t)host[D_FALLBACK];
    st.ms_total = timer.ms(0, 1);
    d8_publish(stats, st);
    return d8_report_invalid(host[D_INVALID]);
}

extern "C" int hdem_dinf_f32(hdem_ctx *ctx, const float *dem, int H, int W,
                             const uint8_t *fallback, double dx, double dy, uint32_t *words,
                             float *angle, float *slope, int flags, hdem_dinf_stats *stats)
{
    int tiles_x;
    int64_t tiles;
    if (int rc = dinf_check(ctx, dem, H, W, dx, dy, words, flags, stats, &tiles_x, &tiles))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf ddem, dfb, dwords, dangle, dslope;
    if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
    if (int rc = dfb.upload(ctx, fallback, n)) return rc;
    if (int rc = dwords.alloc(ctx, n * 4)) return rc;
    if (angle)
        if (int rc = dangle.alloc(ctx, n * 4)) return rc;
    if (slope)
        if (int rc = dslope.alloc(ctx, n * 4)) return rc;
    if (int rc = hdem_dinf_f32_dev(ctx, ddem.as<const float>(), H, W, dfb.as<const uint8_t>(), dx,
                                   dy, dwords.as<uint32_t>(), dangle.as<float>(),
                                   dslope.as<float>(), flags, stats))
        return rc;
    if (int rc = dwords.download(words, n * 4)) return rc;
    if (angle)
        if (int rc = dangle.download(angle, n * 4)) return rc;
    return slope ? dslope.download(slope, n * 4) : HDEM_OK;
}

extern "C" int hdem_dinfacc_u32_dev(hdem_ctx *ctx, const uint32_t *words, int H, int W,
                                    int frac_bits, int64_t *sum, float *value, int flags,
                                    hdem_dinfacc_stats *stats)
{
    d8_grid g;
    if (int rc = dinfacc_check(ctx, words, H, W, frac_bits, sum, value, flags, stats, &g))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dinfsum_stats st = {};
    d8_publish(stats, unweighted_stats(st));
    const dinfacc_call a = {words, H, W, nullptr, 0, frac_bits, sum, value};
    const int rc = dinfacc_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, unweighted_stats(st));
    return rc;
}

extern "C" int hdem_dinfacc_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W, int frac_bits,
                                int64_t *sum, float *value, int flags, hdem_dinfacc_stats *stats)
{
    d8_grid g;
    if (int rc = dinfacc_check(ctx, words, H, W, frac_bits, sum, value, flags, stats, &g))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dwords, dsum, dvalue;
    if (int rc = dwords.upload(ctx, words, n * 4)) return rc;
    if (sum)
        if (int rc = dsum.alloc(ctx, n * 8)) return rc;
    if (value)
        if (int rc = dvalue.alloc(ctx, n * 4)) return rc;
    if (int rc = hdem_dinfacc_u32_dev(ctx, dwords.as<const uint32_t>(), H, W, frac_bits,
                                      dsum.as<int64_t>(), dvalue.as<float>(), flags, stats))
        return rc;
    if (sum)
        if (int rc = dsum.download(sum, n * 8)) return rc;
    return value ? dvalue.download(value, n * 4) : HDEM_OK;
}

extern "C" int hdem_dinfsum_u32_dev(hdem_ctx *ctx, const uint32_t *words, int H, int W,
                                    const void *weights, int weight_type, int frac_bits,
                                    int64_t *sum, float *value, int flags,
                                    hdem_dinfsum_stats *stats)
{
    const dinfacc_call a = {words, H, W, weights, weight_type, frac_bits, sum, value};
    d8_grid g;
    if (int rc = dinfsum_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_dinfsum_stats st = {};
    d8_publish(stats, st);
    const int rc = dinfacc_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, st);
    return rc;
}

extern "C" int hdem_dinfsum_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W,
                                const void *weights, int weight_type, int frac_bits, int64_t *sum,
                                float *value, int flags, hdem_dinfsum_stats *stats)
{
    const dinfacc_call a = {words, H, W, weights, weight_type, frac_bits, sum, value};
    d8_grid g;
    if (int rc = dinfsum_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dwords, dweights, dsum, dvalue;
    if (int rc = dwords.upload(ctx, words, n * 4)) return rc;
    if (int rc = dweights.upload(ctx, weights, n * weight_bytes(weight_type))) return rc;
    if (sum)
        if (int rc = dsum.alloc(ctx, n * 8)) return rc;
    if (value)
        if (int rc = dvalue.alloc(ctx, n * 4)) return rc;
    if (int rc = hdem_dinfsum_u32_dev(ctx, dwords.as<const uint32_t>(), H, W, dweights.p,
                                      weight_type, frac_bits, dsum.as<int64_t>(),
                                      dvalue.as<float>(), flags, stats))
        return rc;
    if (sum)
        if (int rc = dsum.download(sum, n * 8)) return rc;
    return value ? dvalue.download(value, n * 4) : HDEM_OK;
}
