// Longest upstream D8 flow length (new operator; UpstreamFlowLength).
//
// up(c) = (0, 0) for a cell without a donor, else the greatest up(d) + step(d) over the
// neighbours d whose code points at c; step = (1, 0) for a cardinal code, (0, 1) for a diagonal
// one.  A pair (ncard, ndiag) stands for the length ncard + ndiag * sqrt(2), and pairs are
// ordered by that real number, decided in integers (pair_longer): sqrt(2) is irrational, so
// two different pairs never tie, and the order is translation-invariant,
// max(p, q) + s = max(p + s, q + s).  That is flow accumulation's recursion in (max, +) for
// (+, x), and the scheme is hdem_flowacc.hip's: the codes, what makes a cell terminal, the
// tiles and their perimeter slots of hdem_d8tile.h, four launches whatever the length of the
// longest path, no workgroup ever waits on another.
//   A  (upstream_tile_kernel<false>)  per 64 x 64 tile: "last donor continues" walks.  A pair
//      is one 64-bit LDS word (ncard << 32 | ndiag), too wide to be maxed by one atomic in an
//      order that is not lexicographic, so a cell stores its final pair and then makes one
//      returning LDS add on its receiver's arrival counter (a byte of a 32-bit word, acquire /
//      release at workgroup scope); the arrival that completes the receiver gathers its
//      in-tile donors (at most 8, from a mask of their directions) and writes the max.  A
//      receiver with one in-tile donor needs neither: the walk that reaches it is the last,
//      and carries the pair in a register.  Then the tile's 252 perimeter slots:
//      the local pair of each exit cell (a cell whose receiver lies in a neighbouring tile),
//      its step and the slot it drains into, and for every perimeter cell the exit its
//      in-tile path reaches and the steps of that path (pointer jumping with the two counts
//      riding along, in place: every word always says "my pointer is that many steps down my
//      path", whichever of its versions a reader meets).
//   B1 (upstream_forest_degree_kernel) the exit forest: node = exit cell e, next(e) = the exit
//      that the cell p it drains into reaches in p's tile, offset(e) = step(e) + path(p ->
//      next(e)); in-degrees by global atomics.
//   B2 (upstream_forest_walk_kernel)  the last-donor walk over the forest.  A hop is a CAS
//      loop word[next] = max(word[next], value + offset) with the exact order, then a
//      returning add on next's arrival counter; the walk whose add completes the node reads
//      the final word and goes on.  Every access to a word or a counter that another
//      workgroup writes in this launch is an agent-scope atomic (8-byte words, atomics on both
//      sides: no fences), and each waits for the value the one before it returned.
//   C  (upstream_tile_kernel<true>)   A's walk again with each perimeter cell seeded with the
//      max over the halo exits that drain into it of their final forest pair + step; writes
//      the wanted outputs.  Also counts what never completed (a cycle).
// Every walk step completes one arrival on one node, so every loop is bounded by the nodes it
// completes (and, explicitly, by the node count); a CAS can only fail because another donor's
// succeeded, so its retries are capped by the node's in-degree.
// Workspace: 36 B per perimeter slot (2.2 B per cell) from the context's arena.
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per forest workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each)
constexpr int HS = TS + 2;            // staged tile with its one-cell halo
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile
constexpr uint16_t TERM = 0xFFFF;     // rl[]: terminal (code 0, leaves the raster, invalid, outside)
constexpr uint16_t RL_CELL = 0x0FFF;  // rl[]: the receiver's local index ...
constexpr uint16_t RL_DIAG = 0x1000;  // ... and whether the step to it is diagonal
constexpr uint64_t CARD = 1ull << 32; // one cardinal step of a pair; a diagonal one is 1

struct upstream_counters {
    unsigned long long exits;         // exit-forest nodes
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells whose in-tile donors never all arrived
    unsigned long long stuck_exits;   // forest nodes whose donors never all arrived
    unsigned long long heads;         // cells without a donor
    unsigned long long capped;        // forest hops whose CAS loop reached its cap
    int max_hops;                     // longest B2 walk
};

// p > q as lengths: (a1 - a2) + (b1 - b2) * sqrt(2) > 0, in integers.  SMALL: both pairs are
// paths inside a tile (components below 2^12), and 32-bit products do.
template <bool SMALL>
__device__ __forceinline__ bool pair_longer(uint64_t p, uint64_t q)
{
    const int64_t da = (int64_t)(p >> 32) - (int64_t)(q >> 32);
    const int64_t db = (int64_t)(uint32_t)p - (int64_t)(uint32_t)q;
    if (da >= 0 && db >= 0) return (da | db) != 0;
    if (da <= 0 && db <= 0) return false;
    bool card_wins;
    if (SMALL) {
        const uint32_t a2 = (uint32_t)((int)da * (int)da), b2 = (uint32_t)((int)db * (int)db);
        card_wins = a2 > 2 * b2;
    } else {
        // mixed signs: da^2 against 2 db^2.  |da|, |db| < 2^32, so both squares fit 64 bits,
        // and 2 db^2 does unless db^2 >= 2^63, when it is the greater anyway.
        const uint64_t ua = (uint64_t)(da < 0 ? -da : da), ub = (uint64_t)(db < 0 ? -db : db);
        const uint64_t a2 = ua * ua, b2 = ub * ub;
        card_wins = b2 < (1ull << 63) && a2 > 2 * b2;
    }
    return da > 0 ? card_wins : !card_wins;
}
__device__ __forceinline__ uint64_t step_of(int b) { return (b & 1) ? 1ull : CARD; }
// a path inside a tile (at most 4096 steps with the crossing one): ncard << 16 | ndiag
__device__ __forceinline__ uint64_t pair_of_packed(uint32_t k)
{
    return ((uint64_t)(k >> 16) << 32) | (k & 0xFFFFu);
}

// the greatest of `best` and val[d] + step(d) over the in-tile donors d of cell r, which lie
// in the directions of mask m
template <bool SMALL>
__device__ __forceinline__ uint64_t donor_max(const uint64_t *val, int r, uint32_t m,
                                              uint64_t best)
{
    while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        const uint64_t cand = val[r - (code_dy(b) * TS + code_dx(b))] + step_of(b);
        if (pair_longer<SMALL>(cand, best)) best = cand;
    }
    return best;
}

template <bool FINAL>
__global__ __launch_bounds__(TNT) void upstream_tile_kernel(
    const uint8_t *__restrict__ d8, int H, int W, int tiles_x, uint32_t *__restrict__ out_nc,
    uint32_t *__restrict__ out_nd, float *__restrict__ out_len, double cs, double cs2,
    uint64_t *__restrict__ word, uint32_t *__restrict__ arr_b, uint32_t *__restrict__ indeg_b,
    int32_t *__restrict__ link, int32_t *__restrict__ tgt, uint32_t *__restrict__ pathw,
    uint32_t *__restrict__ off, upstream_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[HS * HS];
    __shared__ uint16_t rl[TC];
    __shared__ uint8_t dmask[TC];           // bit b: the neighbour against direction b is a donor
    __shared__ uint32_t arr[TC / 4];        // arrivals, a byte per cell (at most 8)
    __shared__ uint64_t val[TC];            // A: reused by the pointer jumping afterwards
    __shared__ unsigned int s_cnt[4];       // invalid codes, stuck cells, stuck exits, heads

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const int64_t base = tile.base;

    if (tid < 4) s_cnt[tid] = 0;
    for (int i = tid; i < TC / 4; i += TNT) arr[i] = 0;
    for (int i = tid; i < HS * HS; i += TNT) {
        const int gy = y0 + i / HS - 1, gx = x0 + i % HS - 1;
        code[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? d8[(size_t)gy * W + gx] : 0;
    }
    __syncthreads();

    // receivers, in-tile donors (gathered: the neighbours whose code points here) and seeds:
    // (0, 0), in C the greatest final forest pair + step of the halo exits draining here
    unsigned int bad = 0, heads = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) {
            rl[i] = TERM;
            dmask[i] = 0;
            continue;
        }
        const d8_step s = d8_decode(code[(ly + 1) * HS + lx + 1], ly, lx, tile, H, W);
        if (s.invalid) ++bad;
        rl[i] = s.terminal ? TERM
                : s.in_tile() ? (uint16_t)((s.ny * TS + s.nx) | ((s.b & 1) ? RL_DIAG : 0)) : EXIT;
        uint32_t mask = 0;
        int halo = 0;
        uint64_t seed = 0;
        for (int b = 0; b < 8; ++b) {
            const int ny = ly - code_dy(b), nx = lx - code_dx(b);   // a donor in direction b
            if (code[(ny + 1) * HS + nx + 1] != (1 << b)) continue;
            if (ny >= 0 && ny < TS && nx >= 0 && nx < TS) {
                mask |= 1u << b;
            } else {
                ++halo;
                if (FINAL) {
                    const uint64_t cand = word[slot_of(tile, tiles_x, ny, nx)] + step_of(b);
                    if (pair_longer<false>(cand, seed)) seed = cand;
                }
            }
        }
        dmask[i] = (uint8_t)mask;
        val[i] = seed;
        heads += mask == 0 && halo == 0;
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (FINAL && heads) atomicAdd(&s_cnt[3], heads);
    __syncthreads();

    // last donor continues: a walk starts at each cell without in-tile donors, whose seed is
    // its final pair, and carries the pair of the cell it stands on, which is stored.  A
    // receiver with one in-tile donor is completed by whoever reaches it.  At any other the
    // walk arrives (release: its pair is stored; acquire: the other donors' are) and goes on
    // only if its arrival completed the receiver, whose pair it then gathers.  Leaf status
    // and completion come from dmask[] alone.
    for (int i = tid; i < TC; i += TNT) {
        if (dmask[i] != 0) continue;
        uint64_t v = val[i];
        uint16_t e = rl[i];
        for (int step = 0; step < TC && e < EXIT; ++step) {
            const int r = e & RL_CELL;
            const int shift = 8 * (r & 3);
            const uint32_t m = dmask[r];
            const uint16_t next = rl[r];
            // r's seed stays as it is until the arrival that completes r: read with the rest
            const uint64_t seed = FINAL ? val[r] : 0ull;
            if ((m & (m - 1)) == 0) {
                const uint64_t cand = v + ((e & RL_DIAG) ? 1ull : CARD);
                v = !FINAL || pair_longer<false>(cand, seed) ? cand : seed;
                __hip_atomic_fetch_add(&arr[r >> 2], 1u << shift, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                const uint32_t old = __hip_atomic_fetch_add(&arr[r >> 2], 1u << shift,
                                                            __ATOMIC_ACQ_REL,
                                                            __HIP_MEMORY_SCOPE_WORKGROUP);
                if (((old >> shift) & 0xFFu) + 1 != (uint32_t)__builtin_popcount(m)) break;
                v = donor_max<!FINAL>(val, r, m, seed);
            }
            val[r] = v;
            e = next;
        }
    }
    __syncthreads();

    if (FINAL) {
        unsigned int stuck = 0;
        for (int i = tid; i < TC; i += TNT) {
            const int ly = i / TS, lx = i % TS;
            if (!tile.inside(ly, lx)) continue;
            if (((arr[i >> 2] >> (8 * (i & 3))) & 0xFFu) != (uint32_t)__builtin_popcount(dmask[i]))
                ++stuck;
            const uint64_t v = val[i];
            const uint32_t nc = (uint32_t)(v >> 32), nd = (uint32_t)v;
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            if (out_nc) out_nc[g] = nc;
            if (out_nd) out_nd[g] = nd;
            if (out_len)
                out_len[g] = __double2float_rn(__dadd_rn(__dmul_rn((double)nc, cs),
                                                         __dmul_rn((double)nd, cs2)));
        }
        unsigned int stuck_b = 0;
        if (tid < PER && tgt[base + tid] >= 0 && arr_b[base + tid] != indeg_b[base + tid])
            ++stuck_b;
        if (stuck) atomicAdd(&s_cnt[1], stuck);
        if (stuck_b) atomicAdd(&s_cnt[2], stuck_b);
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[1]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[1]);
            if (s_cnt[2]) atomicAdd(&cnt->stuck_exits, (unsigned long long)s_cnt[2]);
            if (s_cnt[3]) atomicAdd(&cnt->heads, (unsigned long long)s_cnt[3]);
        }
        return;
    }

    // A: the perimeter slots -- each exit's local pair, its step and the slot it drains into
    int p_ly = 0, p_lx = 0, p_cell = 0;
    bool p_in = false;
    if (tid < PER) {
        perim_cell(tid, p_ly, p_lx);
        p_cell = p_ly * TS + p_lx;
        p_in = tile.inside(p_ly, p_lx);
        const bool is_exit = p_in && rl[p_cell] == EXIT;
        int32_t to = -1;
        uint32_t step = 0;
        if (is_exit) {
            const int b = __builtin_ctz(code[(p_ly + 1) * HS + p_lx + 1]);
            to = (int32_t)slot_of(tile, tiles_x, p_ly + code_dy(b), p_lx + code_dx(b));
            step = (b & 1) ? 1u : 1u << 16;
        }
        word[base + tid] = is_exit ? val[p_cell] : 0ull;
        arr_b[base + tid] = 0;
        indeg_b[base + tid] = 0;
        tgt[base + tid] = to;
        off[base + tid] = step;
    }
    __syncthreads();

    // pointer jumping in place: jmp[c] = the cell 2^k steps down c's in-tile path (an exit
    // points at itself, TERM when the path ends in the tile) | ncard << 16 | ndiag << 32 of
    // those steps.  Paths are shorter than 2^12 cells.  A word is read and written whole.
    uint64_t *jmp = val;
    for (int i = tid; i < TC; i += TNT) {
        const uint16_t r = rl[i];
        uint64_t w = r;
        if (r == EXIT) w = (uint64_t)i;
        else if (r != TERM) w = (uint64_t)(r & RL_CELL) | ((r & RL_DIAG) ? 1ull << 32 : 1ull << 16);
        jmp[i] = w;
    }
    __syncthreads();
    // (whether a round changed anything goes through three of the counters in turn, zero so
    // far in A: the one a round sets was last read two barriers ago)
    for (int round = 0; round < DOUBLINGS; ++round) {
        unsigned int *any = &s_cnt[1 + round % 3];
        if (tid == 0) s_cnt[1 + (round + 1) % 3] = 0;
        int changed = 0;
        for (int i = tid; i < TC; i += TNT) {
            const uint64_t a = __hip_atomic_load(&jmp[i], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t pa = (uint32_t)a & 0xFFFFu;
            if (pa == TERM) continue;
            const uint64_t b = __hip_atomic_load(&jmp[pa], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t pb = (uint32_t)b & 0xFFFFu;
            if (pb == pa) continue;                       // an exit: the end of the path
            __hip_atomic_store(&jmp[i], (a & ~0xFFFFull) + b, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
            changed = 1;
        }
        if (changed) __hip_atomic_store(any, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (!__hip_atomic_load(any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
    }
    if (tid < PER) {
        int32_t l = -1;
        uint32_t path = 0;
        if (p_in) {
            const uint64_t w = jmp[p_cell];
            const uint16_t e = (uint16_t)(w & 0xFFFFu);
            if (e != TERM && rl[e] == EXIT) {
                l = (int32_t)(base + perim_pos(e / TS, e % TS));
                path = ((uint32_t)(w >> 16) & 0xFFFFu) << 16 | ((uint32_t)(w >> 32) & 0xFFFFu);
            }
        }
        link[base + tid] = l;
        pathw[base + tid] = path;
    }
    if (tid == 0 && s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
}

// B1: next(e) of every exit node (the exit its receiver's in-tile path reaches, -1 when that
// path ends in a terminal cell), its offset and the forest in-degrees.  Grid-stride, so that
// the node count costs one global atomic per workgroup.
__global__ __launch_bounds__(NT) void upstream_forest_degree_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ link,
    const uint32_t *__restrict__ pathw, int32_t *__restrict__ next, uint32_t *__restrict__ off,
    uint32_t *__restrict__ indeg_b, upstream_counters *__restrict__ cnt)
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
            if (n >= 0) {
                atomicAdd(&indeg_b[n], 1u);
                off[s] += pathw[to];                     // 16-bit halves, each at most 4096
            }
        }
        next[s] = n;
    }
    if (exits) atomicAdd(&s_exits, exits);
    __syncthreads();
    if (threadIdx.x == 0 && s_exits) atomicAdd(&cnt->exits, (unsigned long long)s_exits);
}

__device__ __forceinline__ uint64_t word_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// B2: last-donor walks over the exit forest.  A node's final pair is its word once its
// arrivals equal its in-degree.
__global__ __launch_bounds__(NT) void upstream_forest_walk_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ next,
    const uint32_t *__restrict__ off, const uint32_t *__restrict__ indeg_b, uint64_t *word,
    uint32_t *arr_b, upstream_counters *__restrict__ cnt)
{
    __shared__ int s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    int hops = 0;
    if (s < nslots && tgt[s] >= 0 && indeg_b[s] == 0) {
        int64_t e = s;
        uint64_t v = word_load(&word[e]);
        for (int64_t step = 0; step < nslots; ++step) {
            const int32_t t = next[e];
            if (t < 0) break;
            const uint32_t need = indeg_b[t];
            const uint64_t cand = v + pair_of_packed(off[e]);
            // a CAS fails only because another donor's succeeded: fewer than `need` times
            uint64_t cur = word_load(&word[t]);
            uint32_t tries = 0;
            bool capped = false;
            while (pair_longer<false>(cand, cur)) {
                if (tries++ > need) { capped = true; break; }
                if (__hip_atomic_compare_exchange_strong(&word[t], &cur, cand, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT))
                    break;
            }
            if (capped) {
                atomicAdd(&cnt->capped, 1ull);
                break;
            }
            // the add is issued once the CAS has returned, the load once the add has
            asm volatile("" ::: "memory");
            const uint32_t old = __hip_atomic_fetch_add(&arr_b[t], 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            ++hops;
            if (old + 1 != need) break;
            asm volatile("" ::: "memory");
            v = word_load(&word[t]);
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

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const uint8_t *d8, int H, int W, double cellsize,
               const uint32_t *ncard, const uint32_t *ndiag, const float *length, int flags,
               const hdem_upstream_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, d8, d8, H, W)) return rc;
    if (int rc = d8_grid_of("upstream flow length", H, W, g)) return rc;
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "unknown upstream flow length flags 0x%x", flags);
    HDEM_REQUIRE(ncard || ndiag || length, HDEM_ERR_BAD_ARG,
                 "no output wanted: give at least one of ncard, ndiag, length");
    HDEM_REQUIRE(std::isfinite(cellsize) && cellsize > 0.0, HDEM_ERR_BAD_ARG,
                 "cellsize must be finite and positive, got %g", cellsize);
    return d8_check_stats(stats, "hdem_upstream_stats");
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_upstream_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                    double cellsize, uint32_t *ncard, uint32_t *ndiag,
                                    float *length, int flags, hdem_upstream_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, cellsize, ncard, ndiag, length, flags, stats, &g))
        return rc;
    const int64_t tiles = g.tiles, nslots = g.nslots;
    const int tiles_x = g.tiles_x;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_upstream_stats st = {};
    d8_publish(stats, st);

    // arena: counters | word u64 | arr_b u32 | indeg_b u32 | link i32 | tgt i32 | next i32 |
    // pathw u32 | off u32  (per slot)
    const size_t head = 256;
    static_assert(sizeof(upstream_counters) <= head, "counters outgrew their block");
    const size_t bytes = head + (size_t)nslots * (8 + 7 * 4);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    upstream_counters *cnt = reinterpret_cast<upstream_counters *>(ws);
    uint64_t *word = reinterpret_cast<uint64_t *>(ws + head);
    uint32_t *arr_b = reinterpret_cast<uint32_t *>(word + nslots);
    uint32_t *indeg_b = arr_b + nslots;
    int32_t *link = reinterpret_cast<int32_t *>(indeg_b + nslots);
    int32_t *tgt = link + nslots;
    int32_t *next = tgt + nslots;
    uint32_t *pathw = reinterpret_cast<uint32_t *>(next + nslots);
    uint32_t *off = pathw + nslots;

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(upstream_counters), ctx->stream));
    const int64_t forest_blocks = (nslots + NT - 1) / NT;
    const int degree_blocks = (int)std::min<int64_t>(forest_blocks, (int64_t)ctx->num_cus * 8);
    const double cs2 = cellsize * std::sqrt(2.0);
    phases.mark(0);
    hipLaunchKernelGGL(upstream_tile_kernel<false>, dim3((unsigned)tiles), dim3(TNT), 0,
                       ctx->stream, d8, H, W, tiles_x, ncard, ndiag, length, cellsize, cs2, word,
                       arr_b, indeg_b, link, tgt, pathw, off, cnt);
    phases.mark(1);
    hipLaunchKernelGGL(upstream_forest_degree_kernel, dim3(degree_blocks), dim3(NT), 0,
                       ctx->stream, nslots, tgt, link, pathw, next, off, indeg_b, cnt);
    hipLaunchKernelGGL(upstream_forest_walk_kernel, dim3((unsigned)forest_blocks), dim3(NT), 0,
                       ctx->stream, nslots, tgt, next, off, indeg_b, word, arr_b, cnt);
    phases.mark(2);
    hipLaunchKernelGGL(upstream_tile_kernel<true>, dim3((unsigned)tiles), dim3(TNT), 0,
                       ctx->stream, d8, H, W, tiles_x, ncard, ndiag, length, cellsize, cs2, word,
                       arr_b, indeg_b, link, tgt, pathw, off, cnt);
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    upstream_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.max_hops = host.max_hops;
    st.exits = (int64_t)host.exits;
    st.heads = (int64_t)host.heads;
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_tile, &st.ms_forest, &st.ms_final);
    d8_publish(stats, st);
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.capped, HDEM_ERR_NOT_CONVERGED,
                 "upstream flow length: %llu forest hops gave up their compare-and-swap",
                 host.capped);
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_exits, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never drain (%llu of them inside "
                 "tiles, %llu tile exits)",
                 host.stuck_cells + host.stuck_exits, host.stuck_cells, host.stuck_exits);
    return HDEM_OK;
}

extern "C" int hdem_upstream_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, double cellsize,
                                uint32_t *ncard, uint32_t *ndiag, float *length, int flags,
                                hdem_upstream_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, cellsize, ncard, ndiag, length, flags, stats, &g))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dout[3];
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    void *const host_out[3] = {ncard, ndiag, length};
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, n * 4)) return rc;
    const int rc = hdem_upstream_u8_dev(ctx, dd8.as<const uint8_t>(), H, W, cellsize,
                                        dout[0].as<uint32_t>(), dout[1].as<uint32_t>(),
                                        dout[2].as<float>(), flags, stats);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc2 = dout[k].download(host_out[k], n * 4)) return rc2;
    return HDEM_OK;
}
