// Upstream D8 extremes and depression breaching (new operators; UpstreamExtreme,
// BreachDepressions).
//
// E[c] = best(v[c], E[d] over the neighbours d whose code points at c): the least (min mode) or
// greatest (max mode) present value over every cell whose D8 path passes through c, c included,
// and the cell that holds it.  One 64-bit word per cell makes value and holder one reduction:
//   min mode  key << 32 |  index   reduced by unsigned min, identity all ones
//   max mode  key << 32 | ~index   reduced by unsigned max, identity 0
// key is key_of(f) for a float32 (a NaN is absent: its word is the identity) and the value itself
// for a uint32, so among equal keys the smallest flat index wins in both modes.  Neither identity
// is a real cell: a NaN has no key and indices stop at 2^32 - 2.  min and max are idempotent,
// commutative and associative on a total order: the result is the same whatever order the
// reductions land in.  The codes, what makes a cell terminal, the tiles and their perimeter slots
// are those of hdem_d8tile.h, and the scheme is hdem_flowsum.hip's with the reduction in place
// of the add: four launches whatever the length of the longest path, no workgroup ever waits on
// another.
//   A  (upext_tile_kernel<false>)  per 64 x 64 tile: the values are read as words, then "last
//      donor continues" walks over one 64-bit LDS word per cell.  Arrivals are flowsum's byte per
//      cell with the in-tile donor count in its high half: a walk reduces its word into its
//      receiver's (one non-returning LDS min / max), then makes one returning add on the
//      receiver's arrival counter (acquire / release at workgroup scope); the arrival that
//      completes the receiver reads the word and goes on.  A receiver with one in-tile donor
//      needs no atomic to return.  Then the tile's 252 perimeter slots: the local word of each
//      exit cell, the slot of the cell it drains into, and for every perimeter cell the exit its
//      in-tile path reaches.
//   B1 (upext_forest_degree_kernel) the exit forest: next(e) and the in-degrees.
//   B2 (upext_forest_walk_kernel)   the last-donor walk over the forest: a hop is an agent-scope
//      min / max on the node's word, then a returning add on its arrival counter that waits for
//      it; the walk whose add completes the node reads the word with an agent-scope atomic load
//      and goes on.  Words that another workgroup writes during the launch are touched only by
//      agent-scope atomics.
//   C  (upext_tile_kernel<true>)    A's walk again; the seed of a perimeter cell is reduced with
//      the final forest words of the halo exits that drain into it.  Writes the outputs from the
//      words (extreme, where; or carved, source) and counts what never completed.
// Breaching is the min-mode call over a float32 seed raster (the DEM at pits, NaN elsewhere)
// that a radius-1 stencil launch writes into the arena; C then compares with the DEM.
// Every walk step completes one arrival on one node, so every loop is bounded by the nodes it
// completes (and, explicitly, by the node count).
// Workspace: 28 B per perimeter slot (1.7 B per cell) from the context's arena; breaching adds
// the seed raster, 4 B per cell.
#include "hdem_d8tile.h"

namespace {

constexpr int NT = 256;               // threads per forest workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each)
constexpr int HS = TS + 2;            // staged tile with its one-cell halo
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile
constexpr uint16_t TERM = 0xFFFF;     // rl[]: terminal (code 0, leaves the raster, invalid, outside)
constexpr uint8_t OUTSIDE = 0xFF;     // arr[]: cell of a partial tile beyond the raster
constexpr uint32_t QUIET_NAN = 0x7FC00000u;
constexpr uint32_t NOWHERE = 0xFFFFFFFFu;
constexpr int PIT_BX = TS, PIT_BY = 4;   // the pit stencil's workgroup: four waves, a row each

struct upext_counters {
    unsigned long long exits;         // exit-forest nodes
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells whose in-tile donors never all arrived
    unsigned long long stuck_exits;   // forest nodes whose donors never all arrived
    unsigned long long absent;        // NaN values
    unsigned long long pits;          // breaching: cells of the seed raster that are present
    unsigned long long lowered;       // breaching: cells written below the DEM
    int max_hops;                     // longest B2 walk
};

enum { C_BAD, C_STUCK, C_STUCK_B, C_ABSENT, C_LOWERED, C_COUNT };

template <int MODE>
__device__ __forceinline__ constexpr uint64_t identity()
{
    return MODE == HDEM_UPEXT_MIN ? ~0ull : 0ull;
}
template <int MODE>
__device__ __forceinline__ uint64_t best(uint64_t a, uint64_t b)
{
    return MODE == HDEM_UPEXT_MIN ? (a < b ? a : b) : (a > b ? a : b);
}
// the word of cell g holding the 32 value bits raw: the identity for a float32 NaN
template <int MODE>
__device__ __forceinline__ uint64_t word_of(uint32_t raw, int value_type, uint32_t g,
                                            unsigned int &absent)
{
    uint32_t key = raw;
    if (value_type == HDEM_UPEXT_F32) {
        if ((raw & 0x7FFFFFFFu) > 0x7F800000u) { ++absent; return identity<MODE>(); }
        key = key_of(__uint_as_float(raw));
    }
    return (uint64_t)key << 32 | (MODE == HDEM_UPEXT_MIN ? g : ~g);
}
template <int MODE>
__device__ __forceinline__ uint32_t holder_of(uint64_t w)
{
    return MODE == HDEM_UPEXT_MIN ? (uint32_t)w : ~(uint32_t)w;
}

// arr[]: a byte per cell in 32-bit words, in-tile donors << 4 | arrivals (at most 8 each), so
// that what an arrival's add returns says whether it completed the cell
__device__ __forceinline__ uint32_t arr_byte(const uint32_t *arr, int i)
{
    return (__hip_atomic_load(&arr[i >> 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >>
            (8 * (i & 3))) & 0xFFu;
}

template <int MODE>
__device__ __forceinline__ void lds_reduce(uint64_t *p, uint64_t v)
{
    if (MODE == HDEM_UPEXT_MIN)
        (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// dem: breaching's C alone, where out_extreme is carved and out_where is source
template <bool FINAL, int MODE>
__global__ __launch_bounds__(TNT) void upext_tile_kernel(
    const uint8_t *__restrict__ d8, int H, int W, int tiles_x, const uint32_t *__restrict__ values,
    int value_type, const uint32_t *__restrict__ dem, uint32_t *__restrict__ out_extreme,
    uint32_t *__restrict__ out_where, uint64_t *__restrict__ word, uint32_t *__restrict__ arr_b,
    uint32_t *__restrict__ indeg_b, int32_t *__restrict__ link, int32_t *__restrict__ tgt,
    upext_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[HS * HS];
    __shared__ uint16_t rl[TC];
    __shared__ uint32_t arr[TC / 4];        // donors << 4 | arrivals, a byte per cell
    __shared__ uint64_t val[TC];            // A: reused by the pointer jumping afterwards
    __shared__ unsigned int s_cnt[C_COUNT];

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const int64_t base = tile.base;

    if (tid < C_COUNT) s_cnt[tid] = 0;
    for (int i = tid; i < HS * HS; i += TNT) {
        const int gy = y0 + i / HS - 1, gx = x0 + i % HS - 1;
        code[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? d8[(size_t)gy * W + gx] : 0;
    }
    __syncthreads();

    // receivers, in-tile in-degrees (gathered: the neighbours whose code points here) and
    // seeds: the cell's own word, reduced in C with the final forest words of the halo exits
    // that drain here
    unsigned int bad = 0, absent = 0;
    uint8_t *arr_bytes = reinterpret_cast<uint8_t *>(arr);
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) {
            rl[i] = TERM;
            arr_bytes[i] = OUTSIDE;
            continue;
        }
        const d8_step s = d8_decode(code[(ly + 1) * HS + lx + 1], ly, lx, tile, H, W);
        if (s.invalid) ++bad;
        rl[i] = s.terminal ? TERM : s.in_tile() ? (uint16_t)(s.ny * TS + s.nx) : EXIT;
        int deg = 0;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        uint64_t seed = word_of<MODE>(values[g], value_type, (uint32_t)g, absent);
        for (int b = 0; b < 8; ++b) {
            const int ny = ly - code_dy(b), nx = lx - code_dx(b);   // a donor in direction b
            if (code[(ny + 1) * HS + nx + 1] != (1 << b)) continue;
            if (ny >= 0 && ny < TS && nx >= 0 && nx < TS) ++deg;
            else if (FINAL) seed = best<MODE>(seed, word[slot_of(tile, tiles_x, ny, nx)]);
        }
        arr_bytes[i] = (uint8_t)(deg << 4);
        val[i] = seed;
    }
    if (!FINAL) {       // A counts: C reads the same values again
        if (bad) atomicAdd(&s_cnt[C_BAD], bad);
        if (absent) atomicAdd(&s_cnt[C_ABSENT], absent);
    }
    __syncthreads();

    // last donor continues: a walk starts at each cell without in-tile donors, whose seed is
    // its final word, and carries the word of the cell it stands on.  A receiver with one
    // in-tile donor is completed by whoever reaches it: the walk reduces the receiver's seed in
    // a register and stores the word.  At any other the walk reduces its word into the
    // receiver's, then arrives (release: its reduction is done; acquire: the other donors' are)
    // and goes on only if its arrival completed the receiver, whose word it then reads.  Leaf
    // status and completion come from arr[] alone.
    for (int i = tid; i < TC; i += TNT) {
        if (arr_byte(arr, i) >> 4) continue;        // (OUTSIDE too)
        uint64_t v = val[i];
        uint16_t r = rl[i];
        for (int step = 0; step < TC && r < EXIT; ++step) {
            const int shift = 8 * (r & 3);
            const uint32_t need = arr_byte(arr, r) >> 4;
            const uint16_t next = rl[r];
            if (need == 1) {
                v = best<MODE>(v, val[r]);
                val[r] = v;
                __hip_atomic_fetch_add(&arr[r >> 2], 1u << shift, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                lds_reduce<MODE>(&val[r], v);
                const uint32_t old = __hip_atomic_fetch_add(&arr[r >> 2], 1u << shift,
                                                            __ATOMIC_ACQ_REL,
                                                            __HIP_MEMORY_SCOPE_WORKGROUP);
                if (((old >> shift) & 0xFu) + 1 != need) break;
                v = __hip_atomic_load(&val[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            r = next;
        }
    }
    __syncthreads();

    if (FINAL) {
        // the outputs, from LDS row by row: a wave writes one row of the tile
        unsigned int stuck = 0, lowered = 0;
        for (int i = tid; i < TC; i += TNT) {
            const int ly = i / TS, lx = i % TS;
            const uint32_t a = arr_byte(arr, i);
            if (a == OUTSIDE) continue;
            if ((a & 0xFu) != a >> 4) ++stuck;
            const uint64_t w = val[i];
            const bool present = w != identity<MODE>();
            const uint32_t key = (uint32_t)(w >> 32);
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            if (dem) {
                const uint32_t z = dem[g];      // kept bit for bit, NaN payloads included
                const float t = float_of(key);
                const bool lower = present && t < __uint_as_float(z);
                if (lower) ++lowered;
                out_extreme[g] = lower ? __float_as_uint(t) : z;
                if (out_where) out_where[g] = lower ? holder_of<MODE>(w) : NOWHERE;
                continue;
            }
            if (out_extreme)
                out_extreme[g] = value_type != HDEM_UPEXT_F32 ? key
                                 : present ? __float_as_uint(float_of(key)) : QUIET_NAN;
            if (out_where) out_where[g] = present ? holder_of<MODE>(w) : NOWHERE;
        }
        unsigned int stuck_b = 0;
        if (tid < PER && tgt[base + tid] >= 0 && arr_b[base + tid] != indeg_b[base + tid])
            ++stuck_b;
        if (stuck) atomicAdd(&s_cnt[C_STUCK], stuck);
        if (stuck_b) atomicAdd(&s_cnt[C_STUCK_B], stuck_b);
        if (lowered) atomicAdd(&s_cnt[C_LOWERED], lowered);
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[C_STUCK]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[C_STUCK]);
            if (s_cnt[C_STUCK_B]) atomicAdd(&cnt->stuck_exits, (unsigned long long)s_cnt[C_STUCK_B]);
            if (s_cnt[C_LOWERED]) atomicAdd(&cnt->lowered, (unsigned long long)s_cnt[C_LOWERED]);
        }
        return;
    }

    // A: the perimeter slots -- each exit's local word and the slot it drains into
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
        word[base + tid] = is_exit ? val[p_cell] : identity<MODE>();
        arr_b[base + tid] = 0;
        indeg_b[base + tid] = 0;
        tgt[base + tid] = to;
    }
    __syncthreads();

    // pointer jumping: jmp[c] -> the exit c's in-tile path reaches (an exit points at
    // itself), TERM when it ends in the tile.  Paths are shorter than 2^12 cells.
    uint16_t *jmp = reinterpret_cast<uint16_t *>(val);
    uint16_t *jnx = jmp + TC;
    for (int i = tid; i < TC; i += TNT) {
        const uint16_t r = rl[i];
        jmp[i] = r == EXIT ? (uint16_t)i : r;
    }
    __syncthreads();
    for (int round = 0; round < DOUBLINGS; ++round) {
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
    if (tid == 0) {
        if (s_cnt[C_BAD]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[C_BAD]);
        if (s_cnt[C_ABSENT]) atomicAdd(&cnt->absent, (unsigned long long)s_cnt[C_ABSENT]);
    }
}

// B1: next(e) of every exit node (the exit its receiver's in-tile path reaches, -1 when that
// path ends in a terminal cell) and the forest in-degrees.  Grid-stride, so that the node
// count costs one global atomic per workgroup.
__global__ __launch_bounds__(NT) void upext_forest_degree_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ link,
    int32_t *__restrict__ next, uint32_t *__restrict__ indeg_b, upext_counters *__restrict__ cnt)
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

// B2: last-donor walks over the exit forest.  A node's final word is its word once its
// arrivals equal its in-degree.
template <int MODE>
__global__ __launch_bounds__(NT) void upext_forest_walk_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ next,
    const uint32_t *__restrict__ indeg_b, uint64_t *word, uint32_t *arr_b,
    upext_counters *__restrict__ cnt)
{
    __shared__ int s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    int hops = 0;
    if (s < nslots && tgt[s] >= 0 && indeg_b[s] == 0) {
        int64_t e = s;
        uint64_t v = __hip_atomic_load(&word[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int64_t step = 0; step < nslots; ++step) {
            const int32_t t = next[e];
            if (t < 0) break;
            const uint32_t need = indeg_b[t];
            const uint64_t before =
                MODE == HDEM_UPEXT_MIN
                    ? __hip_atomic_fetch_min(&word[t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                    : __hip_atomic_fetch_max(&word[t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // no bit of what the reduction returns is known, so the arrival's operand is tied
            // to it by hand: the arrival is issued once the reduction has returned, the load
            // once the arrival has
            uint32_t one = 1u;
            asm volatile("" : "+v"(one) : "v"((uint32_t)before), "v"((uint32_t)(before >> 32)));
            const uint32_t old = __hip_atomic_fetch_add(&arr_b[t], one, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            ++hops;
            if (old + 1 != need) break;
            asm volatile("" ::: "memory");
            v = __hip_atomic_load(&word[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// Breaching's seeds: the DEM at pits, the quiet NaN elsewhere.  A pit is a non-NaN cell off the
// raster's one-cell ring with no NaN neighbour and no strictly lower one.  A workgroup takes the
// 64 x 64 cells of a tile, a wave a row at a time, so that the pit count costs one global atomic
// per tile.
__global__ __launch_bounds__(PIT_BX * PIT_BY) void upext_pit_seed_kernel(
    const float *__restrict__ dem, int H, int W, int tiles_x, uint32_t *__restrict__ seed,
    upext_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_pits;
    if (threadIdx.x == 0 && threadIdx.y == 0) s_pits = 0;
    __syncthreads();
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int x = tile.x0 + threadIdx.x;
    const int y_end = tile.y0 + tile.th;
    unsigned int pits = 0;
    for (int y = tile.y0 + threadIdx.y; x < W && y < y_end; y += PIT_BY) {
        const int64_t g = (int64_t)y * W + x;
        const float z = dem[g];
        bool pit = z == z && y > 0 && y < H - 1 && x > 0 && x < W - 1;
        if (pit) {
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const float n = dem[g + (int64_t)dy * W + dx];
                    if (n != n || n < z) pit = false;
                }
        }
        seed[g] = pit ? __float_as_uint(z) : QUIET_NAN;
        if (pit) ++pits;
    }
    for (int m = 32; m >= 1; m >>= 1) pits += __shfl_xor(pits, m);
    if (threadIdx.x == 0 && pits) atomicAdd(&s_pits, pits);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && s_pits)
        atomicAdd(&cnt->pits, (unsigned long long)s_pits);
}

// One call of either operator.  Breaching: values is null (the seeds are the call's own), dem is
// the DEM, extreme is carved and where is source.
struct upext_call {
    const char *op;
    const uint8_t *d8;
    int H, W;
    const void *values;
    int value_type, mode;
    const float *dem;
    void *extreme;
    uint32_t *where;
};

struct span {
    const char *name;
    uintptr_t lo, hi;
};

int check_spans(const char *op, const span *in, int n_in, const span *outs, int n_out)
{
    span s[5];
    int ns = 0;
    for (int j = 0; j < n_in; ++j) s[ns++] = in[j];
    for (int k = 0; k < n_out; ++k) {
        const span &o = outs[k];
        if (!o.lo) continue;
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "%s: %s overlaps %s", op, o.name, s[j].name);
        s[ns++] = o;
    }
    return HDEM_OK;
}

// also the tile grid: nothing is allocated for a raster that is refused
int check_extreme_args(const hdem_ctx *ctx, const upext_call &a, const hdem_upextreme_stats *stats,
                       d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, a.d8, a.d8, a.H, a.W)) return rc;
    if (int rc = d8_grid_of(a.op, a.H, a.W, g)) return rc;
    HDEM_REQUIRE(a.values, HDEM_ERR_BAD_ARG, "the value raster is null");
    HDEM_REQUIRE(a.value_type == HDEM_UPEXT_F32 || a.value_type == HDEM_UPEXT_U32,
                 HDEM_ERR_BAD_ARG, "unknown value type %d", a.value_type);
    HDEM_REQUIRE(a.mode == HDEM_UPEXT_MIN || a.mode == HDEM_UPEXT_MAX, HDEM_ERR_BAD_ARG,
                 "unknown mode %d", a.mode);
    HDEM_REQUIRE(a.extreme || a.where, HDEM_ERR_BAD_ARG,
                 "no output wanted: give at least one of extreme, where");
    if (int rc = d8_check_stats(stats, "hdem_upextreme_stats")) return rc;
    const size_t n = (size_t)a.H * a.W;
    const span in[2] = {{"d8", (uintptr_t)a.d8, (uintptr_t)a.d8 + n},
                        {"values", (uintptr_t)a.values, (uintptr_t)a.values + 4 * n}};
    const span outs[2] = {{"extreme", (uintptr_t)a.extreme, (uintptr_t)a.extreme + 4 * n},
                          {"where", (uintptr_t)a.where, (uintptr_t)a.where + 4 * n}};
    return check_spans(a.op, in, 2, outs, 2);
}

int check_breach_args(const hdem_ctx *ctx, const upext_call &a, const hdem_breach_stats *stats,
                      d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, a.dem, a.extreme, a.H, a.W)) return rc;
    if (int rc = d8_grid_of(a.op, a.H, a.W, g)) return rc;
    HDEM_REQUIRE(a.d8, HDEM_ERR_BAD_ARG, "the code raster is null");
    if (int rc = d8_check_stats(stats, "hdem_breach_stats")) return rc;
    const size_t n = (size_t)a.H * a.W;
    const span in[2] = {{"dem", (uintptr_t)a.dem, (uintptr_t)a.dem + 4 * n},
                        {"d8", (uintptr_t)a.d8, (uintptr_t)a.d8 + n}};
    const span outs[2] = {{"carved", (uintptr_t)a.extreme, (uintptr_t)a.extreme + 4 * n},
                          {"source", (uintptr_t)a.where, (uintptr_t)a.where + 4 * n}};
    return check_spans(a.op, in, 2, outs, 2);
}

struct upext_views {
    uint64_t *word;
    uint32_t *arr_b, *indeg_b;
    int32_t *link, *tgt, *next;
    upext_counters *cnt;
};

template <bool FINAL, int MODE>
void launch_tile(hdem_ctx *ctx, const upext_call &a, const d8_grid &g, const upext_views &v)
{
    hipLaunchKernelGGL((upext_tile_kernel<FINAL, MODE>), dim3((unsigned)g.tiles), dim3(TNT), 0,
                       ctx->stream, a.d8, a.H, a.W, g.tiles_x,
                       static_cast<const uint32_t *>(a.values), a.value_type,
                       FINAL ? reinterpret_cast<const uint32_t *>(a.dem) : nullptr,
                       static_cast<uint32_t *>(a.extreme), a.where, v.word, v.arr_b, v.indeg_b,
                       v.link, v.tgt, v.cnt);
}

template <int MODE>
void launch_all(hdem_ctx *ctx, const upext_call &a, const d8_grid &g, const upext_views &v,
                hdem_event_timer<4> &phases)
{
    const int64_t forest_blocks = (g.nslots + NT - 1) / NT;
    const int degree_blocks = (int)std::min<int64_t>(forest_blocks, (int64_t)ctx->num_cus * 8);
    launch_tile<false, MODE>(ctx, a, g, v);
    phases.mark(1);
    hipLaunchKernelGGL(upext_forest_degree_kernel, dim3(degree_blocks), dim3(NT), 0, ctx->stream,
                       g.nslots, v.tgt, v.link, v.next, v.indeg_b, v.cnt);
    hipLaunchKernelGGL(upext_forest_walk_kernel<MODE>, dim3((unsigned)forest_blocks), dim3(NT), 0,
                       ctx->stream, g.nslots, v.tgt, v.next, v.indeg_b, v.word, v.arr_b, v.cnt);
    phases.mark(2);
    launch_tile<true, MODE>(ctx, a, g, v);
    phases.mark(3);
}

// The launches of either operator.  st is the breach struct, which opens with the extreme's
// fields; host: the counters, for the refusals that follow the stats.  The pit stencil is timed
// with phase A.
int upext_launch(hdem_ctx *ctx, upext_call a, const d8_grid &g, bool profile,
                 hdem_breach_stats *st, upext_counters *host)
{
    const int64_t nslots = g.nslots;
    const size_t n = (size_t)a.H * a.W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));

    // arena: counters | word u64 | arr_b u32 | indeg_b u32 | link i32 | tgt i32 | next i32
    // (per slot) | breaching: seed u32 (per cell)
    const size_t head = 256;
    static_assert(sizeof(upext_counters) <= head, "counters outgrew their block");
    const size_t slots_bytes = hdem_round16((size_t)nslots * (8 + 5 * 4));
    const size_t bytes = head + slots_bytes + (a.dem ? 4 * n : 0);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    upext_views v;
    v.cnt = reinterpret_cast<upext_counters *>(ws);
    v.word = reinterpret_cast<uint64_t *>(ws + head);
    v.arr_b = reinterpret_cast<uint32_t *>(v.word + nslots);
    v.indeg_b = v.arr_b + nslots;
    v.link = reinterpret_cast<int32_t *>(v.indeg_b + nslots);
    v.tgt = v.link + nslots;
    v.next = v.tgt + nslots;
    uint32_t *seed = reinterpret_cast<uint32_t *>(ws + head + slots_bytes);

    hdem_event_timer<4> phases(ctx, profile);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(v.cnt, 0, sizeof(upext_counters), ctx->stream));
    phases.mark(0);
    if (a.dem) {
        hipLaunchKernelGGL(upext_pit_seed_kernel, dim3((unsigned)g.tiles), dim3(PIT_BX, PIT_BY),
                           0, ctx->stream, a.dem, a.H, a.W, g.tiles_x, seed, v.cnt);
        a.values = seed;
    }
    if (a.mode == HDEM_UPEXT_MIN) launch_all<HDEM_UPEXT_MIN>(ctx, a, g, v, phases);
    else launch_all<HDEM_UPEXT_MAX>(ctx, a, g, v, phases);
    HDEM_HIP_CHECK(hipGetLastError());
    HDEM_HIP_CHECK(hipMemcpyAsync(host, v.cnt, sizeof(*host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->max_hops = host->max_hops;
    st->exits = (int64_t)host->exits;
    st->absent = (int64_t)host->absent;
    st->tile_h = TS;
    st->tile_w = TS;
    st->pits = (int64_t)host->pits;
    st->lowered = (int64_t)host->lowered;
    phases.read(&st->ms_tile, &st->ms_forest, &st->ms_final);
    return HDEM_OK;
}

int upext_refusals(const upext_counters &host)
{
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_exits, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never drain (%llu of them inside "
                 "tiles, %llu tile exits)",
                 host.stuck_cells + host.stuck_exits, host.stuck_cells, host.stuck_exits);
    return HDEM_OK;
}

// the extreme's stats are the head of the breach's
static_assert(offsetof(hdem_breach_stats, pits) == sizeof(hdem_upextreme_stats),
              "hdem_breach_stats opens with hdem_upextreme_stats");

int extreme_dev(hdem_ctx *ctx, const upext_call &a, const d8_grid &g, hdem_upextreme_stats *stats)
{
    hdem_upextreme_stats head = {};
    d8_publish(stats, head);
    hdem_breach_stats st = {};
    upext_counters host = {};
    if (int rc = upext_launch(ctx, a, g, stats != nullptr, &st, &host)) return rc;
    memcpy(&head, &st, sizeof(head));
    d8_publish(stats, head);
    return upext_refusals(host);
}

int breach_dev(hdem_ctx *ctx, const upext_call &a, const d8_grid &g, hdem_breach_stats *stats)
{
    hdem_breach_stats st = {};
    d8_publish(stats, st);
    upext_counters host = {};
    if (int rc = upext_launch(ctx, a, g, stats != nullptr, &st, &host)) return rc;
    d8_publish(stats, st);
    return upext_refusals(host);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_upextreme_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                     const void *values, int value_type, int mode, void *extreme,
                                     uint32_t *where, hdem_upextreme_stats *stats)
{
    const upext_call a = {"upstream extreme", d8, H, W, values, value_type, mode, nullptr,
                          extreme, where};
    d8_grid g;
    if (int rc = check_extreme_args(ctx, a, stats, &g)) return rc;
    return extreme_dev(ctx, a, g, stats);
}

extern "C" int hdem_upextreme_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                 const void *values, int value_type, int mode, void *extreme,
                                 uint32_t *where, hdem_upextreme_stats *stats)
{
    upext_call a = {"upstream extreme", d8, H, W, values, value_type, mode, nullptr, extreme,
                    where};
    d8_grid g;
    if (int rc = check_extreme_args(ctx, a, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dvalues, dout[2];
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dvalues.upload(ctx, values, 4 * n)) return rc;
    void *const host_out[2] = {extreme, where};
    for (int k = 0; k < 2; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, 4 * n)) return rc;
    a.d8 = dd8.as<const uint8_t>();
    a.values = dvalues.p;
    a.extreme = dout[0].p, a.where = dout[1].as<uint32_t>();
    if (int rc = extreme_dev(ctx, a, g, stats)) return rc;
    for (int k = 0; k < 2; ++k)
        if (host_out[k])
            if (int rc = dout[k].download(host_out[k], 4 * n)) return rc;
    return HDEM_OK;
}

extern "C" int hdem_breach_f32_dev(hdem_ctx *ctx, const float *dem, const uint8_t *d8, int H,
                                   int W, float *carved, uint32_t *source,
                                   hdem_breach_stats *stats)
{
    const upext_call a = {"depression breaching", d8, H, W, nullptr, HDEM_UPEXT_F32,
                          HDEM_UPEXT_MIN, dem, carved, source};
    d8_grid g;
    if (int rc = check_breach_args(ctx, a, stats, &g)) return rc;
    return breach_dev(ctx, a, g, stats);
}

extern "C" int hdem_breach_f32(hdem_ctx *ctx, const float *dem, const uint8_t *d8, int H, int W,
                               float *carved, uint32_t *source, hdem_breach_stats *stats)
{
    upext_call a = {"depression breaching", d8, H, W, nullptr, HDEM_UPEXT_F32, HDEM_UPEXT_MIN,
                    dem, carved, source};
    d8_grid g;
    if (int rc = check_breach_args(ctx, a, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf ddem, dd8, dout[2];
    if (int rc = ddem.upload(ctx, dem, 4 * n)) return rc;
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    void *const host_out[2] = {carved, source};
    for (int k = 0; k < 2; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, 4 * n)) return rc;
    a.dem = ddem.as<const float>();
    a.d8 = dd8.as<const uint8_t>();
    a.extreme = dout[0].p, a.where = dout[1].as<uint32_t>();
    if (int rc = breach_dev(ctx, a, g, stats)) return rc;
    for (int k = 0; k < 2; ++k)
        if (host_out[k])
            if (int rc = dout[k].download(host_out[k], 4 * n)) return rc;
    return HDEM_OK;
}
