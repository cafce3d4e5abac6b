// Weighted D8 flow accumulation (new operator; WeightedFlowAccumulation).
//
// S[c] = q(w[c]) + sum S[d] over the neighbours d whose code points at c: the sum of the
// quantised weights of every cell whose D8 path passes through c, c included.  q(w) = w for
// uint8 and uint32 weights, (int64)rint((double)w * 2^frac_bits) for float32 (hdem_zonal.hip's
// rule), 0 for a NaN; 0 <= q <= 2^31 - 1 or the call is refused, so with H * W < 2^32 every sum
// stays below 2^63.  Integer adds only: bit-exact whatever order they land in.  The codes, what
// makes a cell terminal, the tiles and their perimeter slots are those of hdem_d8tile.h, and
// the scheme is hdem_flowacc.hip's in (+) over 64-bit values: four launches whatever the
// length of the longest path, no workgroup ever waits on another.
//   A  (flowsum_tile_kernel<false>)  per 64 x 64 tile: the weights are read, quantised and
//      counted (NaN, negative, infinite, above 2^31 - 1), then "last donor continues" walks
//      over one 64-bit LDS value per cell.  A 64-bit value leaves no room for the arrivals
//      beside it, so they are hdem_upstream.hip's byte in a 32-bit LDS word per cell, here
//      with the cell's in-tile donor count in the byte's high half: a walk adds its value to
//      its receiver's, then makes one returning add on the receiver's arrival counter
//      (acquire / release at workgroup scope); the arrival that completes the receiver reads
//      the sum and goes on.  A receiver with one in-tile donor needs neither
//      atomic to return: the walk that reaches it is the last, and adds the receiver's seed to
//      the value in its register.  The same scheme serves A and C (C's values need all 64
//      bits, so a packed word could serve A alone, for a second walk to maintain).  Then the
//      tile's 252 perimeter slots: the local sum of each exit cell, the slot of the cell it
//      drains into, and for every perimeter cell the exit its in-tile path reaches.
//   B1 (flowsum_forest_degree_kernel) the exit forest: next(e) and the in-degrees.
//   B2 (flowsum_forest_walk_kernel)  the last-donor walk over the forest: a hop is an
//      agent-scope add on the node's value, then a returning add on its arrival counter; the
//      walk whose add completes the node reads the value with an agent-scope atomic load and
//      goes on.  Words that another workgroup writes during the launch are touched only by
//      agent-scope atomics, and each waits for the value the one before it returned.
//   C  (flowsum_tile_kernel<true>)   A's walk again with seeds q(w) + inflow, the inflow of a
//      perimeter cell being the final forest values of the halo exits that drain into it;
//      writes the wanted outputs (sum, value, mask).  Also counts what never completed.
// Every walk step completes one arrival on one node, so every loop is bounded by the nodes it
// completes (and, explicitly, by the node count).
// Workspace: 28 B per perimeter slot (1.7 B per cell) from the context's arena.
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per forest workgroup
constexpr int TNT = 512;              // threads per tile workgroup (8 cells each)
constexpr int HS = TS + 2;            // staged tile with its one-cell halo
constexpr uint16_t EXIT = 0xFFFE;     // rl[]: receiver in a neighbouring tile
constexpr uint16_t TERM = 0xFFFF;     // rl[]: terminal (code 0, leaves the raster, invalid, outside)
constexpr uint8_t OUTSIDE = 0xFF;     // arr[]: cell of a partial tile beyond the raster
constexpr double Q_MAX = 2147483647.0;

struct flowsum_counters {
    unsigned long long exits;         // exit-forest nodes
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells whose in-tile donors never all arrived
    unsigned long long stuck_exits;   // forest nodes whose donors never all arrived
    unsigned long long nan;           // NaN weights (they contribute 0)
    unsigned long long negative;      // weights below 0 (-inf among them)
    unsigned long long infinite;      // +inf
    unsigned long long over;          // q(w) > 2^31 - 1
    int max_hops;                     // longest B2 walk
};

enum { C_BAD, C_STUCK, C_STUCK_B, C_NAN, C_NEG, C_INF, C_OVER, C_COUNT };

// q(w) of cell g; a weight that is refused counts 0.  n[]: what the weight is counted as.
template <int WT>
__device__ __forceinline__ uint64_t weight_of(const void *__restrict__ weights, size_t g,
                                              double scale, unsigned int (&n)[4])
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
    const uint32_t v = WT == HDEM_FLOWSUM_U32 ? static_cast<const uint32_t *>(weights)[g]
                                              : static_cast<const uint8_t *>(weights)[g];
    if (v > 0x7FFFFFFFu) { ++n[3]; return 0; }
    return v;
}

// arr[]: a byte per cell in 32-bit words, in-tile donors << 4 | arrivals (at most 8 each), so
// that what an arrival's add returns says whether it completed the cell
__device__ __forceinline__ uint32_t arr_byte(const uint32_t *arr, int i)
{
    return (__hip_atomic_load(&arr[i >> 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >>
            (8 * (i & 3))) & 0xFFu;
}

template <bool FINAL, int WT>
__global__ __launch_bounds__(TNT) void flowsum_tile_kernel(
    const uint8_t *__restrict__ d8, int H, int W, int tiles_x, const void *__restrict__ weights,
    double scale, double inv_scale, int64_t threshold, int64_t *__restrict__ out_sum,
    float *__restrict__ out_value, uint8_t *__restrict__ out_mask, uint64_t *__restrict__ word,
    uint32_t *__restrict__ arr_b, uint32_t *__restrict__ indeg_b, int32_t *__restrict__ link,
    int32_t *__restrict__ tgt, flowsum_counters *__restrict__ cnt)
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
    // seeds: q(w), plus in C the final forest values of the halo exits that drain here
    unsigned int bad = 0;
    unsigned int refused[4] = {0, 0, 0, 0};
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
        uint64_t seed = weight_of<WT>(weights, (size_t)(y0 + ly) * W + x0 + lx, scale, refused);
        for (int b = 0; b < 8; ++b) {
            const int ny = ly - code_dy(b), nx = lx - code_dx(b);   // a donor in direction b
            if (code[(ny + 1) * HS + nx + 1] != (1 << b)) continue;
            if (ny >= 0 && ny < TS && nx >= 0 && nx < TS) ++deg;
            else if (FINAL) seed += word[slot_of(tile, tiles_x, ny, nx)];
        }
        arr_bytes[i] = (uint8_t)(deg << 4);
        val[i] = seed;
    }
    if (!FINAL) {       // A counts: C reads the same weights again
        if (bad) atomicAdd(&s_cnt[C_BAD], bad);
        for (int k = 0; k < 4; ++k)
            if (refused[k]) atomicAdd(&s_cnt[C_NAN + k], refused[k]);
    }
    __syncthreads();

    // last donor continues: a walk starts at each cell without in-tile donors, whose seed is
    // its final sum, and carries the sum of the cell it stands on.  A receiver with one
    // in-tile donor is completed by whoever reaches it: the walk adds the receiver's seed in
    // a register and stores the sum.  At any other the walk adds its value, then arrives
    // (release: its add is done; acquire: the other donors' are) and goes on only if its
    // arrival completed the receiver, whose sum it then reads.  Leaf status and completion
    // come from arr[] alone.
    for (int i = tid; i < TC; i += TNT) {
        if (arr_byte(arr, i) >> 4) continue;        // (OUTSIDE too)
        uint64_t v = val[i];
        uint16_t r = rl[i];
        for (int step = 0; step < TC && r < EXIT; ++step) {
            const int shift = 8 * (r & 3);
            const uint32_t need = arr_byte(arr, r) >> 4;
            const uint16_t next = rl[r];
            if (need == 1) {
                v += val[r];
                val[r] = v;
                __hip_atomic_fetch_add(&arr[r >> 2], 1u << shift, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                __hip_atomic_fetch_add(&val[r], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
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
        unsigned int stuck = 0;
        for (int i = tid; i < TC; i += TNT) {
            const int ly = i / TS, lx = i % TS;
            const uint32_t a = arr_byte(arr, i);
            if (a == OUTSIDE) continue;
            if ((a & 0xFu) != a >> 4) ++stuck;
            const int64_t s = (int64_t)val[i];
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            if (out_sum) out_sum[g] = s;
            if (out_value) out_value[g] = __double2float_rn(__dmul_rn((double)s, inv_scale));
            if (out_mask) out_mask[g] = s >= threshold ? 1 : 0;
        }
        unsigned int stuck_b = 0;
        if (tid < PER && tgt[base + tid] >= 0 && arr_b[base + tid] != indeg_b[base + tid])
            ++stuck_b;
        if (stuck) atomicAdd(&s_cnt[C_STUCK], stuck);
        if (stuck_b) atomicAdd(&s_cnt[C_STUCK_B], stuck_b);
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[C_STUCK]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[C_STUCK]);
            if (s_cnt[C_STUCK_B]) atomicAdd(&cnt->stuck_exits, (unsigned long long)s_cnt[C_STUCK_B]);
        }
        return;
    }

    // A: the perimeter slots -- each exit's local sum and the slot it drains into
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
        word[base + tid] = is_exit ? val[p_cell] : 0ull;
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
        if (s_cnt[C_NAN]) atomicAdd(&cnt->nan, (unsigned long long)s_cnt[C_NAN]);
        if (s_cnt[C_NEG]) atomicAdd(&cnt->negative, (unsigned long long)s_cnt[C_NEG]);
        if (s_cnt[C_INF]) atomicAdd(&cnt->infinite, (unsigned long long)s_cnt[C_INF]);
        if (s_cnt[C_OVER]) atomicAdd(&cnt->over, (unsigned long long)s_cnt[C_OVER]);
    }
}

// B1: next(e) of every exit node (the exit its receiver's in-tile path reaches, -1 when that
// path ends in a terminal cell) and the forest in-degrees.  Grid-stride, so that the node
// count costs one global atomic per workgroup.
__global__ __launch_bounds__(NT) void flowsum_forest_degree_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ link,
    int32_t *__restrict__ next, uint32_t *__restrict__ indeg_b, flowsum_counters *__restrict__ cnt)
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

// B2: last-donor walks over the exit forest.  A node's final value is its word once its
// arrivals equal its in-degree.
__global__ __launch_bounds__(NT) void flowsum_forest_walk_kernel(
    int64_t nslots, const int32_t *__restrict__ tgt, const int32_t *__restrict__ next,
    const uint32_t *__restrict__ indeg_b, uint64_t *word, uint32_t *arr_b,
    flowsum_counters *__restrict__ cnt)
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
            // the returned value is below 2^63, which the compiler cannot know: the arrival is
            // issued once the value add has returned, the load once the arrival has
            const uint64_t before = __hip_atomic_fetch_add(&word[t], v, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t old = __hip_atomic_fetch_add(&arr_b[t], 1u + (uint32_t)(before >> 63),
                                                        __ATOMIC_RELAXED,
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

struct flowsum_call {
    const uint8_t *d8;
    int H, W;
    const void *weights;
    int weight_type, frac_bits;
    int64_t threshold;
    int64_t *sum;
    float *value;
    uint8_t *mask;
};

struct span {
    const char *name;
    uintptr_t lo, hi;
};

inline size_t weight_bytes(int weight_type) { return weight_type == HDEM_FLOWSUM_U8 ? 1 : 4; }

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(const hdem_ctx *ctx, const flowsum_call &a, const hdem_flowsum_stats *stats,
               d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, a.d8, a.d8, a.H, a.W)) return rc;
    if (int rc = d8_grid_of("weighted flow accumulation", a.H, a.W, g)) return rc;
    HDEM_REQUIRE(a.weights, HDEM_ERR_BAD_ARG, "the weight raster is null");
    HDEM_REQUIRE(a.weight_type >= HDEM_FLOWSUM_F32 && a.weight_type <= HDEM_FLOWSUM_U8,
                 HDEM_ERR_BAD_ARG, "unknown weight type %d", a.weight_type);
    HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 30, HDEM_ERR_BAD_ARG,
                 "frac_bits is 0 ... 30, got %d", a.frac_bits);
    HDEM_REQUIRE(a.weight_type == HDEM_FLOWSUM_F32 || a.frac_bits == 0, HDEM_ERR_BAD_ARG,
                 "integer weights take frac_bits 0, got %d", a.frac_bits);
    HDEM_REQUIRE(a.sum || a.value || a.mask, HDEM_ERR_BAD_ARG,
                 "no output wanted: give at least one of sum, value, mask");
    HDEM_REQUIRE(!a.mask || a.threshold >= 1, HDEM_ERR_BAD_ARG,
                 "mask needs a threshold >= 1, got %lld", (long long)a.threshold);
    HDEM_REQUIRE(a.mask || a.threshold == 0, HDEM_ERR_BAD_ARG,
                 "a threshold goes with mask: got %lld without one", (long long)a.threshold);
    if (int rc = d8_check_stats(stats, "hdem_flowsum_stats")) return rc;
    const size_t n = (size_t)a.H * a.W;
    span s[5];
    int ns = 0;
    s[ns++] = {"d8", (uintptr_t)a.d8, (uintptr_t)a.d8 + n};
    s[ns++] = {"weights", (uintptr_t)a.weights,
               (uintptr_t)a.weights + n * weight_bytes(a.weight_type)};
    const span outs[3] = {{"sum", (uintptr_t)a.sum, (uintptr_t)a.sum + 8 * n},
                          {"value", (uintptr_t)a.value, (uintptr_t)a.value + 4 * n},
                          {"mask", (uintptr_t)a.mask, (uintptr_t)a.mask + n}};
    for (const span &o : outs) {
        if (!o.lo) continue;
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "weighted flow accumulation: %s overlaps %s", o.name, s[j].name);
        s[ns++] = o;
    }
    return HDEM_OK;
}

template <bool FINAL, int WT>
void launch_tile(hdem_ctx *ctx, const flowsum_call &a, const d8_grid &g, uint64_t *word,
                 uint32_t *arr_b, uint32_t *indeg_b, int32_t *link, int32_t *tgt,
                 flowsum_counters *cnt)
{
    const double scale = (double)(1ll << a.frac_bits);
    hipLaunchKernelGGL((flowsum_tile_kernel<FINAL, WT>), dim3((unsigned)g.tiles), dim3(TNT), 0,
                       ctx->stream, a.d8, a.H, a.W, g.tiles_x, a.weights, scale, 1.0 / scale,
                       a.threshold, a.sum, a.value, a.mask, word, arr_b, indeg_b, link, tgt, cnt);
}
template <bool FINAL, class... Views>
void launch_tile_of_type(hdem_ctx *ctx, const flowsum_call &a, const d8_grid &g, Views... views)
{
    if (a.weight_type == HDEM_FLOWSUM_F32) launch_tile<FINAL, HDEM_FLOWSUM_F32>(ctx, a, g, views...);
    else if (a.weight_type == HDEM_FLOWSUM_U32) launch_tile<FINAL, HDEM_FLOWSUM_U32>(ctx, a, g, views...);
    else launch_tile<FINAL, HDEM_FLOWSUM_U8>(ctx, a, g, views...);
}

int flowsum_dev(hdem_ctx *ctx, const flowsum_call &a, const d8_grid &g, hdem_flowsum_stats *stats)
{
    const int64_t nslots = g.nslots;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_flowsum_stats st = {};
    d8_publish(stats, st);

    // arena: counters | word u64 | arr_b u32 | indeg_b u32 | link i32 | tgt i32 | next i32
    // (per slot)
    const size_t head = 256;
    static_assert(sizeof(flowsum_counters) <= head, "counters outgrew their block");
    const size_t bytes = head + (size_t)nslots * (8 + 5 * 4);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    flowsum_counters *cnt = reinterpret_cast<flowsum_counters *>(ws);
    uint64_t *word = reinterpret_cast<uint64_t *>(ws + head);
    uint32_t *arr_b = reinterpret_cast<uint32_t *>(word + nslots);
    uint32_t *indeg_b = arr_b + nslots;
    int32_t *link = reinterpret_cast<int32_t *>(indeg_b + nslots);
    int32_t *tgt = link + nslots;
    int32_t *next = tgt + nslots;

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(flowsum_counters), ctx->stream));
    const int64_t forest_blocks = (nslots + NT - 1) / NT;
    const int degree_blocks = (int)std::min<int64_t>(forest_blocks, (int64_t)ctx->num_cus * 8);
    phases.mark(0);
    launch_tile_of_type<false>(ctx, a, g, word, arr_b, indeg_b, link, tgt, cnt);
    phases.mark(1);
    hipLaunchKernelGGL(flowsum_forest_degree_kernel, dim3(degree_blocks), dim3(NT), 0,
                       ctx->stream, nslots, tgt, link, next, indeg_b, cnt);
    hipLaunchKernelGGL(flowsum_forest_walk_kernel, dim3((unsigned)forest_blocks), dim3(NT), 0,
                       ctx->stream, nslots, tgt, next, indeg_b, word, arr_b, cnt);
    phases.mark(2);
    launch_tile_of_type<true>(ctx, a, g, word, arr_b, indeg_b, link, tgt, cnt);
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    flowsum_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.max_hops = host.max_hops;
    st.exits = (int64_t)host.exits;
    st.nan_weights = (int64_t)host.nan;
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_tile, &st.ms_forest, &st.ms_final);
    d8_publish(stats, st);
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.negative && !host.infinite && !host.over, HDEM_ERR_BAD_ARG,
                 "weights out of range in %llu cells: %llu negative, %llu infinite, %llu above "
                 "2^31 - 1 once quantised (frac_bits %d)",
                 host.negative + host.infinite + host.over, host.negative, host.infinite,
                 host.over, a.frac_bits);
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_exits, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never drain (%llu of them inside "
                 "tiles, %llu tile exits)",
                 host.stuck_cells + host.stuck_exits, host.stuck_cells, host.stuck_exits);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_flowsum_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                   const void *weights, int weight_type, int frac_bits,
                                   int64_t threshold, int64_t *sum, float *value, uint8_t *mask,
                                   hdem_flowsum_stats *stats)
{
    const flowsum_call a = {d8, H, W, weights, weight_type, frac_bits, threshold, sum, value, mask};
    d8_grid g;
    if (int rc = check_args(ctx, a, stats, &g)) return rc;
    return flowsum_dev(ctx, a, g, stats);
}

extern "C" int hdem_flowsum_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                               const void *weights, int weight_type, int frac_bits,
                               int64_t threshold, int64_t *sum, float *value, uint8_t *mask,
                               hdem_flowsum_stats *stats)
{
    flowsum_call a = {d8, H, W, weights, weight_type, frac_bits, threshold, sum, value, mask};
    d8_grid g;
    if (int rc = check_args(ctx, a, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dweights, dout[3];
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dweights.upload(ctx, weights, n * weight_bytes(weight_type))) return rc;
    void *const host_out[3] = {sum, value, mask};
    const size_t out_bytes[3] = {8 * n, 4 * n, n};
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, out_bytes[k])) return rc;
    a.d8 = dd8.as<const uint8_t>();
    a.weights = dweights.p;
    a.sum = dout[0].as<int64_t>(), a.value = dout[1].as<float>(), a.mask = dout[2].as<uint8_t>();
    if (int rc = flowsum_dev(ctx, a, g, stats)) return rc;
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc = dout[k].download(host_out[k], out_bytes[k])) return rc;
    return HDEM_OK;
}
