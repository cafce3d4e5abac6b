// Downstream D8 path sums and extremes (new operators; FlowPathSum, FlowPathExtreme).
//
// Write the D8 path of c as p_0 = c -> p_1 -> ... -> p_k = s(c), s(c) the first *stop* on it
// exactly as hdem_flowtrace.hip defines one (a terminal cell or, with streams, a stream cell; a
// terminal cell that is no stream cell is *dry* and everything that ends in it is unreached).
//   SUM        S(c) = sum over i < k of q(p_i): the quantised cost of the step that leaves each
//              cell of the path, the stop's own not among them (a stop has S = 0).  q is an
//              integer in 0 ... 2^31 - 1 made once per cell in A: the weight itself or
//              rint(w * 2^frac_bits) per step, rint((w * len) * 2^frac_bits) per unit length
//              with len the length of the leaving step from a table of three doubles per row
//              (east-west, north-south, diagonal).  Integer adds only.
//   MIN / MAX  the least / greatest present value over {p_0, ..., p_k}, c and the stop included,
//              and the cell that holds it: hdem_upextreme.hip's contract (NaN absent, floats by
//              sign-magnitude bits, the smallest flat index among equal bits in both modes).
// Both payloads compose along a path, so the scheme is hdem_flowtrace.hip's with another word
// beside each pointer: 64 x 64 tiles, 252 perimeter slots per tile, a forest over the slots
// (hdem_d8tile.h), pointer jumping, no atomics on the data path.
//   A  (flowpath_tile_kernel)   per tile: receivers and payloads, then Jacobi pointer doubling
//      in LDS on 64-bit words.
//        SUM        pointer | sum << 16.  A path inside a tile has at most 4095 steps, so an
//                   in-tile sum is <= 4095 * (2^31 - 1) < 2^43 and the word holds it in bits
//                   16-58: no carry reaches the pointer from above, none leaves the word, and
//                   composing "a then b" is the one addition (a & ~0xFFFF) + b.  A stop or an
//                   exit holds (itself, 0).
//        MIN / MAX  pointer | field << 16, field = flag << 44 | key << 12 | local holder (its
//                   complement in max mode; the flag says absent in min mode and present in
//                   max mode, so that an absent field loses both ways).  Local row-major order
//                   is flat-index order inside a tile.  After round k a word covers the 2^k
//                   cells of the path from its own on, cut off at the stop or exit that ends
//                   it, which covers itself; the reduction is idempotent, so overlaps do not
//                   matter, and the rounds end only when 2^k exceeds every path: every word
//                   then covers [c ... stop or exit], both included.
//      Writes 8 B per cell (16 bits: which stop / which exit; the in-tile payload; the dry
//      bit) and one 16-byte forest node per perimeter slot: "resolved, stop S, payload" when
//      the frame cell's in-tile path ends in a stop, else "next = the slot of the cell its exit
//      drains into, payload up to and including the exit" -- for a sum that is the in-tile sum
//      plus the cost of the crossing step, q(exit).  Forest payloads are 64 bits: a sum across
//      tiles needs all of them (H * W * 2^31 < 2^63), an extreme is upextreme's word
//      key << 32 | global holder (complemented in max mode).
//   B  (flowpath_forest_kernel) pointer jumping with payload over the slot nodes,
//      node <- (next(next), payload (+) payload').  hdem_flowtrace.hip's race argument carries
//      over unchanged: a node is 16 bytes, nothing is done in place, launch r reads only array
//      r & 1 and writes only array (r + 1) & 1, every node every launch, and the launches are
//      ordered by the stream, so no launch reads what it writes.  The schedule and the counts
//      of unresolved nodes are hdem_d8tile.h's.
//   C  (flowpath_final_kernel)  per tile, streaming: the tile's 252 resolved nodes in LDS,
//      8 B per cell in, every wanted output out.
// Workspace: 8 B per cell, 32 B per perimeter slot (2.0 B per cell) and, per unit length, the
// table (24 B per row) from the context's arena: about 10.0 B per cell.
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per forest / final workgroup
constexpr int TNT = 1024;             // threads per tile workgroup (4 cells each; as the trace)
constexpr int JUMPS = 4;              // forest jumps per node and launch, all in the source array
constexpr uint32_t RESOLVED = 1u;     // node.y
constexpr uint64_t W_DRY = 1ull << 63;   // per-cell word: the stop reached is a dry terminal
constexpr double Q_MAX = 2147483647.0;
constexpr uint32_t QUIET_NAN = 0x7FC00000u;
constexpr uint32_t NOWHERE = 0xFFFFFFFFu;
constexpr uint64_t FIELD_ONES = (1ull << 45) - 1;    // MIN / MAX field: flag, key, holder
constexpr uint64_t SUM_ONES = (1ull << 47) - 1;      // bits 16-62 of a per-cell word

// kind[] of a cell
constexpr uint8_t K_TRAVEL = 0;       // has an in-tile receiver
constexpr uint8_t K_EXIT = 1;         // receiver in a neighbouring tile, cell no stop
constexpr uint8_t K_STOP = 2;         // terminal or stream cell (outside the raster too)
constexpr uint8_t K_DRY = 3;          // terminal, streams given, no stream cell

// node: x = stop (1 + flat index, 0 = dry) when resolved, else the next slot; y = RESOLVED or
// 0; z, w = the 64-bit payload, low half first
typedef uint4 node_t;
__device__ __forceinline__ uint64_t pay_of(const node_t &n) { return (uint64_t)n.w << 32 | n.z; }
__device__ __forceinline__ node_t node_of(uint32_t x, uint32_t y, uint64_t pay)
{
    return make_uint4(x, y, (uint32_t)pay, (uint32_t)(pay >> 32));
}

struct flowpath_counters : d8_forest_counters {
    unsigned long long stops;         // stop cells (stream cells and terminal cells)
    unsigned long long unreached;     // cells whose path ends in a dry terminal
    unsigned long long nan;           // SUM: NaN weights (they cost 0)
    unsigned long long negative;      // SUM: weights below 0 (-inf among them)
    unsigned long long infinite;      // SUM: +inf
    unsigned long long over;          // SUM: q > 2^31 - 1
    unsigned long long absent;        // MIN / MAX: NaN values
};
constexpr size_t FP_HEAD = 512;      // the counters' block at the head of the arena
static_assert(sizeof(flowpath_counters) <= FP_HEAD, "counters outgrew their block");

enum { C_BAD, C_STOPS, C_EXITS, C_STUCK, C_NAN, C_NEG, C_INF, C_OVER, C_ABSENT, C_COUNT };

__device__ __forceinline__ uint32_t w_ptr(uint64_t w) { return (uint32_t)w & 0xFFFFu; }

// the payload (+) of the mode on 64-bit words: forest payloads and, for MIN / MAX, LDS fields
template <int MODE>
__device__ __forceinline__ uint64_t combine(uint64_t a, uint64_t b)
{
    if (MODE == HDEM_FLOWPATH_SUM) return a + b;
    if (MODE == HDEM_FLOWPATH_MIN) return a < b ? a : b;
    return a > b ? a : b;
}

// MIN / MAX: the field of local cell i holding the 32 value bits raw
template <int MODE>
__device__ __forceinline__ uint64_t field_of(uint32_t raw, int value_type, int i,
                                             unsigned int &absent)
{
    uint32_t key = raw;
    if (value_type == HDEM_FLOWPATH_F32) {
        if ((raw & 0x7FFFFFFFu) > 0x7F800000u) {
            ++absent;
            return MODE == HDEM_FLOWPATH_MIN ? FIELD_ONES : 0ull;
        }
        key = key_of(__uint_as_float(raw));
    }
    return MODE == HDEM_FLOWPATH_MIN ? (uint64_t)key << 12 | (uint32_t)i
                                     : 1ull << 44 | (uint64_t)key << 12 | (uint32_t)(~i & 0xFFF);
}
// MIN / MAX: a tile's field as the forest's word, key << 32 | global holder (complemented in
// max mode); the identity (all ones / 0) when nothing is present: no real cell, a NaN has no
// key and flat indices stop at 2^32 - 2
template <int MODE>
__device__ __forceinline__ uint64_t word_of_field(uint64_t f, const d8_tile &t, int W)
{
    const bool flag = (f >> 44) & 1;
    if (MODE == HDEM_FLOWPATH_MIN ? flag : !flag) return MODE == HDEM_FLOWPATH_MIN ? ~0ull : 0ull;
    const uint32_t key = (uint32_t)(f >> 12);
    const int hl = (int)((MODE == HDEM_FLOWPATH_MIN ? f : ~f) & 0xFFF);
    const uint32_t g = (uint32_t)((size_t)(t.y0 + hl / TS) * W + t.x0 + hl % TS);
    return (uint64_t)key << 32 | (MODE == HDEM_FLOWPATH_MIN ? g : ~g);
}

// SUM: q of cell g in row y holding code c.  A weight that is refused counts 0; n[]: what the
// weight is counted as (NaN, negative, infinite, q above 2^31 - 1).  Per unit length a cell
// without a direction (code 0, an invalid byte) has no step to price and q = 0.
__device__ __forceinline__ uint32_t step_cost(const void *__restrict__ weights, int weight_type,
                                              int per, size_t g, int y, uint8_t c, double scale,
                                              const double *__restrict__ step_len,
                                              unsigned int (&n)[4])
{
    double w = 1.0;
    if (weight_type == HDEM_FLOWPATH_F32) {
        const float f = static_cast<const float *>(weights)[g];
        if (f != f) { ++n[0]; return 0; }
        if (f < 0.0f) { ++n[1]; return 0; }                    // -0.0 is not: it counts as 0
        if (f == __builtin_inff()) { ++n[2]; return 0; }
        w = (double)f;
    } else if (weight_type != HDEM_FLOWPATH_NONE) {
        const uint32_t v = weight_type == HDEM_FLOWPATH_U32
                               ? static_cast<const uint32_t *>(weights)[g]
                               : static_cast<const uint8_t *>(weights)[g];
        if (per == HDEM_FLOWPATH_PER_STEP) {
            if (v > 0x7FFFFFFFu) { ++n[3]; return 0; }
            return v;
        }
        w = (double)v;
    }
    double d;
    if (per == HDEM_FLOWPATH_PER_LENGTH) {
        if (!c || (c & (c - 1))) return 0;
        const int b = __builtin_ctz(c);
        const int k = (b & 1) ? 2 : (b & 2) ? 1 : 0;   // diagonal; N, S; E, W
        // one rounding in the product, an exact scaling, one rint
        d = rint(__dmul_rn(__dmul_rn(w, step_len[3 * (size_t)y + k]), scale));
    } else {
        d = rint(__dmul_rn(w, scale));   // exact product, one rounding to nearest even
    }
    if (d > Q_MAX) { ++n[3]; return 0; }
    return (uint32_t)(long long)d;
}

// A.  STREAMS 0: none, 1: uint8 mask, 2: uint32 raster against a threshold.  values: the
// weights of a sum (may be null per unit length), the values of an extreme.
template <int MODE, int STREAMS>
__global__ __launch_bounds__(TNT) void flowpath_tile_kernel(
    const uint8_t *__restrict__ d8, const void *__restrict__ streams, uint32_t threshold, int H,
    int W, int tiles_x, const void *__restrict__ values, int value_type, int per, double scale,
    const double *__restrict__ step_len, uint64_t *__restrict__ cellw, node_t *__restrict__ node,
    flowpath_counters *__restrict__ cnt)
{
    constexpr bool SUM = MODE == HDEM_FLOWPATH_SUM;
    __shared__ uint8_t code[TC];
    __shared__ uint8_t kind[TC];
    __shared__ uint64_t jump[2][TC];
    __shared__ uint32_t exit_q[SUM ? PER : 1];   // SUM: q of an exit cell, by perimeter slot
    __shared__ unsigned int s_cnt[C_COUNT];

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;

    if (tid < C_COUNT) s_cnt[tid] = 0;
    __syncthreads();

    // receivers and payloads; a stop or an exit points at itself: no steps taken, and for an
    // extreme its own value
    unsigned int bad = 0, stops = 0, absent = 0;
    unsigned int refused[4] = {0, 0, 0, 0};
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        uint8_t k = K_STOP;
        uint64_t w = (uint64_t)i;
        if (!SUM) w |= (MODE == HDEM_FLOWPATH_MIN ? FIELD_ONES : 0ull) << 16;
        int c = 0;
        if (tile.inside(ly, lx)) {
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            c = d8[g];
            bool stream = false;
            if (STREAMS == 1) stream = static_cast<const uint8_t *>(streams)[g] != 0;
            if (STREAMS == 2) stream = static_cast<const uint32_t *>(streams)[g] >= threshold;
            const d8_step s = d8_decode(c, ly, lx, tile, H, W);
            if (s.invalid) ++bad;
            uint64_t pay;
            if (SUM)
                pay = step_cost(values, value_type, per, g, y0 + ly, (uint8_t)c, scale, step_len,
                                refused);
            else
                pay = field_of<MODE>(static_cast<const uint32_t *>(values)[g], value_type, i,
                                     absent);
            int to = i;
            if (stream || s.terminal) {
                k = (STREAMS == 0 || stream) ? K_STOP : K_DRY;
                ++stops;
            } else if (s.in_tile()) {
                k = K_TRAVEL;
                to = s.ny * TS + s.nx;
            } else {
                k = K_EXIT;
                if (SUM) exit_q[perim_pos(ly, lx)] = (uint32_t)pay;
            }
            if (SUM && k != K_TRAVEL) pay = 0;
            w = (uint64_t)to | pay << 16;
        }
        code[i] = (uint8_t)c;
        kind[i] = k;
        jump[0][i] = w;
    }
    if (bad) atomicAdd(&s_cnt[C_BAD], bad);
    if (stops) atomicAdd(&s_cnt[C_STOPS], stops);
    if (absent) atomicAdd(&s_cnt[C_ABSENT], absent);
    for (int k = 0; k < 4; ++k)
        if (refused[k]) atomicAdd(&s_cnt[C_NAN + k], refused[k]);
    __syncthreads();

    // pointer doubling: after round k a cell points 2^k steps down its in-tile path, or at
    // the stop / exit that ends it, and carries the payload of the cells up to where it points
    int cur = 0;
    for (int round = 0; round < DOUBLINGS; ++round) {
        int changed = 0;
        for (int i = tid; i < TC; i += TNT) {
            const uint64_t a = jump[cur][i];
            const uint64_t b = jump[cur][w_ptr(a)];
            jump[cur ^ 1][i] = SUM ? (a & ~0xFFFFull) + b
                                   : combine<MODE>(a >> 16, b >> 16) << 16 | w_ptr(b);
            changed |= w_ptr(a) != w_ptr(b);
        }
        cur ^= 1;
        if (!__syncthreads_or(changed)) break;
    }
    const uint64_t *jmp = jump[cur];

    // 8 B per cell for C: the stop (local index) or the exit (perimeter slot) it reaches and
    // the payload up to it: for a sum without its cost, for an extreme with its value
    unsigned int stuck = 0;
    for (int i = tid; i < TC; i += TNT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const uint64_t w = jmp[i];
        const uint32_t t = w_ptr(w);
        const uint8_t k = kind[t];
        if (k == K_TRAVEL) ++stuck;                      // a cycle inside the tile
        const uint64_t target = k == K_EXIT ? (uint64_t)(T_EXIT | perim_pos(t / TS, t % TS)) : t;
        const uint64_t pay = SUM ? (w >> 16) & SUM_ONES : w >> 16;
        cellw[(size_t)blockIdx.x * TC + i] = target | pay << 16 | (k == K_DRY ? W_DRY : 0ull);
    }
    if (stuck) atomicAdd(&s_cnt[C_STUCK], stuck);

    // the perimeter slots
    if (tid < PER) {
        int ly, lx;
        perim_cell(tid, ly, lx);
        node_t n = node_of(0u, RESOLVED, 0ull);          // outside the raster: never read
        if (tile.inside(ly, lx)) {
            const int i = ly * TS + lx;
            const uint64_t w = jmp[i];
            const int t = (int)w_ptr(w);
            const uint8_t k = kind[t];
            const int t_ly = t / TS, t_lx = t % TS;
            uint64_t pay = SUM ? w >> 16 : word_of_field<MODE>(w >> 16, tile, W);
            if (k == K_STOP) {
                n = node_of((uint32_t)((size_t)(y0 + t_ly) * W + x0 + t_lx) + 1u, RESOLVED, pay);
            } else if (k == K_DRY) {
                n = node_of(0u, RESOLVED, pay);
            } else if (k == K_EXIT) {
                const int b = __builtin_ctz(code[t]);
                if (SUM) pay += exit_q[perim_pos(t_ly, t_lx)];       // the crossing step
                n = node_of((uint32_t)slot_of(tile, tiles_x, t_ly + code_dy(b), t_lx + code_dx(b)),
                            0u, pay);
            } else {
                n = node_of((uint32_t)(tile.base + tid), 0u, 0ull);  // a cycle: unresolved
            }
            if (kind[i] == K_EXIT) atomicAdd(&s_cnt[C_EXITS], 1u);
        }
        node[tile.base + tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[C_BAD]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[C_BAD]);
        if (s_cnt[C_STOPS]) atomicAdd(&cnt->stops, (unsigned long long)s_cnt[C_STOPS]);
        if (s_cnt[C_EXITS]) atomicAdd(&cnt->exits, (unsigned long long)s_cnt[C_EXITS]);
        if (s_cnt[C_STUCK]) atomicAdd(&cnt->stuck_cells, (unsigned long long)s_cnt[C_STUCK]);
        if (s_cnt[C_NAN]) atomicAdd(&cnt->nan, (unsigned long long)s_cnt[C_NAN]);
        if (s_cnt[C_NEG]) atomicAdd(&cnt->negative, (unsigned long long)s_cnt[C_NEG]);
        if (s_cnt[C_INF]) atomicAdd(&cnt->infinite, (unsigned long long)s_cnt[C_INF]);
        if (s_cnt[C_OVER]) atomicAdd(&cnt->over, (unsigned long long)s_cnt[C_OVER]);
        if (s_cnt[C_ABSENT]) atomicAdd(&cnt->absent, (unsigned long long)s_cnt[C_ABSENT]);
    }
}

// B: one round of pointer jumping with payload, src -> dst.  Grid-stride.
template <int MODE>
__global__ __launch_bounds__(NT) void flowpath_forest_kernel(int64_t nslots, int round,
                                                             const node_t *__restrict__ src,
                                                             node_t *__restrict__ dst,
                                                             flowpath_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_left;
    if (!d8_forest_begin(cnt, round, &s_left)) return;
    unsigned int left = 0;
    for (int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x; s < nslots;
         s += (int64_t)gridDim.x * NT) {
        node_t n = src[s];
        uint64_t pay = pay_of(n);
        for (int j = 0; j < JUMPS && !(n.y & RESOLVED); ++j) {
            const node_t t = src[n.x];                   // my pointer's node, as the last launch left it
            pay = combine<MODE>(pay, pay_of(t));
            n.x = t.x, n.y = t.y;
        }
        dst[s] = node_of(n.x, n.y, pay);
        left += !(n.y & RESOLVED);
    }
    d8_forest_end(cnt, round, left, &s_left);
}

// C.  Every output pointer may be null (not wanted).  SUM: out_a is sum (int64), out_b value
// (float32); MIN / MAX: out_a is extreme (32 bits), out_b where (uint32).
template <int MODE>
__global__ __launch_bounds__(NT) void flowpath_final_kernel(
    int H, int W, int tiles_x, int rounds, const uint64_t *__restrict__ cellw,
    const node_t *__restrict__ node0, const node_t *__restrict__ node1, int value_type,
    double inv_scale, uint32_t *__restrict__ out_stop, void *__restrict__ out_a,
    uint32_t *__restrict__ out_b, flowpath_counters *__restrict__ cnt)
{
    constexpr bool SUM = MODE == HDEM_FLOWPATH_SUM;
    __shared__ uint32_t n_stop[PER];
    __shared__ uint64_t n_pay[PER];
    __shared__ uint8_t known[PER];
    __shared__ unsigned int s_cnt[3];            // stuck cells, stuck slots, unreached cells

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const uint64_t *cw = cellw + (size_t)blockIdx.x * TC;

    if (tid < 3) s_cnt[tid] = 0;
    if (tid < PER) {
        // launch r of B wrote array (r + 1) & 1; the first that left nothing unresolved wrote
        // the result, and every later one returned at once
        int r = 0;
        while (r < rounds - 1 && cnt->unresolved[r]) ++r;
        const node_t n = (((r + 1) & 1) ? node1 : node0)[tile.base + tid];
        const bool ok = (n.y & RESOLVED) != 0;
        n_stop[tid] = ok ? n.x : 0u;                     // a slot number is no cell
        n_pay[tid] = pay_of(n);
        known[tid] = ok;
    }
    __syncthreads();
    if (tid < PER && !known[tid]) atomicAdd(&s_cnt[1], 1u);

    unsigned int stuck = 0, unreached = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        const uint64_t c = cw[i];
        const uint32_t v = (uint32_t)c & 0xFFFFu;
        uint64_t pay = SUM ? (c >> 16) & SUM_ONES
                           : word_of_field<MODE>((c >> 16) & FIELD_ONES, tile, W);
        uint32_t stop;
        if (v & T_EXIT) {
            const int p = v & 0xFF;
            stop = n_stop[p];
            pay = combine<MODE>(pay, n_pay[p]);
            stuck += !known[p];
        } else {
            stop = (c & W_DRY) ? 0u : (uint32_t)((size_t)(y0 + v / TS) * W + x0 + v % TS) + 1u;
        }
        unreached += stop == 0u;
        if (out_stop) out_stop[g] = stop;
        if (SUM) {
            if (out_a) static_cast<int64_t *>(out_a)[g] = (int64_t)pay;
            if (out_b)
                out_b[g] = stop ? __float_as_uint(__double2float_rn(
                                      __dmul_rn((double)(int64_t)pay, inv_scale)))
                                : QUIET_NAN;
        } else {
            const bool present = pay != (MODE == HDEM_FLOWPATH_MIN ? ~0ull : 0ull);
            const uint32_t key = (uint32_t)(pay >> 32);
            const uint32_t holder = MODE == HDEM_FLOWPATH_MIN ? (uint32_t)pay : ~(uint32_t)pay;
            if (out_a)
                static_cast<uint32_t *>(out_a)[g] =
                    value_type != HDEM_FLOWPATH_F32 ? key
                    : present ? __float_as_uint(float_of(key)) : QUIET_NAN;
            if (out_b) out_b[g] = present ? holder : NOWHERE;
        }
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

// One call.  values: the weights of a sum, the values of an extreme.  out_a / out_b: sum and
// value, or extreme and where (the final kernel's pair).
struct flowpath_call {
    const uint8_t *d8;
    int H, W;
    const void *streams;
    int stream_kind;
    uint32_t threshold;
    int mode;
    const void *values;
    int value_type, per, frac_bits;
    const double *step_len;           // host, 3 * H doubles, or null
    uint32_t *stop;
    int64_t *sum;
    float *value;
    void *extreme;
    uint32_t *where;
    int flags;
};

struct span {
    const char *name;
    uintptr_t lo, hi;
};

inline size_t value_bytes(int value_type) { return value_type == HDEM_FLOWPATH_U8 ? 1 : 4; }

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(const hdem_ctx *ctx, const flowpath_call &a, const hdem_flowpath_stats *stats,
               d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, a.d8, a.d8, a.H, a.W)) return rc;
    if (int rc = d8_grid_of("the flow path", a.H, a.W, g)) return rc;
    HDEM_REQUIRE(!a.flags, HDEM_ERR_BAD_ARG, "unknown flow path flags 0x%x", a.flags);
    HDEM_REQUIRE(a.mode >= HDEM_FLOWPATH_SUM && a.mode <= HDEM_FLOWPATH_MAX, HDEM_ERR_BAD_ARG,
                 "unknown mode %d", a.mode);
    HDEM_REQUIRE(a.value_type >= HDEM_FLOWPATH_NONE && a.value_type <= HDEM_FLOWPATH_U8,
                 HDEM_ERR_BAD_ARG, "unknown value type %d", a.value_type);
    HDEM_REQUIRE((a.value_type == HDEM_FLOWPATH_NONE) == !a.values, HDEM_ERR_BAD_ARG,
                 "values and value type %d do not go together: HDEM_FLOWPATH_NONE takes null "
                 "values, every other type a raster", a.value_type);
    if (int rc = d8_check_streams(a.streams, a.stream_kind, a.threshold)) return rc;
    if (a.mode == HDEM_FLOWPATH_SUM) {
        HDEM_REQUIRE(a.per == HDEM_FLOWPATH_PER_STEP || a.per == HDEM_FLOWPATH_PER_LENGTH,
                     HDEM_ERR_BAD_ARG, "unknown per %d", a.per);
        HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 30, HDEM_ERR_BAD_ARG,
                     "frac_bits is 0 ... 30, got %d", a.frac_bits);
        HDEM_REQUIRE(!a.extreme && !a.where, HDEM_ERR_BAD_ARG,
                     "extreme and where are outputs of the min and max modes, not of a sum");
        HDEM_REQUIRE(a.stop || a.sum || a.value, HDEM_ERR_BAD_ARG,
                     "no output wanted: give at least one of stop, sum, value");
        if (a.per == HDEM_FLOWPATH_PER_STEP) {
            HDEM_REQUIRE(a.values, HDEM_ERR_BAD_ARG,
                         "a sum per step needs the weights it sums (per unit length they may be "
                         "null)");
            HDEM_REQUIRE(!a.step_len, HDEM_ERR_BAD_ARG,
                         "step_len goes with HDEM_FLOWPATH_PER_LENGTH: null per step");
            HDEM_REQUIRE(a.value_type == HDEM_FLOWPATH_F32 || a.frac_bits == 0, HDEM_ERR_BAD_ARG,
                         "integer weights per step take frac_bits 0, got %d", a.frac_bits);
        } else {
            HDEM_REQUIRE(a.step_len, HDEM_ERR_BAD_ARG,
                         "a sum per unit length needs step_len, 3 * H doubles");
        }
    } else {
        HDEM_REQUIRE(a.value_type == HDEM_FLOWPATH_F32 || a.value_type == HDEM_FLOWPATH_U32,
                     HDEM_ERR_BAD_ARG, "min and max take float32 or uint32 values, got type %d",
                     a.value_type);
        HDEM_REQUIRE(a.per == HDEM_FLOWPATH_PER_STEP && a.frac_bits == 0 && !a.step_len,
                     HDEM_ERR_BAD_ARG,
                     "per, frac_bits and step_len belong to a sum: 0, 0 and null with min and max");
        HDEM_REQUIRE(!a.sum && !a.value, HDEM_ERR_BAD_ARG,
                     "sum and value are outputs of a sum, not of the min and max modes");
        HDEM_REQUIRE(a.stop || a.extreme || a.where, HDEM_ERR_BAD_ARG,
                     "no output wanted: give at least one of stop, extreme, where");
    }
    if (int rc = d8_check_stats(stats, "hdem_flowpath_stats")) return rc;
    const size_t n = (size_t)a.H * a.W;
    span s[8];
    int ns = 0;
    s[ns++] = {"d8", (uintptr_t)a.d8, (uintptr_t)a.d8 + n};
    if (a.streams)
        s[ns++] = {"streams", (uintptr_t)a.streams,
                   (uintptr_t)a.streams + n * (a.stream_kind == HDEM_FT_STREAMS_ACC_U32 ? 4 : 1)};
    if (a.values)
        s[ns++] = {a.mode == HDEM_FLOWPATH_SUM ? "weights" : "values", (uintptr_t)a.values,
                   (uintptr_t)a.values + n * value_bytes(a.value_type)};
    const span outs[5] = {{"stop", (uintptr_t)a.stop, (uintptr_t)a.stop + 4 * n},
                          {"sum", (uintptr_t)a.sum, (uintptr_t)a.sum + 8 * n},
                          {"value", (uintptr_t)a.value, (uintptr_t)a.value + 4 * n},
                          {"extreme", (uintptr_t)a.extreme, (uintptr_t)a.extreme + 4 * n},
                          {"where", (uintptr_t)a.where, (uintptr_t)a.where + 4 * n}};
    for (const span &o : outs) {
        if (!o.lo) continue;
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "the flow path: %s overlaps %s", o.name, s[j].name);
        s[ns++] = o;
    }
    // the table, before any launch
    if (a.step_len) {
        long long wrong = 0, first = -1;
        for (long long k = 0; k < 3ll * a.H; ++k)
            if (!(std::isfinite(a.step_len[k]) && a.step_len[k] > 0.0)) {
                if (!wrong) first = k;
                ++wrong;
            }
        HDEM_REQUIRE(!wrong, HDEM_ERR_BAD_ARG,
                     "step_len has %lld entries that are not finite and positive, the first in "
                     "row %lld (%g)", wrong, first / 3, a.step_len[first < 0 ? 0 : first]);
    }
    return HDEM_OK;
}

struct flowpath_views {
    flowpath_counters *cnt;
    node_t *node[2];
    uint64_t *cellw;
    double *step_len;
};

template <int MODE, int STREAMS>
void launch_tile(hdem_ctx *ctx, const flowpath_call &a, const d8_grid &g, const flowpath_views &v)
{
    hipLaunchKernelGGL((flowpath_tile_kernel<MODE, STREAMS>), dim3((unsigned)g.tiles), dim3(TNT),
                       0, ctx->stream, a.d8, a.streams, a.threshold, a.H, a.W, g.tiles_x, a.values,
                       a.value_type, a.per, (double)(1ll << a.frac_bits),
                       a.step_len ? v.step_len : nullptr, v.cellw, v.node[0], v.cnt);
}

template <int MODE>
void launch_all(hdem_ctx *ctx, const flowpath_call &a, const d8_grid &g, const flowpath_views &v,
                const d8_forest_plan &forest, hdem_event_timer<4> &phases)
{
    if (a.stream_kind == HDEM_FT_STREAMS_NONE) launch_tile<MODE, 0>(ctx, a, g, v);
    else if (a.stream_kind == HDEM_FT_STREAMS_MASK_U8) launch_tile<MODE, 1>(ctx, a, g, v);
    else launch_tile<MODE, 2>(ctx, a, g, v);
    phases.mark(1);
    for (int r = 0; r < forest.rounds; ++r)
        hipLaunchKernelGGL(flowpath_forest_kernel<MODE>, dim3(forest.grid), dim3(NT), 0,
                           ctx->stream, g.nslots, r, v.node[r & 1], v.node[(r + 1) & 1], v.cnt);
    phases.mark(2);
    const bool sum = MODE == HDEM_FLOWPATH_SUM;
    hipLaunchKernelGGL(flowpath_final_kernel<MODE>, dim3((unsigned)g.tiles), dim3(NT), 0,
                       ctx->stream, a.H, a.W, g.tiles_x, forest.rounds, v.cellw, v.node[0],
                       v.node[1], a.value_type, 1.0 / (double)(1ll << a.frac_bits), a.stop,
                       sum ? static_cast<void *>(a.sum) : a.extreme,
                       sum ? reinterpret_cast<uint32_t *>(a.value) : a.where, v.cnt);
    phases.mark(3);
}

// the rasters of `a` are device pointers, step_len a host pointer
int flowpath_dev(hdem_ctx *ctx, const flowpath_call &a, const d8_grid &g,
                 hdem_flowpath_stats *stats)
{
    const int64_t tiles = g.tiles, nslots = g.nslots;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_flowpath_stats st = {};
    d8_publish(stats, st);

    // arena: counters | two node arrays, 16 B per slot each | the cell words, u64 per cell |
    // the table, 3 doubles per row
    const size_t table = a.step_len ? (size_t)a.H * 3 * sizeof(double) : 0;
    const size_t bytes = FP_HEAD + (size_t)nslots * 32 + (size_t)tiles * TC * 8 + table;
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    flowpath_views v;
    v.cnt = reinterpret_cast<flowpath_counters *>(ws);
    v.node[0] = reinterpret_cast<node_t *>(ws + FP_HEAD);
    v.node[1] = v.node[0] + nslots;
    v.cellw = reinterpret_cast<uint64_t *>(v.node[1] + nslots);
    v.step_len = reinterpret_cast<double *>(v.cellw + (size_t)tiles * TC);

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(v.cnt, 0, sizeof(flowpath_counters), ctx->stream));
    if (table)      // the caller's table stays as it is until the call's one synchronisation
        HDEM_HIP_CHECK(hipMemcpyAsync(v.step_len, a.step_len, table, hipMemcpyHostToDevice,
                                      ctx->stream));
    const d8_forest_plan forest = d8_forest_plan_of(ctx, nslots, NT);
    phases.mark(0);
    if (a.mode == HDEM_FLOWPATH_SUM) launch_all<HDEM_FLOWPATH_SUM>(ctx, a, g, v, forest, phases);
    else if (a.mode == HDEM_FLOWPATH_MIN) launch_all<HDEM_FLOWPATH_MIN>(ctx, a, g, v, forest, phases);
    else launch_all<HDEM_FLOWPATH_MAX>(ctx, a, g, v, forest, phases);
    HDEM_HIP_CHECK(hipGetLastError());
    flowpath_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, v.cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.forest_rounds = d8_forest_rounds(forest, host);
    st.stops = (int64_t)host.stops;
    st.unreached = (int64_t)host.unreached;
    st.exits = (int64_t)host.exits;
    st.nan_weights = (int64_t)host.nan;
    st.absent = (int64_t)host.absent;
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
    return d8_report_forest(host);
}

flowpath_call call_of(const uint8_t *d8, int H, int W, const void *streams, int stream_kind,
                      uint32_t threshold, int mode, const void *values, int value_type, int per,
                      int frac_bits, const double *step_len, uint32_t *stop, int64_t *sum,
                      float *value, void *extreme, uint32_t *where, int flags)
{
    return {d8,  H,         W,        streams, stream_kind, threshold, mode,    values, value_type,
            per, frac_bits, step_len, stop,    sum,         value,     extreme, where,  flags};
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_flowpath_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                    const void *streams, int stream_kind, uint32_t threshold,
                                    int mode, const void *values, int value_type, int per,
                                    int frac_bits, const double *step_len, uint32_t *stop,
                                    int64_t *sum, float *value, void *extreme, uint32_t *where,
                                    int flags, hdem_flowpath_stats *stats)
{
    const flowpath_call a = call_of(d8, H, W, streams, stream_kind, threshold, mode, values,
                                    value_type, per, frac_bits, step_len, stop, sum, value,
                                    extreme, where, flags);
    d8_grid g;
    if (int rc = check_args(ctx, a, stats, &g)) return rc;
    return flowpath_dev(ctx, a, g, stats);
}

extern "C" int hdem_flowpath_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                const void *streams, int stream_kind, uint32_t threshold,
                                int mode, const void *values, int value_type, int per,
                                int frac_bits, const double *step_len, uint32_t *stop,
                                int64_t *sum, float *value, void *extreme, uint32_t *where,
                                int flags, hdem_flowpath_stats *stats)
{
    flowpath_call a = call_of(d8, H, W, streams, stream_kind, threshold, mode, values, value_type,
                              per, frac_bits, step_len, stop, sum, value, extreme, where, flags);
    d8_grid g;
    if (int rc = check_args(ctx, a, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dstreams, dvalues, dout[5];
    const size_t sb = n * (stream_kind == HDEM_FT_STREAMS_ACC_U32 ? sizeof(uint32_t) : 1);
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dstreams.upload(ctx, streams, sb)) return rc;
    if (int rc = dvalues.upload(ctx, values, n * value_bytes(value_type))) return rc;
    void *const host_out[5] = {stop, sum, value, extreme, where};
    const size_t out_bytes[5] = {4 * n, 8 * n, 4 * n, 4 * n, 4 * n};
    for (int k = 0; k < 5; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, out_bytes[k])) return rc;
    a.d8 = dd8.as<const uint8_t>();
    a.streams = dstreams.p;
    a.values = dvalues.p;
    a.stop = dout[0].as<uint32_t>(), a.sum = dout[1].as<int64_t>(), a.value = dout[2].as<float>();
    a.extreme = dout[3].p, a.where = dout[4].as<uint32_t>();
    if (int rc = flowpath_dev(ctx, a, g, stats)) return rc;
    for (int k = 0; k < 5; ++k)
        if (host_out[k])
            if (int rc = dout[k].download(host_out[k], out_bytes[k])) return rc;
    return HDEM_OK;
}
