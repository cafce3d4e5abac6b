// The tiled D8 scheme shared by hdem_flowacc.hip, hdem_watershed.hip and hdem_flowtrace.hip;
// not part of the C ABI.  Codes are ESRI (E=1, SE=2, S=4, SW=8, W=16, NW=32, N=64, NE=128).
// The raster is cut into 64 x 64 tiles, the frame of a tile is its 252 perimeter slots, and a
// forest is built over the slots of all tiles: A per tile, B the forest, C per tile again with
// B's result.  What A, B and C do, and with how many threads, is each operator's own.
// Watersheds and the flow trace resolve their forest by pointer jumping and share its
// schedule, its count of unresolved nodes and its counters; flow accumulation counts arrivals.
// Every tiled operator, the ones without a forest too, takes the tile of a workgroup, the event
// timer, the stream-set check and the stats helpers from here.
#pragma once

#include "hdem_internal.h"

#include <algorithm>
#include <cstring>

constexpr int TS = 64;                // tile edge
constexpr int TC = TS * TS;           // cells per tile (12-bit local index)
constexpr int PER = 4 * TS - 4;       // perimeter slots per tile
constexpr int DOUBLINGS = 12;         // 2^12 >= the longest path inside a tile (4095 steps)
constexpr int MAX_ROUNDS = 32;        // forest launches: slots < 2^31
constexpr uint16_t T_EXIT = 0x8000;   // per-cell target: perimeter slot of the exit reached

// float -> uint32 whose unsigned order is the floats' order: -0.0 below +0.0.
// What the depression table and the zonal statistics gather a float minimum or maximum as.
__device__ __forceinline__ uint32_t key_of(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float float_of(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k);
}

// bit b of a code -> (dy, dx), packed (d + 1) in 4 bits per entry; odd bits are diagonal
__device__ __forceinline__ int code_dy(int b) { return ((0x00012221u >> (4 * b)) & 3) - 1; }
__device__ __forceinline__ int code_dx(int b) { return ((0x21000122u >> (4 * b)) & 3) - 1; }

// perimeter slot of a frame cell: top row, bottom row, left column, right column
__device__ __forceinline__ int perim_pos(int ly, int lx)
{
    return ly == 0 ? lx : ly == TS - 1 ? TS + lx : lx == 0 ? 2 * TS + ly - 1 : 3 * TS - 2 + ly - 1;
}
__device__ __forceinline__ void perim_cell(int p, int &ly, int &lx)
{
    if (p < TS) { ly = 0; lx = p; }
    else if (p < 2 * TS) { ly = TS - 1; lx = p - TS; }
    else if (p < 3 * TS - 2) { ly = p - 2 * TS + 1; lx = 0; }
    else { ly = p - (3 * TS - 2) + 1; lx = TS - 1; }
}

// The tile of a workgroup: one workgroup per tile, row-major.
struct d8_tile {
    int ty, tx;                       // tile coordinates
    int y0, x0;                       // its first cell
    int th, tw;                       // its extent inside the raster (< TS in a partial tile)
    int64_t base;                     // its first perimeter slot
    __device__ __forceinline__ bool inside(int ly, int lx) const { return ly < th && lx < tw; }
};
__device__ __forceinline__ d8_tile d8_tile_of_block(int tiles_x, int H, int W)
{
    d8_tile t;
    t.ty = blockIdx.x / tiles_x, t.tx = blockIdx.x % tiles_x;
    t.y0 = t.ty * TS, t.x0 = t.tx * TS;
    t.th = min(TS, H - t.y0), t.tw = min(TS, W - t.x0);
    t.base = (int64_t)blockIdx.x * PER;
    return t;
}

// Slot of local frame position (ny, nx) that may lie one cell outside tile t: the perimeter
// slot of that cell in the tile that holds it.
__device__ __forceinline__ int64_t slot_of(const d8_tile &t, int tiles_x, int ny, int nx)
{
    const int sy = ny < 0 ? -1 : ny >= TS ? 1 : 0;
    const int sx = nx < 0 ? -1 : nx >= TS ? 1 : 0;
    const int64_t tile = (int64_t)(t.ty + sy) * tiles_x + (t.tx + sx);
    return tile * PER + perim_pos(ny - sy * TS, nx - sx * TS);
}

// Where the code c of cell (ly, lx) of tile t sends that cell: the operators' one definition
// of D8.  0, a byte with more than one bit set and a code pointing outside the raster make
// the cell terminal.
struct d8_step {
    bool invalid;                     // more than one bit set
    bool terminal;
    int b;                            // direction bit
    int ny, nx;                       // the receiver, local to the tile (may be -1 or TS)
    // not terminal: the receiver lies in this tile (else the cell is one of the tile's exits)
    __device__ __forceinline__ bool in_tile() const
    {
        return ny >= 0 && ny < TS && nx >= 0 && nx < TS;
    }
};
__device__ __forceinline__ d8_step d8_decode(uint8_t c, int ly, int lx, const d8_tile &t, int H,
                                              int W)
{
    d8_step s = {false, true, 0, 0, 0};
    if (c & (c - 1)) {
        s.invalid = true;
    } else if (c) {
        s.b = __builtin_ctz(c);
        s.ny = ly + code_dy(s.b);
        s.nx = lx + code_dx(s.b);
        const int gy = t.y0 + s.ny, gx = t.x0 + s.nx;
        s.terminal = !(gy >= 0 && gy < H && gx >= 0 && gx < W);
    }
    return s;
}

// Counters of an operator whose forest is resolved by pointer jumping; its own derive from it.
struct d8_forest_counters {
    unsigned long long exits;         // exit cells (forest pointers of their own)
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stuck_cells;   // cells that never reached a stop
    unsigned long long stuck_slots;   // forest nodes that never resolved
    unsigned long long unresolved[MAX_ROUNDS];   // forest nodes left after each round
};

// One launch of B, all threads.  begin: false when the previous round left nothing unresolved
// (this launch has no work).  end: adds the nodes the workgroup's threads left unresolved to
// unresolved[round]: wave shuffle, LDS, one global atomic.
__device__ __forceinline__ bool d8_forest_begin(const d8_forest_counters *cnt, int round,
                                                unsigned int *s_left)
{
    if (round > 0 && __hip_atomic_load(&cnt->unresolved[round - 1], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT) == 0)
        return false;
    if (threadIdx.x == 0) *s_left = 0;
    __syncthreads();
    return true;
}
__device__ __forceinline__ void d8_forest_end(d8_forest_counters *cnt, int round,
                                              unsigned int left, unsigned int *s_left)
{
    for (int m = 32; m >= 1; m >>= 1) left += __shfl_xor(left, m);
    if ((threadIdx.x & 63) == 0 && left) atomicAdd(s_left, left);
    __syncthreads();
    if (threadIdx.x == 0 && *s_left)
        atomicAdd(&cnt->unresolved[round], (unsigned long long)*s_left);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct d8_grid {
    int tiles_y, tiles_x;
    int64_t tiles, nslots;
};
// The tile grid of an H x W raster, or why `op` cannot take it.  Allocates nothing.
inline int d8_grid_of(const char *op, int H, int W, d8_grid *g)
{
    const int64_t cells = (int64_t)H * W;
    HDEM_REQUIRE(cells <= (int64_t)UINT32_MAX, HDEM_ERR_BAD_ARG,
                 "%s works in uint32: %d x %d = %lld cells is more than 2^32 - 1", op, H, W,
                 (long long)cells);
    g->tiles_y = (H + TS - 1) / TS, g->tiles_x = (W + TS - 1) / TS;
    g->tiles = (int64_t)g->tiles_y * g->tiles_x;
    g->nslots = g->tiles * PER;
    // (slots are int32; only rasters a few cells wide and ~10^9 long get here)
    HDEM_REQUIRE(g->nslots <= INT32_MAX, HDEM_ERR_BAD_ARG,
                 "%s: %d x %d has %lld tiles of %d x %d, more than %d", op, H, W,
                 (long long)g->tiles, TS, TS, INT32_MAX / PER);
    return HDEM_OK;
}

// HIP-event times between N marks on the context's stream, taken when the context profiles and
// the caller wants stats.  The events go with the object, whichever way the call returns.
template <int N>
struct hdem_event_timer {
    hipEvent_t ev[N] = {};
    hipStream_t stream;
    bool on;
    hdem_event_timer(const hdem_ctx *ctx, bool wanted)
        : stream(ctx->stream), on(ctx->profiling && wanted) {}
    hdem_event_timer(const hdem_event_timer &) = delete;
    ~hdem_event_timer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int start()
    {
        for (int k = 0; on && k < N; ++k) HDEM_HIP_CHECK(hipEventCreate(&ev[k]));
        return HDEM_OK;
    }
    void mark(int k) { if (on) (void)hipEventRecord(ev[k], stream); }
    float ms(int from, int to) const   // after a synchronise; 0 when the timer is off
    {
        float t = 0.f;
        if (on) (void)hipEventElapsedTime(&t, ev[from], ev[to]);
        return t;
    }
    // the phases A, B, C between four marks; what they point at stays when the timer is off
    void read(float *ms_a, float *ms_b, float *ms_c) const
    {
        static_assert(N >= 4, "three phases take four marks");
        if (on) *ms_a = ms(0, 1), *ms_b = ms(1, 2), *ms_c = ms(2, 3);
    }
};

// The stream set of the flow trace, the stream order and the stream network: what `streams` and
// `threshold` must be for each HDEM_FT_STREAMS_* kind.
inline int d8_check_streams(const void *streams, int stream_kind, uint32_t threshold)
{
    switch (stream_kind) {
    case HDEM_FT_STREAMS_NONE:
        HDEM_REQUIRE(!streams && !threshold, HDEM_ERR_BAD_ARG,
                     "streams and threshold must be null and 0 with HDEM_FT_STREAMS_NONE");
        break;
    case HDEM_FT_STREAMS_MASK_U8:
        HDEM_REQUIRE(streams, HDEM_ERR_BAD_ARG, "the stream mask is null");
        HDEM_REQUIRE(!threshold, HDEM_ERR_BAD_ARG,
                     "a uint8 stream mask takes no threshold (got %u)", threshold);
        break;
    case HDEM_FT_STREAMS_ACC_U32:
        HDEM_REQUIRE(streams, HDEM_ERR_BAD_ARG, "the stream raster is null");
        HDEM_REQUIRE(threshold >= 1, HDEM_ERR_BAD_ARG,
                     "a uint32 stream raster needs a threshold >= 1");
        break;
    default:
        HDEM_REQUIRE(false, HDEM_ERR_BAD_ARG, "unknown stream kind %d", stream_kind);
    }
    return HDEM_OK;
}

// What the caller's stats struct has room for (its struct_size) is filled, and nothing beyond.
template <class Stats>
inline void d8_publish(Stats *stats, Stats st)
{
    if (!stats) return;
    st.struct_size = std::min<uint32_t>(stats->struct_size, sizeof(Stats));
    memcpy(stats, &st, st.struct_size);
}

// A stats struct that is passed holds at least its struct_size; `name` is the struct's.
template <class Stats>
inline int d8_check_stats(const Stats *stats, const char *name)
{
    HDEM_REQUIRE(!stats || stats->struct_size >= sizeof(uint32_t), HDEM_ERR_BAD_ARG,
                 "%s.struct_size is %u: set it to sizeof(%s)", name,
                 stats ? stats->struct_size : 0u, name);
    return HDEM_OK;
}

// The pointer-jumping forest: ceil(log2 nslots) + 1 launches (a round at least halves every
// chain) of `grid` workgroups of nt threads, grid-stride.
struct d8_forest_plan {
    int rounds, grid;
};
inline d8_forest_plan d8_forest_plan_of(const hdem_ctx *ctx, int64_t nslots, int nt)
{
    d8_forest_plan p = {1, 0};
    while ((1ll << (p.rounds - 1)) < nslots) ++p.rounds;
    p.grid = (int)std::min<int64_t>((nslots + nt - 1) / nt, (int64_t)ctx->num_cus * 8);
    return p;
}
// the launches that had work: a launch whose predecessor left nothing returned at once
inline int d8_forest_rounds(const d8_forest_plan &p, const d8_forest_counters &host)
{
    int r = 1;
    while (r < p.rounds && host.unresolved[r - 1]) ++r;
    return r;
}

// hdem_flowtrace.hip: the bytes hdem_flowtrace_u8_dev takes from the head of the arena, for
// an operator that calls it and keeps views of its own behind them
size_t hdem_flowtrace_arena_bytes(int64_t tiles, int64_t nslots);

inline int d8_report_invalid(unsigned long long bad)
{
    HDEM_REQUIRE(!bad, HDEM_ERR_BAD_ARG,
                 "invalid D8 code in %llu cells: a code is 0 or one of 1, 2, 4, ..., 128", bad);
    return HDEM_OK;
}
// invalid codes, then what the pointer jumping never resolved
inline int d8_report_forest(const d8_forest_counters &host)
{
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.stuck_cells && !host.stuck_slots, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu cells never resolve (and %llu tile "
                 "perimeter slots)",
                 host.stuck_cells, host.stuck_slots);
    return HDEM_OK;
}
