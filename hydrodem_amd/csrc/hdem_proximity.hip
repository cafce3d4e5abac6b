// A15  Proximity: the exact Euclidean distance transform of a source set, the nearest source of
// every cell under the smallest-flat-index tie rule, and the rasters built on it
// (include/hydrodem_hip.h has the contract).
//
// The transform is separable, and every comparison in it is between integers.  A row pass
// finds for every cell the nearest source of its own row, ties to the left; a column pass then
// finds for every cell (r, x) the row r' that minimises (r - r')^2 + g(r', x)^2, g being the
// row pass's distance, ties to the smaller r'.  With those two tie rules the winner is the
// source with the smallest flat index among the nearest, and the argmin of the column pass is
// monotone along the column, which is what bounds its cost.  Five launches:
//
//   bits     one wave per 64 x 64 cells: the source flags of a row segment as one ballot word,
//            kept [chunk][row], and the count of S.  The only kernel that reads `sources`.
//   carry    one thread per row over the row's words: for every chunk the last source column
//            to its left and the first to its right (uint16, [chunk][row], 0xFFFF: none).
//   row      one workgroup per 64 x 64 tile: a lane takes the nearest set bit on either side
//            from the word, or the carry where the word has none, picks the nearer (the left
//            one in a tie) and the tile goes through LDS to be stored COLUMN-MAJOR: XS[x][r] is
//            the source column, so that the column pass reads and writes whole lines.
//   column   one workgroup per column x.  Divide and conquer on the monotone argmin: the rows
//            are the nodes 1 ... P - 1 of a complete binary tree (P the power of two above H),
//            level by level; a node between two solved neighbours searches only between their
//            argmins, so a level costs at most H + 2^level evaluations and the line
//            O(H log H), whatever the sources are.  A level with fewer nodes than threads is
//            searched by teams of up to 64 lanes (a strided scan, then a shuffle minimum on
//            (cost, r')); from 256 nodes on a thread owns a node.  Up to PX_LDS_LINE rows the
//            line's distances live in LDS (2 bytes per row); past that the same code reads
//            them from the global line, where the lanes of a team still touch neighbouring
//            bytes.  The argmins are read and written in AR[x][r], the nearest row, itself.
//   final    one workgroup per 64 x 64 tile: AR and XS[x][AR] are read along the lines, packed
//            and transposed through LDS, and every wanted output is written row-major from
//            (d2, nearest) in this one launch; counts the cells out of reach.
//
// Scratch, all from the context's arena: XS and AR, 2 bytes per cell each, plus 8 + 2 + 2 bytes
// per 64 cells of words and carries and two counters: 4.19 bytes per cell.  Every byte of it
// that is read was written by an earlier launch of the same call.
#include "hdem_d8tile.h"

#include <cmath>

namespace {

constexpr int NT = 256;                       // threads per workgroup, every kernel
constexpr int PX_TILE = 64;                   // tile edge of bits, row and final; a chunk
constexpr int PX_LDS_LINE = 16384;            // rows a column keeps in LDS: 2 B each, 32 KiB
constexpr uint32_t NONE16 = 0xFFFFu;          // no source: in XS, in a carry
constexpr uint32_t PX_INF = 0xFFFFFFFFu;      // cost of a row without sources; d2 out of reach
constexpr int PX_PITCH = PX_TILE + 2;         // uint16 tile: lanes 33 dwords apart
constexpr int PX_PITCH32 = PX_TILE + 1;       // uint32 tile

enum { O_D2, O_NEAREST, O_LABEL, O_DISTANCE, O_RISE, O_BURNED, O_COUNT };
enum { C_SOURCES, C_UNREACHED, C_COUNT };

struct px_grid {
    int bands, chunks, hp;                    // 64-row bands, 64-column chunks, bands * 64
};

template <int KIND>
__device__ __forceinline__ bool is_source(const void *src, size_t at, uint32_t threshold)
{
    if (KIND == HDEM_FT_STREAMS_MASK_U8) return static_cast<const uint8_t *>(src)[at] != 0;
    const uint32_t v = static_cast<const uint32_t *>(src)[at];
    return KIND == HDEM_FT_STREAMS_ACC_U32 ? v >= threshold : v != 0;
}

// ---------------------------------------------------------------------------
// bits: words[chunk * hp + row], every row below hp written
// ---------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(NT) void bits_kernel(const void *src, uint32_t threshold, int H,
                                                  int W, px_grid g, int groups,
                                                  unsigned long long *words,
                                                  unsigned long long *cnt)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int band = blockIdx.x / groups, chunk = (blockIdx.x % groups) * 4 + wave;
    if (chunk >= g.chunks) return;
    const int y0 = band * PX_TILE, x = chunk * PX_TILE + lane;
    unsigned long long mine = 0;
    for (int i = 0; i < PX_TILE; ++i) {
        const int y = y0 + i;
        const bool in = y < H && x < W && is_source<KIND>(src, (size_t)y * W + x, threshold);
        const unsigned long long word = __ballot(in);
        if (lane == i) mine = word;
    }
    words[(size_t)chunk * g.hp + y0 + lane] = mine;
    unsigned int n = __popcll(mine);
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
    if (lane == 0 && n) atomicAdd(&cnt[C_SOURCES], (unsigned long long)n);
}

// ---------------------------------------------------------------------------
// carry: left[chunk * hp + row], right[...]: the nearest source column outside the chunk
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void carry_kernel(const unsigned long long *words, px_grid g,
                                                   uint16_t *left, uint16_t *right)
{
    const int row = blockIdx.x * NT + threadIdx.x;
    if (row >= g.hp) return;
    uint32_t at = NONE16;
    for (int k = 0; k < g.chunks; ++k) {
        const size_t i = (size_t)k * g.hp + row;
        left[i] = (uint16_t)at;
        const unsigned long long w = words[i];
        if (w) at = k * PX_TILE + 63 - __clzll(w);
    }
    at = NONE16;
    for (int k = g.chunks - 1; k >= 0; --k) {
        const size_t i = (size_t)k * g.hp + row;
        right[i] = (uint16_t)at;
        const unsigned long long w = words[i];
        if (w) at = k * PX_TILE + __ffsll(w) - 1;
    }
}

// ---------------------------------------------------------------------------
// row: XS[x * H + r] = column of the nearest source of row r, ties to the left
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void row_kernel(const unsigned long long *words,
                                                 const uint16_t *left, const uint16_t *right,
                                                 int H, int W, px_grid g, uint16_t *xs)
{
    __shared__ uint16_t t[PX_TILE * PX_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int band = blockIdx.x / g.chunks, chunk = blockIdx.x % g.chunks;
    const int y0 = band * PX_TILE, x0 = chunk * PX_TILE;
    for (int k = 0; k < 16; ++k) {
        const int ly = wave * 16 + k;
        const size_t i = (size_t)chunk * g.hp + y0 + ly;
        const unsigned long long w = words[i];
        const unsigned long long below = w & (~0ull >> (63 - lane)), above = w & (~0ull << lane);
        const uint32_t l = below ? x0 + 63 - __clzll(below) : left[i];
        const uint32_t r = above ? x0 + __ffsll(above) - 1 : right[i];
        const uint32_t x = x0 + lane;
        uint32_t pick;
        if (l == NONE16) pick = r;
        else if (r == NONE16) pick = l;
        else pick = x - l <= r - x ? l : r;
        t[lane * PX_PITCH + ly] = (uint16_t)pick;
    }
    __syncthreads();
    const int y = y0 + lane;
    for (int k = 0; k < 16; ++k) {
        const int lx = wave * 16 + k, x = x0 + lx;
        if (x < W && y < H) xs[(size_t)x * H + y] = t[lx * PX_PITCH + lane];
    }
}

// ---------------------------------------------------------------------------
// column: AR[x * H + r] = the row r' that minimises (r - r')^2 + (x - XS[x][r'])^2, ties to the
// smaller r'.  A line without any source keeps valid rows (the final launch reads XS there).
// ---------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(NT) void column_kernel(const uint16_t *xs, uint16_t *ar, int H,
                                                    int levels)
{
    extern __shared__ uint16_t g[];           // LDS: the row pass's distances of the line
    const int x = blockIdx.x, tid = threadIdx.x;
    const uint16_t *line = xs + (size_t)x * H;
    // the argmins are read where they are written: in the global line, which every wave of the
    // workgroup sees after the level's barrier (kept in LDS too they halve the occupancy of a
    // long column and win nothing on a short one, section 3.20 of DESIGN)
    uint16_t *arg = ar + (size_t)x * H;
    if (LDS) {
        for (int r = tid; r < H; r += NT) {
            const uint32_t xp = line[r];
            g[r] = (uint16_t)(xp == NONE16 ? NONE16 : xp > (uint32_t)x ? xp - x : x - xp);
        }
        __syncthreads();
    }
    const int P = 1 << levels;
    for (int lv = 0; lv < levels; ++lv) {
        const int half = P >> (lv + 1), nodes = 1 << lv;
        const int shift = lv >= 8 ? 0 : lv <= 2 ? 6 : 8 - lv;      // log2 of the team's lanes
        const int team = tid >> shift, tl = tid & ((1 << shift) - 1), teams = NT >> shift;
        for (int j = team; j < nodes; j += teams) {
            const int q = (2 * j + 1) * half, r = q - 1;
            if (r >= H) break;
            const int lo = q - half >= 1 ? arg[q - half - 1] : 0;
            const int hi = q + half <= H ? arg[q + half - 1] : H - 1;
            uint32_t best = PX_INF, at = lo;
            for (int rp = lo + tl; rp <= hi; rp += 1 << shift) {
                uint32_t gv;
                if (LDS) {
                    gv = g[rp];
                } else {
                    const uint32_t xp = line[rp];
                    gv = xp == NONE16 ? NONE16 : xp > (uint32_t)x ? xp - x : x - xp;
                }
                const uint32_t dr = r > rp ? r - rp : rp - r;
                const uint32_t c = gv == NONE16 ? PX_INF : dr * dr + gv * gv;
                if (c < best) best = c, at = rp;
            }
            for (int m = (1 << shift) >> 1; m >= 1; m >>= 1) {
                const uint32_t ob = __shfl_xor(best, m), oa = __shfl_xor(at, m);
                if (ob < best || (ob == best && oa < at)) best = ob, at = oa;
            }
            if (tl == 0) arg[r] = (uint16_t)at;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// final
// ---------------------------------------------------------------------------
struct final_args {
    const uint16_t *xs, *ar;
    const float *dem;
    const uint32_t *labels;
    uint32_t *d2, *nearest, *label;
    float *distance, *rise, *burned;
    int H, W, tiles_x;
    unsigned long long max2;          // max_distance^2, or 2^64 - 1 without one
    double cellsize;
    float buffer, inv, smooth, sharp;
    unsigned long long *cnt;
};

__global__ __launch_bounds__(NT) void final_kernel(const final_args p)
{
    __shared__ uint32_t t[PX_TILE * PX_PITCH32];
    const int H = p.H, W = p.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = (blockIdx.x / p.tiles_x) * PX_TILE, x0 = (blockIdx.x % p.tiles_x) * PX_TILE;
    {   // along the lines: lane = row
        const int y = y0 + lane;
        for (int k = 0; k < 16; ++k) {
            const int lx = wave * 16 + k, x = x0 + lx;
            uint32_t packed = NONE16;
            if (x < W && y < H) {
                const uint32_t rp = p.ar[(size_t)x * H + y];
                packed = rp << 16 | p.xs[(size_t)x * H + rp];
            }
            t[lane * PX_PITCH32 + lx] = packed;
        }
    }
    __syncthreads();
    const float nan = __builtin_nanf("");
    const int x = x0 + lane;
    unsigned int lost = 0;
    for (int k = 0; k < 16; ++k) {
        const int ly = wave * 16 + k, y = y0 + ly;
        if (y >= H) break;
        if (x >= W) continue;
        const uint32_t packed = t[ly * PX_PITCH32 + lane];
        const uint32_t rp = packed >> 16, xp = packed & 0xFFFFu;
        const uint32_t dr = (uint32_t)y > rp ? y - rp : rp - y, dx = (uint32_t)x > xp ? x - xp : xp - x;
        uint32_t d2 = dr * dr + dx * dx, near = rp * (uint32_t)W + xp;
        const bool reached = xp != NONE16 && d2 <= p.max2;
        if (!reached) d2 = near = PX_INF, ++lost;
        const size_t at = (size_t)y * W + x;
        if (p.d2) p.d2[at] = d2;
        if (p.nearest) p.nearest[at] = near;
        if (p.label) p.label[at] = reached ? p.labels[near] : 0u;
        const double root = sqrt((double)d2);
        if (p.distance) p.distance[at] = reached ? (float)(root * p.cellsize) : nan;
        if (p.rise || p.burned) {
            const float z = p.dem[at];
            if (p.rise) p.rise[at] = reached ? z - p.dem[near] : nan;
            if (p.burned) {
                const float d = (float)root;
                float b = z;
                if (reached && d < p.buffer) {
                    const float w = 1.0f - d * p.inv;
                    b = (z - p.smooth * w) - (d2 == 0 ? p.sharp : 0.0f);
                }
                p.burned[at] = b;
            }
        }
    }
    for (int m = 32; m >= 1; m >>= 1) lost += __shfl_xor(lost, m);
    if (lane == 0 && lost) atomicAdd(&p.cnt[C_UNREACHED], (unsigned long long)lost);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct span {
    const char *name;
    uintptr_t lo, hi;
};

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }
inline bool not_negative(double v) { return std::isfinite(v) && v >= 0.0; }

int check_args(const hdem_ctx *ctx, const void *sources, int kind, uint32_t threshold, int H,
               int W, const float *dem, double cellsize, double buffer, double smooth,
               double sharp, void *const (&out)[O_COUNT], const hdem_proximity_stats *stats)
{
    static const char *const names[O_COUNT] = {"d2", "nearest", "label", "distance", "rise",
                                               "burned"};
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(H > 0 && W > 0, HDEM_ERR_BAD_ARG, "raster dimensions must be positive, got %d x %d",
                 H, W);
    const int64_t cells = (int64_t)H * W;
    HDEM_REQUIRE(cells <= (int64_t)UINT32_MAX, HDEM_ERR_BAD_ARG,
                 "proximity works in uint32: %d x %d = %lld cells is more than 2^32 - 1", H, W,
                 (long long)cells);
    const uint64_t diagonal2 = (uint64_t)(H - 1) * (H - 1) + (uint64_t)(W - 1) * (W - 1);
    HDEM_REQUIRE(diagonal2 <= (uint64_t)UINT32_MAX - 1, HDEM_ERR_BAD_ARG,
                 "proximity: the squared diagonal of %d x %d is %llu, more than 2^32 - 2", H, W,
                 (unsigned long long)diagonal2);
    HDEM_REQUIRE(H <= 65535 && W <= 65535, HDEM_ERR_BAD_ARG,
                 "proximity: %d x %d has a side of more than 65535 cells", H, W);
    if (int rc = d8_check_stats(stats, "hdem_proximity_stats")) return rc;
    switch (kind) {
    case HDEM_FT_STREAMS_MASK_U8:
    case HDEM_PX_SOURCES_LABELS_U32:
        HDEM_REQUIRE(!threshold, HDEM_ERR_BAD_ARG,
                     "a source mask and a label raster take no threshold (got %u)", threshold);
        break;
    case HDEM_FT_STREAMS_ACC_U32:
        HDEM_REQUIRE(threshold >= 1, HDEM_ERR_BAD_ARG,
                     "a uint32 source raster needs a threshold >= 1");
        break;
    default:
        HDEM_REQUIRE(false, HDEM_ERR_BAD_ARG, "proximity: unknown source kind %d", kind);
    }
    HDEM_REQUIRE(sources, HDEM_ERR_BAD_ARG, "the source raster is null");
    bool any = false;
    for (int k = 0; k < O_COUNT; ++k) any |= out[k] != nullptr;
    HDEM_REQUIRE(any, HDEM_ERR_BAD_ARG, "proximity: no output wanted");
    HDEM_REQUIRE(!out[O_LABEL] || kind == HDEM_PX_SOURCES_LABELS_U32, HDEM_ERR_BAD_ARG,
                 "label needs label sources (HDEM_PX_SOURCES_LABELS_U32)");
    HDEM_REQUIRE(dem || (!out[O_RISE] && !out[O_BURNED]), HDEM_ERR_BAD_ARG,
                 "rise and burned need the dem");
    HDEM_REQUIRE(!out[O_DISTANCE] || positive(cellsize), HDEM_ERR_BAD_ARG,
                 "cellsize must be finite and positive, got %g", cellsize);
    if (out[O_BURNED]) {
        HDEM_REQUIRE(positive(buffer), HDEM_ERR_BAD_ARG,
                     "buffer must be finite and positive, got %g", buffer);
        HDEM_REQUIRE(not_negative(smooth) && not_negative(sharp), HDEM_ERR_BAD_ARG,
                     "smooth and sharp must be finite and not negative, got %g and %g", smooth,
                     sharp);
    }
    const size_t n = (size_t)cells;
    span s[2 + O_COUNT];
    int ns = 0;
    s[ns++] = {"sources", (uintptr_t)sources,
               (uintptr_t)sources + (kind == HDEM_FT_STREAMS_MASK_U8 ? n : 4 * n)};
    if (dem) s[ns++] = {"dem", (uintptr_t)dem, (uintptr_t)dem + 4 * n};
    for (int k = 0; k < O_COUNT; ++k) {
        if (!out[k]) continue;
        const span o = {names[k], (uintptr_t)out[k], (uintptr_t)out[k] + 4 * n};
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "proximity: %s overlaps %s", o.name, s[j].name);
        s[ns++] = o;
    }
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_proximity_dev(hdem_ctx *ctx, const void *sources, int source_kind,
                                  uint32_t threshold, int H, int W, const float *dem,
                                  double cellsize, uint32_t max_distance, double buffer,
                                  double smooth, double sharp, uint32_t *d2, uint32_t *nearest,
                                  uint32_t *label, float *distance, float *rise, float *burned,
                                  hdem_proximity_stats *stats)
{
    void *const out[O_COUNT] = {d2, nearest, label, distance, rise, burned};
    if (int rc = check_args(ctx, sources, source_kind, threshold, H, W, dem, cellsize, buffer,
                            smooth, sharp, out, stats))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_proximity_stats st = {};
    d8_publish(stats, st);

    px_grid g;
    g.bands = (H + PX_TILE - 1) / PX_TILE, g.chunks = (W + PX_TILE - 1) / PX_TILE;
    g.hp = g.bands * PX_TILE;
    const size_t n = (size_t)H * W, slots = (size_t)g.chunks * g.hp;
    const size_t b_words = hdem_round16(slots * 8), b_carry = hdem_round16(slots * 2);
    const size_t b_line = hdem_round16(n * 2), b_cnt = hdem_round16(C_COUNT * 8);
    char *base = static_cast<char *>(hdem_arena(ctx, b_words + 2 * b_carry + 2 * b_line + b_cnt));
    if (!base) return HDEM_ERR_OOM;
    unsigned long long *words = reinterpret_cast<unsigned long long *>(base);
    uint16_t *left = reinterpret_cast<uint16_t *>(base + b_words);
    uint16_t *right = reinterpret_cast<uint16_t *>(base + b_words + b_carry);
    uint16_t *xs = reinterpret_cast<uint16_t *>(base + b_words + 2 * b_carry);
    uint16_t *ar = reinterpret_cast<uint16_t *>(base + b_words + 2 * b_carry + b_line);
    unsigned long long *cnt =
        reinterpret_cast<unsigned long long *>(base + b_words + 2 * b_carry + 2 * b_line);

    hdem_event_timer<4> timer(ctx, stats != nullptr);
    if (int rc = timer.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, C_COUNT * 8, ctx->stream));
    timer.mark(0);
    const dim3 block(NT);
    const int groups = (g.chunks + 3) / 4;
    const dim3 bits_grid((unsigned)g.bands * groups);
    if (source_kind == HDEM_FT_STREAMS_MASK_U8)
        hipLaunchKernelGGL((bits_kernel<HDEM_FT_STREAMS_MASK_U8>), bits_grid, block, 0,
                           ctx->stream, sources, threshold, H, W, g, groups, words, cnt);
    else if (source_kind == HDEM_FT_STREAMS_ACC_U32)
        hipLaunchKernelGGL((bits_kernel<HDEM_FT_STREAMS_ACC_U32>), bits_grid, block, 0,
                           ctx->stream, sources, threshold, H, W, g, groups, words, cnt);
    else
        hipLaunchKernelGGL((bits_kernel<HDEM_PX_SOURCES_LABELS_U32>), bits_grid, block, 0,
                           ctx->stream, sources, threshold, H, W, g, groups, words, cnt);
    hipLaunchKernelGGL(carry_kernel, dim3((unsigned)((g.hp + NT - 1) / NT)), block, 0,
                       ctx->stream, words, g, left, right);
    hipLaunchKernelGGL(row_kernel, dim3((unsigned)g.bands * g.chunks), block, 0, ctx->stream,
                       words, left, right, H, W, g, xs);
    timer.mark(1);
    int levels = 1;
    while ((1 << levels) <= H) ++levels;              // P = 2^levels > H
    if (H <= PX_LDS_LINE)
        hipLaunchKernelGGL((column_kernel<true>), dim3((unsigned)W), block,
                           (size_t)((H + 1) & ~1) * 2, ctx->stream, xs, ar, H, levels);
    else
        hipLaunchKernelGGL((column_kernel<false>), dim3((unsigned)W), block, 0, ctx->stream, xs,
                           ar, H, levels);
    timer.mark(2);

    final_args p = {};
    p.xs = xs, p.ar = ar, p.dem = dem;
    p.labels = static_cast<const uint32_t *>(sources);
    p.d2 = d2, p.nearest = nearest, p.label = label;
    p.distance = distance, p.rise = rise, p.burned = burned;
    p.H = H, p.W = W, p.tiles_x = g.chunks;
    p.max2 = max_distance ? (unsigned long long)max_distance * max_distance : ~0ull;
    p.cellsize = cellsize;
    p.buffer = (float)buffer, p.inv = (float)(1.0 / buffer);
    p.smooth = (float)smooth, p.sharp = (float)sharp;
    p.cnt = cnt;
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)g.bands * g.chunks), block, 0, ctx->stream, p);
    timer.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    unsigned long long host[C_COUNT] = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.sources = (int64_t)host[C_SOURCES];
    st.unreached = (int64_t)host[C_UNREACHED];
    timer.read(&st.ms_row, &st.ms_column, &st.ms_final);
    d8_publish(stats, st);
    return HDEM_OK;
}

extern "C" int hdem_proximity(hdem_ctx *ctx, const void *sources, int source_kind,
                              uint32_t threshold, int H, int W, const float *dem, double cellsize,
                              uint32_t max_distance, double buffer, double smooth, double sharp,
                              uint32_t *d2, uint32_t *nearest, uint32_t *label, float *distance,
                              float *rise, float *burned, hdem_proximity_stats *stats)
{
    void *const out[O_COUNT] = {d2, nearest, label, distance, rise, burned};
    if (int rc = check_args(ctx, sources, source_kind, threshold, H, W, dem, cellsize, buffer,
                            smooth, sharp, out, stats))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dsrc, ddem, dout[O_COUNT];
    if (int rc = dsrc.upload(ctx, sources, source_kind == HDEM_FT_STREAMS_MASK_U8 ? n : n * 4))
        return rc;
    if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
    for (int k = 0; k < O_COUNT; ++k)
        if (out[k])
            if (int rc = dout[k].alloc(ctx, n * 4)) return rc;
    const int rc = hdem_proximity_dev(
        ctx, dsrc.p, source_kind, threshold, H, W, ddem.as<const float>(), cellsize, max_distance,
        buffer, smooth, sharp, dout[O_D2].as<uint32_t>(), dout[O_NEAREST].as<uint32_t>(),
        dout[O_LABEL].as<uint32_t>(), dout[O_DISTANCE].as<float>(), dout[O_RISE].as<float>(),
        dout[O_BURNED].as<float>(), stats);
    if (rc) return rc;
    for (int k = 0; k < O_COUNT; ++k)
        if (out[k])
            if (int rc2 = dout[k].download(out[k], n * 4)) return rc2;
    return HDEM_OK;
}
