// The stream network as a table: one record per link (new operator; StreamNetwork,
// DemToStreamNetwork).
//
// In: the codes, the stream set S and the link raster of hdem_streamorder_u8 (link[c] = 1 + the
// flat index of the last cell, the *end*, of c's link), K = the number of links, and, as the
// columns ask for them, the order and magnitude rasters and a dem.  The links are numbered
// 0 ... K - 1 in ascending flat index of their end; row r of every column describes link r.
//   1  (streamnet_ends_kernel, hdem_scan.h)  ends and ranks.  One bit per cell "is its own
//      end" in 64-cell words (a tile row is a wave: one ballot), the count per word, an
//      exclusive scan of the counts; rank of an end = scanned count of its word + popcount of
//      the bits in front of it.  The scan, the rank lookup and the table's views are the shared
//      ones of hdem_scan.h.
//   2  hdem_flowtrace_u8_dev with the caller's streams and `stop` alone: the first stream cell
//      of every cell.  Only when `catchment` is wanted, and not when every cell is a stream
//      cell (a cell is then its own first stream cell and there is nothing to trace).
//   3  (streamnet_tile_kernel)  per 64 x 64 tile: codes, membership and link ids with a one-cell
//      halo in LDS; nin and the link id of a cell's one donor from the halo.  Every cell adds to
//      one row at most: a stream cell 1 to `cells`, its step to `ncard` or `ndiag` when its
//      receiver is in S, and 1 to `catchment`; a cell off the streams 1 to the `catchment` of
//      its first stream cell's row.  The adds are gathered per row in an LDS table (open
//      addressing, 4 096 slots >= the rows a tile can touch, two packed 16-bit counters per
//      word: a tile adds at most 4 096 to any of them), then one global atomic add per (tile,
//      row, column) that is not zero.  The one cell of a link with nin != 1 stores `top` and
//      `z_top`.  Writes `row`.  Every check of the link raster that a cell can make on its
//      neighbourhood is made here and counted.
//   4  (streamnet_end_kernel / streamnet_end_sparse_kernel, streamnet_length_kernel)  the ends
//      of every word of the bitmap, a wave per word and a lane per cell where there are many,
//      else a thread per word: `end`, `down` (the rank of the receiver's link), `order` and
//      `magnitude` gathered at the end, `z_end`; then `length` from the finished step counts.
// Integer adds, counts and gathers only: exact, identical from run to run.  No walk: the only
// loops are the table's probe (capped at the table size) and the flow trace's.  A rank is
// compared with K before it indexes a column, so a K that is too small writes nowhere.
// Workspace (arena): 12 B per 64 cells (bitmap + counts), 4 B per cell for the first stream
// cells behind the flow trace's own bytes when step 2 runs, 8 B per link when `length` is
// wanted without `ncard` and `ndiag`.
#include "hdem_d8tile.h"
#include "hdem_scan.h"

#include <cmath>

namespace {

constexpr int NT = 256;               // threads per workgroup, all kernels but the scan's one
constexpr int HL = TS + 2;            // staged rasters: the tile and one ring
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int SLOTS = 4096;           // table slots of the tile kernel: a cell adds to one row
constexpr size_t HEAD = 256;          // bytes of the counter block

struct streamnet_counters {
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long foreign;       // cells whose link id fails a check
    unsigned long long ends;          // cells with link[c] == 1 + c
    unsigned long long tops;          // stream cells with nin != 1
    unsigned long long stream_cells;
    unsigned long long reached;       // cells with a first stream cell
    unsigned long long capped;        // table inserts that found no slot
};
static_assert(sizeof(streamnet_counters) <= HEAD, "counters outgrew their block");

template <int STREAMS>
__device__ __forceinline__ bool in_streams(const void *__restrict__ streams, uint32_t threshold,
                                           size_t g)
{
    if (STREAMS == 1) return static_cast<const uint8_t *>(streams)[g] != 0;
    if (STREAMS == 2) return static_cast<const uint32_t *>(streams)[g] >= threshold;
    return true;
}

// 1.  bits[y * tiles_x + tx]: which cells of that tile row are ends, and how many.
__global__ __launch_bounds__(NT) void streamnet_ends_kernel(int H, int W, int tiles_x,
                                                            const uint32_t *__restrict__ link,
                                                            unsigned long long *__restrict__ bits,
                                                            uint32_t *__restrict__ count,
                                                            streamnet_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_ends;
    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    if (tid == 0) s_ends = 0;
    __syncthreads();
    unsigned int ends = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (ly >= tile.th) break;                // (whole waves: a wave is a row)
        bool end = false;
        if (lx < tile.tw) {
            const size_t g = (size_t)(tile.y0 + ly) * W + tile.x0 + lx;
            end = link[g] == (uint32_t)g + 1u;
        }
        const unsigned long long m = __ballot(end);
        if (lx == 0) {
            const size_t w = (size_t)(tile.y0 + ly) * tiles_x + tile.tx;
            bits[w] = m;
            count[w] = (uint32_t)__popcll(m);
            ends += (unsigned int)__popcll(m);
        }
    }
    if (ends) atomicAdd(&s_ends, ends);
    __syncthreads();
    if (tid == 0 && s_ends) atomicAdd(&cnt->ends, (unsigned long long)s_ends);
}

// The row of link id l (1 + flat index of its end), or false: l is 0, points outside the
// raster or at a cell that is not its own end, or its rank is not below K.
__device__ __forceinline__ bool row_of(uint32_t l, uint32_t cells, int W, int tiles_x, uint32_t K,
                                       const unsigned long long *__restrict__ bits,
                                       const uint32_t *__restrict__ before, uint32_t &r)
{
    if (l == 0u || l - 1u >= cells) return false;
    const uint32_t e = l - 1u;
    const uint32_t ey = e / (uint32_t)W, ex = e - ey * (uint32_t)W;
    return hdem_rank_of(bits, before, (size_t)ey * tiles_x + ex / TS, (int)(ex % TS), K, r);
}

// 3.  STREAMS as in hdem_streamorder.hip.  first: 1 + the first stream cell of every cell, or
// null; catchment is gathered when the column is not null (STREAMS == 0 needs no first).
template <int STREAMS>
__global__ __launch_bounds__(NT) void streamnet_tile_kernel(
    const uint8_t *__restrict__ d8, const void *__restrict__ streams, uint32_t threshold,
    const uint32_t *__restrict__ link, const uint32_t *__restrict__ first,
    const float *__restrict__ dem, int H, int W, int tiles_x, uint32_t K,
    const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ before,
    uint32_t *__restrict__ top, float *__restrict__ z_top, uint32_t *cells_col, uint32_t *ncard,
    uint32_t *ndiag, uint32_t *catchment, uint32_t *__restrict__ row,
    streamnet_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[HL * HL];
    __shared__ uint8_t strm[HL * HL];
    __shared__ uint32_t lnk[HL * HL];
    __shared__ uint32_t s_key[SLOTS];            // 1 + row
    __shared__ uint32_t s_a[SLOTS];              // cells | ncard << 16
    __shared__ uint32_t s_b[SLOTS];              // ndiag | catchment << 16
    __shared__ unsigned int s_cnt[6];            // bad, foreign, tops, stream, reached, capped

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;
    const uint32_t ncells = (uint32_t)((int64_t)H * W);

    if (tid < 6) s_cnt[tid] = 0;
    for (int s = tid; s < SLOTS; s += NT) s_key[s] = 0u, s_a[s] = 0u, s_b[s] = 0u;
    for (int i = tid; i < HL * HL; i += NT) {
        const int gy = y0 + i / HL - 1, gx = x0 + i % HL - 1;
        uint8_t c = 0, s = 0;
        uint32_t l = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = (size_t)gy * W + gx;
            c = d8[g];
            s = in_streams<STREAMS>(streams, threshold, g);
            l = link[g];
        }
        code[i] = c;
        strm[i] = s;
        lnk[i] = l;
    }
    __syncthreads();

    unsigned int bad = 0, foreign = 0, tops = 0, stream_cells = 0, reached = 0, capped = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        const int at = (ly + 1) * HL + lx + 1;
        const d8_step s = d8_decode(code[at], ly, lx, tile, H, W);
        bad += s.invalid;
        const uint32_t l = lnk[at];
        uint32_t key = 0, a = 0, b = 0;          // what the cell adds, and to which row + 1
        if (!strm[at]) {
            foreign += l != 0u;
            if (catchment && first) {
                const uint32_t f = first[g];
                if (f) {
                    ++reached;
                    uint32_t r;
                    if (row_of(link[f - 1u], ncells, W, tiles_x, K, bits, before, r))
                        key = r + 1u, b = 1u << 16;
                    else
                        ++foreign;
                }
            }
        } else {
            ++stream_cells;
            reached += catchment != nullptr;
            int n = 0;
            uint32_t donor = 0;                  // the link id of the one donor when n == 1
            for (int k = 0; k < 8; ++k) {
                const int d = at - (code_dy(k) * HL + code_dx(k));   // the neighbour against k
                if (code[d] == (1 << k) && strm[d]) ++n, donor = lnk[d];
            }
            tops += n != 1;
            const int rat = (s.ny + 1) * HL + s.nx + 1;
            const bool to_stream = !s.terminal && strm[rat];
            uint32_t r;
            bool ok = row_of(l, ncells, W, tiles_x, K, bits, before, r);
            // a cell that is no end hands its id on; a cell with one donor took its id over
            if (ok && l != (uint32_t)g + 1u) ok = to_stream && lnk[rat] == l;
            if (ok && n == 1) ok = donor == l;
            if (!ok) {
                ++foreign;
            } else {
                key = r + 1u;
                a = 1u;
                if (to_stream) {
                    if (s.b & 1) b = 1u;
                    else a += 1u << 16;
                }
                if (catchment) b += 1u << 16;
                if (n != 1) {
                    if (top) top[r] = (uint32_t)g;
                    if (z_top) z_top[r] = dem[g];
                }
            }
        }
        if (row) row[g] = strm[at] ? key : 0u;
#ifdef HDEM_STREAMNET_PLAIN
        // the comparison build of DESIGN 3.17: no table, global atomics cell by cell
        if (key) {
            const size_t r = key - 1u;
            if (cells_col && (a & 0xFFFFu)) atomicAdd(&cells_col[r], a & 0xFFFFu);
            if (ncard && (a >> 16)) atomicAdd(&ncard[r], a >> 16);
            if (ndiag && (b & 0xFFFFu)) atomicAdd(&ndiag[r], b & 0xFFFFu);
            if (catchment && (b >> 16)) atomicAdd(&catchment[r], b >> 16);
        }
#else
        if (key) {
            uint32_t slot = (key * 2654435761u) >> 20;           // 12 bits
            int probe = 0;
            for (; probe < SLOTS; ++probe) {
                const uint32_t seen = atomicCAS(&s_key[slot], 0u, key);
                if (seen == 0u || seen == key) break;
                slot = (slot + 1) & (SLOTS - 1);
            }
            if (probe < SLOTS) {
                if (a) atomicAdd(&s_a[slot], a);
                if (b) atomicAdd(&s_b[slot], b);
            } else {                             // more rows than cells: not from this kernel
                ++capped;
            }
        }
#endif
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (foreign) atomicAdd(&s_cnt[1], foreign);
    if (tops) atomicAdd(&s_cnt[2], tops);
    if (stream_cells) atomicAdd(&s_cnt[3], stream_cells);
    if (reached) atomicAdd(&s_cnt[4], reached);
    if (capped) atomicAdd(&s_cnt[5], capped);
    __syncthreads();

    // one global atomic per (tile, row) and column that the tile adds to; key - 1 < K
    for (int s = tid; s < SLOTS; s += NT) {
        const uint32_t key = s_key[s];
        if (!key) continue;
        const size_t r = key - 1u;
        const uint32_t a = s_a[s], b = s_b[s];
        if (cells_col && (a & 0xFFFFu)) atomicAdd(&cells_col[r], a & 0xFFFFu);
        if (ncard && (a >> 16)) atomicAdd(&ncard[r], a >> 16);
        if (ndiag && (b & 0xFFFFu)) atomicAdd(&ndiag[r], b & 0xFFFFu);
        if (catchment && (b >> 16)) atomicAdd(&catchment[r], b >> 16);
    }
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->foreign, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->tops, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->stream_cells, (unsigned long long)s_cnt[3]);
        if (s_cnt[4]) atomicAdd(&cnt->reached, (unsigned long long)s_cnt[4]);
        if (s_cnt[5]) atomicAdd(&cnt->capped, (unsigned long long)s_cnt[5]);
    }
}

// 4.  The columns read off the end cell (y, x) of row r < K.
struct streamnet_end_args {
    int H, W, tiles_x;
    uint32_t K;
    const uint8_t *d8;
    const void *streams;
    uint32_t threshold;
    const uint32_t *link;
    const uint8_t *order_in;
    const uint32_t *magnitude_in;
    const float *dem;
    const unsigned long long *bits;
    const uint32_t *before;
    uint32_t *end, *down;
    uint8_t *order;
    uint32_t *magnitude;
    float *z_end;
    streamnet_counters *cnt;
};

template <int STREAMS>
__device__ __forceinline__ void end_row(const streamnet_end_args &a, uint32_t r, int y, int x)
{
    const size_t e = (size_t)y * a.W + x;
    if (a.end) a.end[r] = (uint32_t)e;
    if (a.down) {
        uint32_t to = NONE;
        const uint32_t c = a.d8[e];
        if (c && !(c & (c - 1u))) {
            const int k = __builtin_ctz(c);
            const int ny = y + code_dy(k), nx = x + code_dx(k);
            if (ny >= 0 && ny < a.H && nx >= 0 && nx < a.W) {
                const size_t j = (size_t)ny * a.W + nx;
                if (in_streams<STREAMS>(a.streams, a.threshold, j) &&
                    !row_of(a.link[j], (uint32_t)((int64_t)a.H * a.W), a.W, a.tiles_x, a.K, a.bits,
                            a.before, to)) {
                    to = NONE;
                    atomicAdd(&a.cnt->foreign, 1ull);
                }
            }
        }
        a.down[r] = to;
    }
    if (a.order) a.order[r] = a.order_in[e];
    if (a.magnitude) a.magnitude[r] = a.magnitude_in[e];
    if (a.z_end) a.z_end[r] = a.dem[e];
}

// The ends of word w have the ranks before[w], before[w] + 1, ...  Two forms, chosen by the host
// on K against the number of words.  Many ends per word: one wave per word, one lane per cell of
// it (TS is the wave size), so that a wave's stores to a column are contiguous.
template <int STREAMS>
__global__ __launch_bounds__(NT) void streamnet_end_kernel(int64_t words, streamnet_end_args a)
{
    static_assert(TS == 64, "a bitmap word is a wave");
    const int64_t w = (int64_t)blockIdx.x * (NT / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (w >= words) return;
    const unsigned long long m = a.bits[w];
    if (!((m >> lane) & 1ull)) return;
    const uint32_t r = hdem_rank_in(m, lane, a.before[w]);
    if (r >= a.K) return;                        // (more ends than K: counted, refused)
    end_row<STREAMS>(a, r, (int)(w / a.tiles_x), (int)(w % a.tiles_x) * TS + lane);
}

// Few ends per word: one thread per word walks its set bits; 64 times fewer threads, most of
// which find an empty word.
template <int STREAMS>
__global__ __launch_bounds__(NT) void streamnet_end_sparse_kernel(int64_t words,
                                                                  streamnet_end_args a)
{
    const int64_t w = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (w >= words) return;
    unsigned long long m = a.bits[w];
    if (!m) return;
    const int y = (int)(w / a.tiles_x), x0 = (int)(w % a.tiles_x) * TS;
    for (uint32_t r = a.before[w]; m && r < a.K; m &= m - 1ull, ++r)
        end_row<STREAMS>(a, r, y, x0 + __builtin_ctzll(m));
}

// cs2 = cellsize * sqrt(2), in double: the flow trace's distance formula
__global__ __launch_bounds__(NT) void streamnet_length_kernel(uint32_t K,
                                                              const uint32_t *__restrict__ ncard,
                                                              const uint32_t *__restrict__ ndiag,
                                                              double cs, double cs2,
                                                              float *__restrict__ length)
{
    const uint32_t r = blockIdx.x * NT + threadIdx.x;
    if (r < K)
        length[r] = __double2float_rn(__dadd_rn(__dmul_rn((double)ncard[r], cs),
                                                __dmul_rn((double)ndiag[r], cs2)));
}

// the operands and outputs of a call, as both forms take them
struct streamnet_call {
    const uint8_t *d8;
    int H, W;
    const void *streams;
    int stream_kind;
    uint32_t threshold;
    const uint32_t *link;
    const uint8_t *order_in;
    const uint32_t *magnitude_in;
    const float *dem;
    double cellsize;
    int64_t K;
    uint32_t *end, *top, *down;
    uint8_t *order;
    uint32_t *magnitude, *cells, *ncard, *ndiag;
    float *length;
    uint32_t *catchment;
    float *z_top, *z_end;
    uint32_t *row;
    int flags;
    hdem_streamlinks_stats *stats;
};

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const streamnet_call &a, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, a.d8, a.d8, a.H, a.W)) return rc;
    if (int rc = d8_grid_of("the stream network", a.H, a.W, g)) return rc;
    HDEM_REQUIRE(!a.flags, HDEM_ERR_BAD_ARG, "unknown stream network flags 0x%x", a.flags);
    HDEM_REQUIRE(a.link, HDEM_ERR_BAD_ARG, "the link raster is null");
    if (int rc = d8_check_streams(a.streams, a.stream_kind, a.threshold)) return rc;
    HDEM_REQUIRE(std::isfinite(a.cellsize) && a.cellsize > 0.0, HDEM_ERR_BAD_ARG,
                 "cellsize must be finite and positive, got %g", a.cellsize);
    HDEM_REQUIRE(a.K >= 0 && a.K <= (int64_t)a.H * a.W, HDEM_ERR_BAD_ARG,
                 "K is the number of links, 0 ... H * W: got %lld", (long long)a.K);
    HDEM_REQUIRE((!a.z_top && !a.z_end) || a.dem, HDEM_ERR_BAD_ARG,
                 "z_top and z_end need the dem they are read from");
    HDEM_REQUIRE(!a.order || a.order_in, HDEM_ERR_BAD_ARG,
                 "the order column needs the order raster");
    HDEM_REQUIRE(!a.magnitude || a.magnitude_in, HDEM_ERR_BAD_ARG,
                 "the magnitude column needs the magnitude raster");
    HDEM_REQUIRE(a.end || a.top || a.down || a.order || a.magnitude || a.cells || a.ncard ||
                     a.ndiag || a.length || a.catchment || a.z_top || a.z_end || a.row,
                 HDEM_ERR_BAD_ARG, "no output wanted: give at least one column or row");
    return d8_check_stats(a.stats, "hdem_streamlinks_stats");
}

typedef hdem_event_timer<6> step_timer;   // marks around the four steps

template <int STREAMS>
void launch_tile_and_end(hdem_ctx *ctx, const streamnet_call &a, const d8_grid &g, int64_t words,
                         const uint32_t *first, const hdem_rank_table &rank, uint32_t *ncard,
                         uint32_t *ndiag, streamnet_counters *cnt, step_timer &steps)
{
    const uint32_t K = (uint32_t)a.K;
    hipLaunchKernelGGL(streamnet_tile_kernel<STREAMS>, dim3((unsigned)g.tiles), dim3(NT), 0,
                       ctx->stream, a.d8, a.streams, a.threshold, a.link, first, a.dem, a.H, a.W,
                       g.tiles_x, K, rank.bits, rank.count, a.top, a.z_top, a.cells, ncard, ndiag,
                       a.catchment, a.row, cnt);
    steps.mark(4);
    if (!(a.end || a.down || a.order || a.magnitude || a.z_end)) return;
    const streamnet_end_args e = {a.H, a.W, g.tiles_x, K, a.d8, a.streams, a.threshold, a.link,
                                  a.order_in, a.magnitude_in, a.dem, rank.bits, rank.count, a.end,
                                  a.down, a.order, a.magnitude, a.z_end, cnt};
    // measured: at 0.03 and 0.37 ends per word the thread form is 3 to 5 times
    // faster, at 34 the wave form 6 times; the crossover in between was not located
    if (a.K >= 2 * words)
        hipLaunchKernelGGL(streamnet_end_kernel<STREAMS>,
                           dim3((unsigned)((words + NT / 64 - 1) / (NT / 64))), dim3(NT), 0,
                           ctx->stream, words, e);
    else
        hipLaunchKernelGGL(streamnet_end_sparse_kernel<STREAMS>,
                           dim3((unsigned)((words + NT - 1) / NT)), dim3(NT), 0, ctx->stream,
                           words, e);
}

int streamlinks_dev(hdem_ctx *ctx, const streamnet_call &a, const d8_grid &g)
{
    const int64_t cells = (int64_t)a.H * a.W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_streamlinks_stats st = {};
    st.tile_h = TS;
    st.tile_w = TS;
    d8_publish(a.stats, st);
    if (a.K == 0) {
        if (a.row) HDEM_HIP_CHECK(hipMemsetAsync(a.row, 0, (size_t)cells * 4, ctx->stream));
        return HDEM_OK;
    }
    const size_t n = (size_t)a.K;

    // arena: the flow trace's bytes and first u32 per cell (when it runs) | counters | the rank
    // table of the end bits | ncard, ndiag u32 per link (when length is wanted and they are not)
    const bool traced = a.catchment && a.stream_kind != HDEM_FT_STREAMS_NONE;
    const size_t trace = traced ? hdem_round16(hdem_flowtrace_arena_bytes(g.tiles, g.nslots)) : 0;
    const size_t first_bytes = traced ? hdem_round16((size_t)cells * 4) : 0;
    const int64_t words = (int64_t)a.H * g.tiles_x;
    const size_t table_bytes = hdem_rank_table_bytes(words);
    const size_t col_bytes = hdem_round16(n * 4);
    const bool own_card = a.length && !a.ncard, own_diag = a.length && !a.ndiag;
    const size_t bytes = trace + first_bytes + HEAD + table_bytes + (own_card ? col_bytes : 0) +
                         (own_diag ? col_bytes : 0);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    char *at = ws + trace;
    uint32_t *first = traced ? reinterpret_cast<uint32_t *>(at) : nullptr;
    at += first_bytes;
    streamnet_counters *cnt = reinterpret_cast<streamnet_counters *>(at);
    at += HEAD;
    hdem_rank_table rank;
    hdem_rank_table_at(at, words, &rank);
    at += table_bytes;
    uint32_t *ncard = a.ncard, *ndiag = a.ndiag;
    if (own_card) ncard = reinterpret_cast<uint32_t *>(at), at += col_bytes;
    if (own_diag) ndiag = reinterpret_cast<uint32_t *>(at), at += col_bytes;

    step_timer steps(ctx, a.stats != nullptr);
    if (int rc = steps.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, HEAD, ctx->stream));
    steps.mark(0);
    hipLaunchKernelGGL(streamnet_ends_kernel, dim3((unsigned)g.tiles), dim3(NT), 0, ctx->stream,
                       a.H, a.W, g.tiles_x, a.link, rank.bits, rank.count, cnt);
    hdem_scan_exclusive(ctx->stream, rank.count, words, rank.sums);
    steps.mark(1);
    HDEM_HIP_CHECK(hipGetLastError());
    // the first stream cell of every cell; the trace takes the head of the arena, refuses
    // invalid bytes and loops that hold no stream cell, and synchronises
    if (traced) {
        if (int rc = hdem_flowtrace_u8_dev(ctx, a.d8, a.H, a.W, a.streams, a.stream_kind,
                                           a.threshold, nullptr, 1.0, first, nullptr, nullptr,
                                           nullptr, nullptr, 0, nullptr))
            return rc;
        steps.mark(2);
    }
    for (uint32_t *column : {a.cells, ncard, ndiag, a.catchment})
        if (column) HDEM_HIP_CHECK(hipMemsetAsync(column, 0, n * 4, ctx->stream));
    steps.mark(3);
    if (a.stream_kind == HDEM_FT_STREAMS_NONE)
        launch_tile_and_end<0>(ctx, a, g, words, first, rank, ncard, ndiag, cnt, steps);
    else if (a.stream_kind == HDEM_FT_STREAMS_MASK_U8)
        launch_tile_and_end<1>(ctx, a, g, words, first, rank, ncard, ndiag, cnt, steps);
    else
        launch_tile_and_end<2>(ctx, a, g, words, first, rank, ncard, ndiag, cnt, steps);
    if (a.length)
        hipLaunchKernelGGL(streamnet_length_kernel, dim3((unsigned)((a.K + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, (uint32_t)a.K, ncard, ndiag, a.cellsize,
                           a.cellsize * std::sqrt(2.0), a.length);
    steps.mark(5);
    HDEM_HIP_CHECK(hipGetLastError());
    streamnet_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.links = (int64_t)host.ends;
    st.stream_cells = (int64_t)host.stream_cells;
    st.catchment_cells = (int64_t)host.reached;
    st.tops = (int64_t)host.tops;
    st.ms_rank = steps.ms(0, 1);
    st.ms_trace = traced ? steps.ms(1, 2) : 0.f;
    st.ms_tile = steps.ms(3, 4);
    st.ms_final = steps.ms(4, 5);
    d8_publish(a.stats, st);
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.foreign, HDEM_ERR_BAD_ARG,
                 "the links do not belong to these codes and streams: %llu cells", host.foreign);
    HDEM_REQUIRE((int64_t)host.ends == a.K && (int64_t)host.tops == a.K, HDEM_ERR_BAD_ARG,
                 "the links do not belong to these codes and streams: %llu ends and %llu first "
                 "cells for K = %lld",
                 host.ends, host.tops, (long long)a.K);
    HDEM_REQUIRE(!host.capped, HDEM_ERR_NOT_CONVERGED,
                 "stream network: %llu cells found no slot in their tile's table", host.capped);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_streamlinks_u8_dev(
    hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams, int stream_kind,
    uint32_t threshold, const uint32_t *link, const uint8_t *order_raster,
    const uint32_t *magnitude_raster, const float *dem, double cellsize, int64_t K, uint32_t *end,
    uint32_t *top, uint32_t *down, uint8_t *order, uint32_t *magnitude, uint32_t *cells,
    uint32_t *ncard, uint32_t *ndiag, float *length, uint32_t *catchment, float *z_top,
    float *z_end, uint32_t *row, int flags, hdem_streamlinks_stats *stats)
{
    const streamnet_call a = {d8, H, W, streams, stream_kind, threshold, link, order_raster,
                              magnitude_raster, dem, cellsize, K, end, top, down, order, magnitude,
                              cells, ncard, ndiag, length, catchment, z_top, z_end, row, flags,
                              stats};
    d8_grid g;
    if (int rc = check_args(ctx, a, &g)) return rc;
    return streamlinks_dev(ctx, a, g);
}

extern "C" int hdem_streamlinks_u8(
    hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams, int stream_kind,
    uint32_t threshold, const uint32_t *link, const uint8_t *order_raster,
    const uint32_t *magnitude_raster, const float *dem, double cellsize, int64_t K, uint32_t *end,
    uint32_t *top, uint32_t *down, uint8_t *order, uint32_t *magnitude, uint32_t *cells,
    uint32_t *ncard, uint32_t *ndiag, float *length, uint32_t *catchment, float *z_top,
    float *z_end, uint32_t *row, int flags, hdem_streamlinks_stats *stats)
{
    streamnet_call a = {d8, H, W, streams, stream_kind, threshold, link, order_raster,
                        magnitude_raster, dem, cellsize, K, end, top, down, order, magnitude,
                        cells, ncard, ndiag, length, catchment, z_top, z_end, row, flags, stats};
    d8_grid g;
    if (int rc = check_args(ctx, a, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W, k = (size_t)K;
    hdem_dbuf dd8, dstreams, dlink, dorder, dmagnitude, ddem, dout[13];
    const size_t sb = n * (stream_kind == HDEM_FT_STREAMS_ACC_U32 ? sizeof(uint32_t) : 1);
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dstreams.upload(ctx, streams, sb)) return rc;
    if (int rc = dlink.upload(ctx, link, n * 4)) return rc;
    if (int rc = dorder.upload(ctx, order_raster, n)) return rc;
    if (int rc = dmagnitude.upload(ctx, magnitude_raster, n * 4)) return rc;
    if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
    // the twelve columns in the ABI's order, then row
    void *const host_out[13] = {end, top, down, order, magnitude, cells, ncard, ndiag, length,
                                catchment, z_top, z_end, row};
    size_t out_bytes[13];
    for (int c = 0; c < 12; ++c) out_bytes[c] = k * (c == 3 ? 1 : 4);
    out_bytes[12] = n * 4;
    for (int c = 0; c < 13; ++c)
        if (host_out[c] && out_bytes[c])
            if (int rc = dout[c].alloc(ctx, out_bytes[c])) return rc;
    a.d8 = dd8.as<const uint8_t>();
    a.streams = dstreams.p;
    a.link = dlink.as<const uint32_t>();
    a.order_in = dorder.as<const uint8_t>();
    a.magnitude_in = dmagnitude.as<const uint32_t>();
    a.dem = ddem.as<const float>();
    a.end = dout[0].as<uint32_t>(), a.top = dout[1].as<uint32_t>();
    a.down = dout[2].as<uint32_t>(), a.order = dout[3].as<uint8_t>();
    a.magnitude = dout[4].as<uint32_t>(), a.cells = dout[5].as<uint32_t>();
    a.ncard = dout[6].as<uint32_t>(), a.ndiag = dout[7].as<uint32_t>();
    a.length = dout[8].as<float>(), a.catchment = dout[9].as<uint32_t>();
    a.z_top = dout[10].as<float>(), a.z_end = dout[11].as<float>();
    a.row = dout[12].as<uint32_t>();
    if (int rc = streamlinks_dev(ctx, a, g)) return rc;
    for (int c = 0; c < 13; ++c)
        if (dout[c].p)
            if (int rc = dout[c].download(host_out[c], out_bytes[c])) return rc;
    return HDEM_OK;
}
