// Strahler stream order, Shreve magnitude and stream links (new operator; StreamOrder,
// DemToStreamOrder).
//
// S is the stream set (every cell, a mask, or acc >= threshold); a stream donor of c is a
// neighbour in S whose code points at c, nin(c) their number.  A *link* is a run of stream
// cells between two junctions (cells with nin >= 2); its last cell, the *stop*, is the first
// cell b on a stream cell's D8 path that is terminal, or whose receiver is not in S, or whose
// receiver is a junction.  Order and magnitude are constant on a link, so they are worked out
// on the link graph (node = stop, a few per cent of the stream cells), not per cell and not
// per tile: the order at a tile's exit is no linear function of the orders entering the tile,
// which is what flow accumulation's exit forest would need.
//   1  (streamorder_node_kernel)   per 64 x 64 tile, a stencil: codes and stream membership
//      with a two-cell halo in LDS (the receiver of a frame cell lies in the first ring, its
//      donors in the second), nin of the tile and its first ring, then for every cell its
//      info byte (in S | nin) and whether it is a stop; zeroes the word of each stop.
//   2  hdem_flowtrace_u8_dev with the stop mask as its streams: stop[c], the first stop on
//      c's path, for every cell.  A loop without a stop (a stream loop without a junction, any
//      loop off the streams) is refused there, as a cycle, after its full schedule.
//   3  (streamorder_walk_kernel)   last donor continues, over links.  next(b) = stop[J] with J
//      b's receiver, when J is in S; the node's in-degree is nin(J), read off J.  A walk starts
//      at every head (stream cell with nin = 0), whose link has order 1 and magnitude 1, and
//      a hop is one compare-and-swap loop on the 64-bit word of next(b),
//      magnitude << 32 | arrivals << 16 | m << 8 | n  (m the greatest order arrived, n how
//      many arrivals had it): the new word says whether this arrival was the last, and if so
//      the node's order m + (n >= 2) and magnitude, with which the walk goes on.  Words are
//      touched by agent-scope atomics only.  A swap fails only because another donor's
//      succeeded, fewer than nin(J) <= 8 times; every hop completes one arrival, and a walk
//      takes at most as many hops as there are links.
//   4  (streamorder_gather_kernel) order and magnitude of c from the word of stop[c]; 0 off
//      the streams.  A junction whose node is short of arrivals is counted: a stream loop that
//      a tributary joins (its nodes wait for each other), refused as a cycle.
// Workspace: 10 B per cell (word 8, stop mask 1, info 1), 4 more for stop[] when the caller
// wants no link raster, behind the flow trace's own bytes in the context's arena.
#include "hdem_d8tile.h"

namespace {

constexpr int NT = 256;               // threads per workgroup, all kernels
constexpr int HC = TS + 4;            // staged codes and membership: the tile and two rings
constexpr int HN = TS + 2;            // nin: the tile and one ring
constexpr uint8_t IN_S = 0x10;        // info byte: in S; bits 0-3: nin

struct streamorder_counters {
    unsigned long long bad;           // cells holding an invalid byte
    unsigned long long stream_cells;
    unsigned long long heads;         // stream cells with nin = 0
    unsigned long long junctions;     // stream cells with nin >= 2
    unsigned long long links;         // stops
    unsigned long long capped;        // hops whose compare-and-swap loop reached its cap
    unsigned long long stuck;         // junctions whose node never saw all its arrivals
    int max_hops;                     // longest walk
    int max_order;
};

// the word of a node
__device__ __forceinline__ uint32_t w_arrivals(uint64_t w) { return (uint32_t)(w >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t w_order(uint64_t w)
{
    return ((uint32_t)(w >> 8) & 0xFFu) + (((uint32_t)w & 0xFFu) >= 2u);
}
__device__ __forceinline__ uint32_t w_magnitude(uint64_t w) { return (uint32_t)(w >> 32); }
// one more arrival, of order k and magnitude mag: (m, n) + k
__device__ __forceinline__ uint64_t w_arrive(uint64_t w, uint32_t k, uint32_t mag)
{
    uint32_t m = (uint32_t)(w >> 8) & 0xFFu, n = (uint32_t)w & 0xFFu;
    if (k > m) m = k, n = 1;
    else if (k == m) ++n;
    return ((uint64_t)(w_magnitude(w) + mag) << 32) | ((uint64_t)(w_arrivals(w) + 1u) << 16) |
           (m << 8) | n;
}

// 1.  STREAMS 0: every cell, 1: uint8 mask, 2: uint32 raster against a threshold.
template <int STREAMS>
__global__ __launch_bounds__(NT) void streamorder_node_kernel(
    const uint8_t *__restrict__ d8, const void *__restrict__ streams, uint32_t threshold, int H,
    int W, int tiles_x, uint8_t *__restrict__ stopmask, uint8_t *__restrict__ info,
    uint64_t *__restrict__ word, streamorder_counters *__restrict__ cnt)
{
    __shared__ uint8_t code[HC * HC];
    __shared__ uint8_t strm[HC * HC];
    __shared__ uint8_t nin[HN * HN];
    __shared__ unsigned int s_cnt[5];            // invalid, stream cells, heads, junctions, stops

    const int tid = threadIdx.x;
    const d8_tile tile = d8_tile_of_block(tiles_x, H, W);
    const int y0 = tile.y0, x0 = tile.x0;

    if (tid < 5) s_cnt[tid] = 0;
    for (int i = tid; i < HC * HC; i += NT) {
        const int gy = y0 + i / HC - 2, gx = x0 + i % HC - 2;
        uint8_t c = 0, s = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = (size_t)gy * W + gx;
            c = d8[g];
            s = 1;
            if (STREAMS == 1) s = static_cast<const uint8_t *>(streams)[g] != 0;
            if (STREAMS == 2) s = static_cast<const uint32_t *>(streams)[g] >= threshold;
        }
        code[i] = c;
        strm[i] = s;
    }
    __syncthreads();

    // stream donors of the tile's cells and of its first ring (an invalid byte is no code)
    for (int i = tid; i < HN * HN; i += NT) {
        const int at = (i / HN + 1) * HC + i % HN + 1;
        int n = 0;
        for (int b = 0; b < 8; ++b) {
            const int d = at - (code_dy(b) * HC + code_dx(b));   // the neighbour against b
            n += code[d] == (1 << b) && strm[d];
        }
        nin[i] = (uint8_t)n;
    }
    __syncthreads();

    unsigned int bad = 0, cells = 0, heads = 0, junctions = 0, stops = 0;
    for (int i = tid; i < TC; i += NT) {
        const int ly = i / TS, lx = i % TS;
        if (!tile.inside(ly, lx)) continue;
        const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
        const int at = (ly + 2) * HC + lx + 2;
        const d8_step s = d8_decode(code[at], ly, lx, tile, H, W);
        bad += s.invalid;
        uint8_t inf = 0, stop = 0;
        if (strm[at]) {
            const int n = nin[(ly + 1) * HN + lx + 1];
            inf = (uint8_t)(IN_S | n);
            ++cells;
            heads += n == 0;
            junctions += n >= 2;
            stop = s.terminal || !strm[(s.ny + 2) * HC + s.nx + 2] ||
                   nin[(s.ny + 1) * HN + s.nx + 1] >= 2;
            if (stop) {
                ++stops;
                word[g] = 0ull;
            }
        }
        info[g] = inf;
        stopmask[g] = stop;
    }
    if (bad) atomicAdd(&s_cnt[0], bad);
    if (cells) atomicAdd(&s_cnt[1], cells);
    if (heads) atomicAdd(&s_cnt[2], heads);
    if (junctions) atomicAdd(&s_cnt[3], junctions);
    if (stops) atomicAdd(&s_cnt[4], stops);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(&cnt->bad, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->stream_cells, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->heads, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->junctions, (unsigned long long)s_cnt[3]);
        if (s_cnt[4]) atomicAdd(&cnt->links, (unsigned long long)s_cnt[4]);
    }
}

// 3: one thread per cell; a head starts the walk of its link.
__global__ __launch_bounds__(NT) void streamorder_walk_kernel(
    int64_t cells, int H, int W, const uint8_t *__restrict__ d8, const uint8_t *__restrict__ info,
    const uint32_t *__restrict__ stop, uint64_t *word, streamorder_counters *__restrict__ cnt)
{
    __shared__ int s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
    int hops = 0;
    if (g < cells && info[g] == IN_S && stop[g]) {
        const unsigned long long links = cnt->links;
        uint32_t b = stop[g] - 1u, order = 1, magnitude = 1;
        for (unsigned long long step = 0; step < links; ++step) {
            const uint32_t c = d8[b];
            if (c == 0 || (c & (c - 1))) break;
            const int bit = __builtin_ctz(c);
            const int ny = (int)(b / (uint32_t)W) + code_dy(bit);
            const int nx = (int)(b % (uint32_t)W) + code_dx(bit);
            if (ny < 0 || ny >= H || nx < 0 || nx >= W) break;
            const size_t j = (size_t)ny * W + nx;
            const uint32_t inf = info[j], t1 = stop[j];
            if (!(inf & IN_S) || !t1) break;             // the link ends off the streams
            const uint32_t need = inf & 0xFu, t = t1 - 1u;
            // a swap fails only because another donor's succeeded: fewer than `need` times
            uint64_t cur = __hip_atomic_load(&word[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint64_t arrived;
            uint32_t tries = 0;
            bool capped = false;
            for (;;) {
                arrived = w_arrive(cur, order, magnitude);
                if (__hip_atomic_compare_exchange_strong(&word[t], &cur, arrived, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT))
                    break;
                if (++tries > need) { capped = true; break; }
            }
            if (capped) {
                atomicAdd(&cnt->capped, 1ull);
                break;
            }
            ++hops;
            if (w_arrivals(arrived) != need) break;      // another donor's walk goes on
            order = w_order(arrived);
            magnitude = w_magnitude(arrived);
            b = t;
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

// 4: one thread per cell, a block row per raster row.  stop may be out_link (read, then
// rewritten by the same thread).
__global__ __launch_bounds__(NT) void streamorder_gather_kernel(
    int H, int W, const uint8_t *__restrict__ info, const uint32_t *stop,
    const uint64_t *__restrict__ word, uint8_t *__restrict__ out_order,
    uint32_t *__restrict__ out_magnitude, uint32_t *out_link,
    streamorder_counters *__restrict__ cnt)
{
    __shared__ unsigned int s_stuck;
    __shared__ int s_order;
    if (threadIdx.x == 0) s_stuck = 0, s_order = 0;
    __syncthreads();
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    int order = 0;
    unsigned int stuck = 0;
    if (x < W) {
        const size_t g = (size_t)y * W + x;
        const uint32_t inf = info[g];
        uint32_t magnitude = 0, l = 0;
        if (inf & IN_S) {
            l = stop[g];
            order = 1, magnitude = 1;
            const uint64_t w = l ? word[l - 1u] : 0ull;
            if (w_arrivals(w)) order = (int)w_order(w), magnitude = w_magnitude(w);
            // c is a junction: the first cell of its link, whose node its donors arrive at
            if ((inf & 0xFu) >= 2u && w_arrivals(w) != (inf & 0xFu)) stuck = 1;
        }
        if (out_order) out_order[g] = (uint8_t)order;
        if (out_magnitude) out_magnitude[g] = magnitude;
        if (out_link) out_link[g] = l;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        order = max(order, __shfl_xor(order, m));
        stuck += __shfl_xor(stuck, m);
    }
    if ((threadIdx.x & 63) == 0) {
        if (order) atomicMax(&s_order, order);
        if (stuck) atomicAdd(&s_stuck, stuck);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_order > __hip_atomic_load(&cnt->max_order, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&cnt->max_order, s_order);
        if (s_stuck) atomicAdd(&cnt->stuck, (unsigned long long)s_stuck);
    }
}

// also the tile grid: nothing is allocated for a raster that is refused
int check_args(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
               int stream_kind, uint32_t threshold, const uint8_t *order,
               const uint32_t *magnitude, const uint32_t *link, int flags,
               const hdem_streamorder_stats *stats, d8_grid *g)
{
    if (int rc = hdem_check_call(ctx, d8, d8, H, W)) return rc;
    if (int rc = d8_grid_of("stream order", H, W, g)) return rc;
    HDEM_REQUIRE(!flags, HDEM_ERR_BAD_ARG, "unknown stream order flags 0x%x", flags);
    HDEM_REQUIRE(order || magnitude || link, HDEM_ERR_BAD_ARG,
                 "no output wanted: give at least one of order, magnitude, link");
    if (int rc = d8_check_streams(streams, stream_kind, threshold)) return rc;
    return d8_check_stats(stats, "hdem_streamorder_stats");
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_streamorder_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                       const void *streams, int stream_kind, uint32_t threshold,
                                       uint8_t *order, uint32_t *magnitude, uint32_t *link,
                                       int flags, hdem_streamorder_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, streams, stream_kind, threshold, order, magnitude, link,
                            flags, stats, &g))
        return rc;
    const int64_t cells = (int64_t)H * W;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_streamorder_stats st = {};
    d8_publish(stats, st);

    // arena: the flow trace's bytes | counters | word u64 per cell | stop u32 per cell (when
    // the caller's link raster does not hold it) | stop mask u8 | info u8
    const size_t trace = hdem_round16(hdem_flowtrace_arena_bytes(g.tiles, g.nslots));
    const size_t head = 256;
    static_assert(sizeof(streamorder_counters) <= head, "counters outgrew their block");
    const size_t stop_bytes = link ? 0 : hdem_round16((size_t)cells * 4);
    const size_t bytes = trace + head + (size_t)cells * 8 + stop_bytes +
                         2 * hdem_round16((size_t)cells);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    streamorder_counters *cnt = reinterpret_cast<streamorder_counters *>(ws + trace);
    uint64_t *word = reinterpret_cast<uint64_t *>(ws + trace + head);
    char *after = reinterpret_cast<char *>(word + cells);
    uint32_t *stop = link ? link : reinterpret_cast<uint32_t *>(after);
    uint8_t *stopmask = reinterpret_cast<uint8_t *>(after + stop_bytes);
    uint8_t *info = stopmask + hdem_round16((size_t)cells);

    hdem_event_timer<4> phases(ctx, stats != nullptr);
    if (int rc = phases.start()) return rc;

    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(streamorder_counters), ctx->stream));
    const dim3 grid((unsigned)g.tiles);
    phases.mark(0);
    if (stream_kind == HDEM_FT_STREAMS_NONE)
        hipLaunchKernelGGL(streamorder_node_kernel<0>, grid, dim3(NT), 0, ctx->stream, d8, streams,
                           threshold, H, W, g.tiles_x, stopmask, info, word, cnt);
    else if (stream_kind == HDEM_FT_STREAMS_MASK_U8)
        hipLaunchKernelGGL(streamorder_node_kernel<1>, grid, dim3(NT), 0, ctx->stream, d8, streams,
                           threshold, H, W, g.tiles_x, stopmask, info, word, cnt);
    else
        hipLaunchKernelGGL(streamorder_node_kernel<2>, grid, dim3(NT), 0, ctx->stream, d8, streams,
                           threshold, H, W, g.tiles_x, stopmask, info, word, cnt);
    HDEM_HIP_CHECK(hipGetLastError());
    // the first stop of every cell; the trace takes the head of the arena, refuses invalid
    // bytes and loops that hold no stop, and synchronises
    if (int rc = hdem_flowtrace_u8_dev(ctx, d8, H, W, stopmask, HDEM_FT_STREAMS_MASK_U8, 0, nullptr,
                                       1.0, stop, nullptr, nullptr, nullptr, nullptr, 0, nullptr))
        return rc;
    phases.mark(1);
    hipLaunchKernelGGL(streamorder_walk_kernel, dim3((unsigned)((cells + NT - 1) / NT)), dim3(NT),
                       0, ctx->stream, cells, H, W, d8, info, stop, word, cnt);
    phases.mark(2);
    hipLaunchKernelGGL(streamorder_gather_kernel, hdem_grid2(W, H, NT), dim3(NT), 0, ctx->stream,
                       H, W, info, stop, word, order, magnitude, link, cnt);
    phases.mark(3);
    HDEM_HIP_CHECK(hipGetLastError());
    streamorder_counters host = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.max_order = host.max_order;
    st.stream_cells = (int64_t)host.stream_cells;
    st.heads = (int64_t)host.heads;
    st.junctions = (int64_t)host.junctions;
    st.links = (int64_t)host.links;
    st.max_hops = host.max_hops;
    st.tile_h = TS;
    st.tile_w = TS;
    phases.read(&st.ms_nodes, &st.ms_walk, &st.ms_gather);
    d8_publish(stats, st);
    if (int rc = d8_report_invalid(host.bad)) return rc;
    HDEM_REQUIRE(!host.capped, HDEM_ERR_NOT_CONVERGED,
                 "stream order: %llu hops gave up their compare-and-swap", host.capped);
    HDEM_REQUIRE(!host.stuck, HDEM_ERR_BAD_ARG,
                 "flow directions form a cycle: %llu stream junctions never receive all their "
                 "tributaries",
                 host.stuck);
    return HDEM_OK;
}

extern "C" int hdem_streamorder_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                                   const void *streams, int stream_kind, uint32_t threshold,
                                   uint8_t *order, uint32_t *magnitude, uint32_t *link, int flags,
                                   hdem_streamorder_stats *stats)
{
    d8_grid g;
    if (int rc = check_args(ctx, d8, H, W, streams, stream_kind, threshold, order, magnitude, link,
                            flags, stats, &g))
        return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)H * W;
    hdem_dbuf dd8, dstreams, dout[3];
    const size_t sb = n * (stream_kind == HDEM_FT_STREAMS_ACC_U32 ? sizeof(uint32_t) : 1);
    if (int rc = dd8.upload(ctx, d8, n)) return rc;
    if (int rc = dstreams.upload(ctx, streams, sb)) return rc;
    void *const host_out[3] = {order, magnitude, link};
    const size_t out_bytes[3] = {n, n * 4, n * 4};
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc = dout[k].alloc(ctx, out_bytes[k])) return rc;
    const int rc = hdem_streamorder_u8_dev(ctx, dd8.as<const uint8_t>(), H, W, dstreams.p,
                                           stream_kind, threshold, dout[0].as<uint8_t>(),
                                           dout[1].as<uint32_t>(), dout[2].as<uint32_t>(), flags,
                                           stats);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k)
        if (host_out[k])
            if (int rc2 = dout[k].download(host_out[k], out_bytes[k])) return rc2;
    return HDEM_OK;
}
