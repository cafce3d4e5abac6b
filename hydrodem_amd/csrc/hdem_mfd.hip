// A24 / A25  Multiple-flow-direction (MFD) flow direction and accumulation (Quinn 1991, Freeman
// 1991, Holmgren 1994; new operators; include/hydrodem_hip.h has the contract, DESIGN 3.26 the
// argument).
//
// The word of a cell, one uint64: bit 59 "has outflow", the main receiver's direction m in bits
// 56-58, and seven 8-bit shares p_1 ... p_7 in bits 0-55, p_j for the neighbour in direction
// (m + j) & 7 in units of 2^-8; the main receiver takes what the others leave.  Directions are
// those of hdem_dinf.hip: 0 = E, 1 = NE, 2 = N ... 7 = SE, north is row - 1.
//
// Direction (mfd_kernel): one launch on the staging of hdem_stencil_tile.h, a thread per column
// of the 256 x 32 tile, float64 on the float32 elevations.  mfd_pw is the contract's own power
// function: a fixed sequence of float64 operations, so that the words do not depend on a math
// library.
//
// Accumulation is the pull over donors on a DAG of hdem_dinf.hip (classify, rounds of tile
// visits in LDS, schedule, final; its header comment has the argument for schedule freedom,
// which nowhere depends on the number of receivers) with the routing of the MFD word: up to
// eight donors per cell, a uint64 word beside the uint64 value in LDS (16 B per cell), and the
// donor mask of a cell in bits 48-55 of its own not-yet-final value word, which until then
// holds only q(w) < 2^31 or nothing.  The kernels are this file's own copies: hdem_dinf.hip is
// left as it is (DESIGN 3.26 says why).
#include "hdem_d8tile.h"
#include "hdem_stencil_tile.h"

#include <cmath>

namespace {

constexpr uint64_t FINAL = 1ull << 63;
constexpr uint64_t HAS_FLOW = 1ull << 59;
constexpr uint64_t SHARES = (1ull << 56) - 1;     // the seven share fields
constexpr uint64_t AMOUNT = (1ull << 48) - 1;     // the low bits of a value word: A or q(w)
constexpr int LH = TS + 2;                        // LDS rows: the tile and its halo
constexpr int LW = TS + 3;                        // LDS row pitch: odd (hdem_dinf.hip)

// direction d -> (dy, dx), packed (d + 1) in 4 bits per entry
__host__ __device__ __forceinline__ int dir_dy(int d) { return ((0x22210001u >> (4 * d)) & 3) - 1; }
__host__ __device__ __forceinline__ int dir_dx(int d) { return ((0x21000122u >> (4 * d)) & 3) - 1; }

__device__ __forceinline__ int word_main(uint64_t w) { return (int)((w >> 56) & 7); }
// the share field of the (valid, non-zero) word w for direction `toward`; 0 for the main one
__device__ __forceinline__ uint64_t word_field(uint64_t w, int toward)
{
    const int j = (toward - word_main(w)) & 7;
    return j ? (w >> (8 * (j - 1))) & 0xFFu : 0u;
}
__device__ __forceinline__ uint32_t word_field_sum(uint64_t w)
{
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) sum += (uint32_t)((w >> (8 * j)) & 0xFFu);
    return sum;
}
__device__ __forceinline__ bool word_valid(uint64_t w)
{
    return w == 0 || ((w >> 59) == 1 && word_field_sum(w) <= 255);
}
// does the (valid) word w name the neighbour in direction `toward` as a receiver?
__device__ __forceinline__ bool word_gives(uint64_t w, int toward)
{
    return w != 0 && (word_main(w) == toward || word_field(w, toward) != 0);
}
// what a donor with word w and amount a sends in direction `toward` (word_gives holds):
// (a * p) >> 8 to a receiver with a share field, the rest to the main one
__device__ __forceinline__ uint64_t word_share(uint64_t w, uint64_t a, int toward)
{
    if (word_main(w) != toward) return (a * word_field(w, toward)) >> 8;
    uint64_t rest = a;
#pragma unroll
    for (int j = 0; j < 7; ++j) rest -= (a * ((w >> (8 * j)) & 0xFFu)) >> 8;
    return rest;
}
// the canonical word of the ESRI D8 code c (one bit set): bit b is direction (8 - b) & 7
__device__ __forceinline__ uint64_t word_of_code(uint32_t c)
{
    return HAS_FLOW | ((uint64_t)((8 - __builtin_ctz(c)) & 7) << 56);
}

// ---------------------------------------------------------------------------
// A24  direction
// ---------------------------------------------------------------------------
// pw(t, e) = t^e for t in [2^-64, 1], e in [0.25, 16], as the header writes it out: the same
// float64 operations in the same order as tests/test_mfd.py's transcription.  Constants of the
// form 1.0 / n are the correctly rounded quotients.
__device__ __forceinline__ double mfd_pw(double t, double e)
{
    int k;
    double m = frexp(t, &k);                       // t = m * 2^k, m in [0.5, 1)
    if (m < 0.7071067811865476) {
        m = m * 2.0;
        k = k - 1;
    }
    const double s = (m - 1.0) / (m + 1.0);        // ln m = 2 atanh s, |s| < 0.1716
    const double s2 = s * s;
    double r = 1.0 / 15.0;
    r = r * s2 + 1.0 / 13.0;
    r = r * s2 + 1.0 / 11.0;
    r = r * s2 + 1.0 / 9.0;
    r = r * s2 + 1.0 / 7.0;
    r = r * s2 + 1.0 / 5.0;
    r = r * s2 + 1.0 / 3.0;
    r = r * s2 + 1.0;
    const double l2 = (double)k + ((2.0 * s) * r) * 1.4426950408889634;   // log2 t
    const double y = e * l2;
    const double n = floor(y + 0.5);
    const double u = (y - n) * 0.6931471805599453;                      // |u| <= 0.3466
    double p = 1.0;
    p = 1.0 + (u * p) * (1.0 / 12.0);
    p = 1.0 + (u * p) * (1.0 / 11.0);
    p = 1.0 + (u * p) * (1.0 / 10.0);
    p = 1.0 + (u * p) * (1.0 / 9.0);
    p = 1.0 + (u * p) * (1.0 / 8.0);
    p = 1.0 + (u * p) * (1.0 / 7.0);
    p = 1.0 + (u * p) * (1.0 / 6.0);
    p = 1.0 + (u * p) * (1.0 / 5.0);
    p = 1.0 + (u * p) * (1.0 / 4.0);
    p = 1.0 + (u * p) * (1.0 / 3.0);
    p = 1.0 + (u * p) * (1.0 / 2.0);
    p = 1.0 + u * p;
    return ldexp(p, (int)n);
}

enum { M_NOFLOW, M_FALLBACK, M_INVALID, M_SPLIT, M_COUNT };
constexpr double T_MIN = 5.421010862427522e-20;    // 2^-64

struct mfd_args {
    const float *z;
    const uint8_t *fallback;
    uint64_t *words;
    float *slope;
    int H, W, tiles_x;
    double dx, dy, diag;            // diag = sqrt(dx^2 + dy^2)
    double exponent, w_card, w_diag;
    unsigned long long *cnt;        // M_COUNT counters, zeroed by the caller
};

__global__ __launch_bounds__(NT) void mfd_kernel(const mfd_args p)
{
    __shared__ __attribute__((aligned(16))) float t[(TH + 2) * LS];
    __shared__ unsigned int s_cnt[M_COUNT];
    const int H = p.H, W = p.W;
    const int bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int x0 = bx * TW, y0 = by * TH;
    if (threadIdx.x < M_COUNT) s_cnt[threadIdx.x] = 0;
    // outside the raster reads NaN: the raster's edge and nodata are one rule
    stage_tile<float, false, true>(p.z, H, W, y0, x0, t);
    __syncthreads();

    const int x = x0 + (int)threadIdx.x;
    const bool linear = p.exponent == 1.0;
    unsigned int n[M_COUNT] = {0, 0, 0, 0};
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
            double s[8], smax = 0.0;
            const bool finite = fabsf(centre) < HDEM_INF;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const double dist = (d & 1) ? p.diag : (d & 2) ? p.dy : p.dx;
                const double drop = e0 - nb[d];
                s[d] = (finite && nb[d] == nb[d] && drop > 0.0) ? drop / dist : 0.0;
                smax = s[d] > smax ? s[d] : smax;
            }
            uint64_t word = 0;
            if (smax > 0.0) {
                double f[8], fbest = 0.0;
                int m = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    double fd = 0.0;
                    if (s[d] > 0.0) {
                        const double td = s[d] == smax ? 1.0 : s[d] / smax;
                        if (td >= T_MIN)
                            fd = ((d & 1) ? p.w_diag : p.w_card) *
                                 (linear ? td : mfd_pw(td, p.exponent));
                    }
                    f[d] = fd;
                    if (fd > fbest) fbest = fd, m = d;
                }
                double total = 0.0;
#pragma unroll
                for (int d = 0; d < 8; ++d) total = total + f[d];
                word = HAS_FLOW | ((uint64_t)m << 56);
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    if (d == m || !(f[d] > 0.0)) continue;
                    const uint64_t share = (uint64_t)floor((256.0 * f[d]) / total + 0.5);
                    word |= share << (8 * (((d - m) & 7) - 1));
                }
                n[M_SPLIT] += (word & SHARES) != 0;
            } else if (p.fallback) {
                const uint32_t code = p.fallback[(size_t)y * W + x];
                if (code & (code - 1)) {
                    ++n[M_INVALID];
                } else if (code) {
                    word = word_of_code(code);
                    ++n[M_FALLBACK];
                }
            }
            n[M_NOFLOW] += word == 0;
            const size_t at = (size_t)y * W + x;
            p.words[at] = word;
            if (p.slope) p.slope[at] = centre == centre ? (float)smax : __builtin_nanf("");
        }
    }
    // lane -> wave -> workgroup -> one global atomic per counter
#pragma unroll
    for (int j = 0; j < M_COUNT; ++j) {
        unsigned int v = n[j];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[j], v);
    }
    __syncthreads();
    if (threadIdx.x < M_COUNT && s_cnt[threadIdx.x])
        atomicAdd(&p.cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

struct mfd_call {
    const float *dem;
    int H, W;
    const uint8_t *fallback;
    double dx, dy, exponent, w_card, w_diag;
    uint64_t *words;
    float *slope;
};

int mfd_check(const hdem_ctx *ctx, const mfd_call &a, int flags, const hdem_mfd_stats *stats,
              int *tiles_x, int64_t *tiles)
{
    if (int rc = hdem_check_call(ctx, a.dem, a.words, a.H, a.W)) return rc;
    if (int rc = d8_check_stats(stats, "hdem_mfd_stats")) return rc;
    HDEM_REQUIRE(!(flags & ~HDEM_ON_DEVICE), HDEM_ERR_BAD_ARG,
                 "MFD flow direction: unknown flags 0x%x", flags);
    HDEM_REQUIRE(positive(a.dx) && positive(a.dy), HDEM_ERR_BAD_ARG,
                 "dx and dy must be finite and positive, got %g and %g", a.dx, a.dy);
    HDEM_REQUIRE(a.exponent >= 0.25 && a.exponent <= 16.0, HDEM_ERR_BAD_ARG,
                 "the exponent is 0.25 ... 16, got %g", a.exponent);
    HDEM_REQUIRE(positive(a.w_card) && positive(a.w_diag), HDEM_ERR_BAD_ARG,
                 "w_card and w_diag must be finite and positive, got %g and %g", a.w_card,
                 a.w_diag);
    *tiles_x = (a.W + TW - 1) / TW;
    *tiles = (int64_t)*tiles_x * ((a.H + TH - 1) / TH);
    HDEM_REQUIRE(*tiles <= INT32_MAX, HDEM_ERR_BAD_ARG,
                 "MFD flow direction: %d x %d has %lld tiles of %d x %d, more than %d", a.H, a.W,
                 (long long)*tiles, TH, TW, INT32_MAX);
    return HDEM_OK;
}

// The direction on device pointers, after mfd_check.
int mfd_dev(hdem_ctx *ctx, const mfd_call &a, int tiles_x, int64_t tiles, hdem_mfd_stats *stats)
{
    hdem_mfd_stats st = {};
    d8_publish(stats, st);
    unsigned long long *cnt =
        static_cast<unsigned long long *>(hdem_arena(ctx, M_COUNT * sizeof(unsigned long long)));
    if (!cnt) return HDEM_ERR_OOM;

    mfd_args p = {};
    p.z = a.dem, p.fallback = a.fallback, p.words = a.words, p.slope = a.slope;
    p.H = a.H, p.W = a.W, p.tiles_x = tiles_x;
    p.dx = a.dx, p.dy = a.dy, p.diag = std::sqrt(a.dx * a.dx + a.dy * a.dy);
    p.exponent = a.exponent, p.w_card = a.w_card, p.w_diag = a.w_diag;
    p.cnt = cnt;

    hdem_event_timer<2> timer(ctx, stats != nullptr);   // around the launch
    if (int rc = timer.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, M_COUNT * sizeof(unsigned long long), ctx->stream));
    timer.mark(0);
    hipLaunchKernelGGL(mfd_kernel, dim3((unsigned)tiles), dim3(NT), 0, ctx->stream, p);
    timer.mark(1);
    HDEM_HIP_CHECK(hipGetLastError());
    unsigned long long host[M_COUNT] = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st.no_flow = (int64_t)host[M_NOFLOW];
    st.fallback_cells = (int64_t)host[M_FALLBACK];
    st.split_cells = (int64_t)host[M_SPLIT];
    st.ms_total = timer.ms(0, 1);
    d8_publish(stats, st);
    return d8_report_invalid(host[M_INVALID]);
}

// ---------------------------------------------------------------------------
// A25  accumulation
// ---------------------------------------------------------------------------
struct mfdacc_counters {
    unsigned long long split;         // cells with more than one receiver
    unsigned long long terminal;      // cells with word 0
    unsigned long long bad;           // invalid words
    unsigned long long outside;       // cells with a receiver outside the raster
    unsigned long long unresolved;    // cells that never became final
    unsigned int listed;              // length of the list for the next round
    unsigned int pad;
    // the weighted form alone, behind what the unweighted one reads
    unsigned long long nan;           // NaN weights (they contribute 0)
    unsigned long long negative;      // weights below 0 (-inf among them)
    unsigned long long infinite;      // +inf
    unsigned long long over;          // q(w) > 2^31 - 1
    unsigned long long total;         // the sum of q(w) over the raster
};
constexpr size_t COUNTERS_UNWEIGHTED = offsetof(mfdacc_counters, nan);
constexpr double Q_MAX = 2147483647.0;
constexpr unsigned long long TOTAL_LIMIT = 1ull << 48;

// q(w) of cell g, A22's rule; a weight that is refused counts 0.  n[]: what the weight is
// counted as (nan, negative, infinite, over).
template <int WT>
__device__ __forceinline__ uint64_t mfd_weight_of(const void *__restrict__ weights, size_t g,
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
__global__ __launch_bounds__(NT) void mfdacc_classify_kernel(
    const uint64_t *__restrict__ words, int H, int W, int tiles_x, uint64_t *__restrict__ work,
    uint32_t *__restrict__ left, uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    mfdacc_counters *__restrict__ cnt, const void *__restrict__ weights, double scale,
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
        const uint64_t w = words[g];
        if (!word_valid(w)) {
            ++n[2];
        } else if (!w) {
            ++n[1];
        } else {
            n[0] += (w & SHARES) != 0;
            bool out = false;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int ny = gy + dir_dy(d), nx = gx + dir_dx(d);
                out |= word_gives(w, d) && (ny < 0 || ny >= H || nx < 0 || nx >= W);
            }
            n[3] += out;
        }
        if (WT) {                                // not final, the own term in the low bits
            const uint64_t q = mfd_weight_of<WT>(weights, g, scale, frac_bits, nw);
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
__global__ __launch_bounds__(NT) void mfdacc_schedule_kernel(
    int tiles_y, int tiles_x, uint32_t round, const uint32_t *__restrict__ left,
    const uint32_t *__restrict__ stamp, uint32_t *__restrict__ list,
    mfdacc_counters *__restrict__ cnt)
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
__global__ __launch_bounds__(NT) void mfdacc_visit_kernel(
    const uint64_t *__restrict__ words, uint64_t *work, int H, int W, int tiles_x,
    const uint32_t *__restrict__ list, uint32_t round, uint64_t unit, uint32_t *__restrict__ stamp,
    uint32_t *__restrict__ left)
{
    // bit 63: final, and then the low 48 bits A.  Not final: q(w) in the low bits (weighted),
    // the cell's donors in bits 48-55 (the cells of the tile, once the first pass has run)
    __shared__ uint64_t v[LH * LW];
    __shared__ uint64_t w[LH * LW];              // the word
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
        w[hy * LW + hx] = in ? words[g] : 0ull;
        lds_store(&v[hy * LW + hx], in ? work_load(work + g) : FINAL);
    }
    __syncthreads();

    // the donors of the thread's 16 cells that are not final yet (`pending`: which of them);
    // a cell without donors is final at once.  Only a cell's own thread writes its value word
    // here, and the donor test reads the words alone: the pass needs no barrier of its own.
    uint32_t pending = 0;
    int changed = 0;
#pragma unroll
    for (int k = 0; k < TC / NT; ++k) {
        const int i = tid + k * NT;
        const int c = (i / TS + 1) * LW + i % TS + 1;
        const uint64_t own = lds_load(&v[c]);
        if (own & FINAL) continue;
        pending |= 1u << k;
        uint64_t donors = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (word_gives(w[c + dir_dy(d) * LW + dir_dx(d)], (d + 4) & 7)) donors |= 1ull << d;
        if (!donors) {
            lds_store(&v[c], FINAL | (WEIGHTED ? own & AMOUNT : unit));
            changed = 1;
        } else {
            lds_store(&v[c], (own & AMOUNT) | (donors << 48));
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
            uint32_t donors = (uint32_t)(own >> 48) & 0xFFu;
            uint64_t sum = WEIGHTED ? own & AMOUNT : unit;
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
                sum += word_share(w[n], vn & AMOUNT, (d + 4) & 7);
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

__global__ __launch_bounds__(NT) void mfdacc_final_kernel(
    const uint64_t *work, int H, int W, int tiles_x, double scale, int64_t *sum,
    float *__restrict__ value, mfdacc_counters *__restrict__ cnt)
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
        const uint64_t a = vc & AMOUNT;
        if (sum) sum[g] = (int64_t)a;                    // may be the working raster itself
        if (value) value[g] = (float)((double)a * scale);
    }
    if (unresolved) atomicAdd(&s_unresolved, unresolved);
    __syncthreads();
    if (tid == 0 && s_unresolved)
        atomicAdd(&cnt->unresolved, (unsigned long long)s_unresolved);
}

struct mfdacc_call {
    const uint64_t *words;
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
int mfdacc_check(const hdem_ctx *ctx, const mfdacc_call &a, int flags,
                 const hdem_mfdacc_stats *stats, d8_grid *g)
{
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.words, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(a.H > 0 && a.W > 0, HDEM_ERR_BAD_ARG,
                 "raster dimensions must be positive, got %d x %d", a.H, a.W);
    if (int rc = d8_check_stats(stats, "hdem_mfdacc_stats")) return rc;
    HDEM_REQUIRE(a.sum || a.value, HDEM_ERR_BAD_ARG, "MFD flow accumulation: no output wanted");
    if (!a.weights) {
        HDEM_REQUIRE(!a.weight_type, HDEM_ERR_BAD_ARG,
                     "weight type %d without a weight raster", a.weight_type);
        HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 16, HDEM_ERR_BAD_ARG,
                     "frac_bits is 0 ... 16, got %d", a.frac_bits);
    } else {
        HDEM_REQUIRE(a.weight_type >= HDEM_FLOWSUM_F32 && a.weight_type <= HDEM_FLOWSUM_U8,
                     HDEM_ERR_BAD_ARG, "unknown weight type %d", a.weight_type);
        if (a.weight_type == HDEM_FLOWSUM_F32)
            HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 30, HDEM_ERR_BAD_ARG,
                         "frac_bits is 0 ... 30, got %d", a.frac_bits);
        else
            HDEM_REQUIRE(a.frac_bits >= 0 && a.frac_bits <= 16, HDEM_ERR_BAD_ARG,
                         "integer weights take frac_bits 0 ... 16, got %d", a.frac_bits);
    }
    HDEM_REQUIRE(!(flags & ~HDEM_ON_DEVICE), HDEM_ERR_BAD_ARG,
                 "MFD flow accumulation: unknown flags 0x%x", flags);
    if (int rc = d8_grid_of("MFD flow accumulation", a.H, a.W, g)) return rc;
    const size_t n = (size_t)a.H * a.W;
    span s[4];
    int ns = 0;
    s[ns++] = {"words", (uintptr_t)a.words, (uintptr_t)a.words + 8 * n};
    if (a.weights)
        s[ns++] = {"weights", (uintptr_t)a.weights,
                   (uintptr_t)a.weights + n * weight_bytes(a.weight_type)};
    const span outs[2] = {{"sum", (uintptr_t)a.sum, (uintptr_t)a.sum + 8 * n},
                          {"value", (uintptr_t)a.value, (uintptr_t)a.value + 4 * n}};
    for (const span &o : outs) {
        if (!o.lo) continue;
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "MFD flow accumulation: %s overlaps %s", o.name, s[j].name);
        s[ns++] = o;
    }
    return HDEM_OK;
}

void launch_classify(hdem_ctx *ctx, const mfdacc_call &a, const d8_grid &g, uint64_t *work,
                     uint32_t *left, uint32_t *stamp, uint32_t *list, mfdacc_counters *cnt)
{
    const dim3 grid((unsigned)g.tiles), block(NT);
    const double scale = (double)(1ll << a.frac_bits);
#define HDEM_MFD_CLASSIFY(WT)                                                                     \
    hipLaunchKernelGGL((mfdacc_classify_kernel<WT>), grid, block, 0, ctx->stream, a.words, a.H,   \
                       a.W, g.tiles_x, work, left, stamp, list, cnt, a.weights, scale, a.frac_bits)
    if (!a.weights) HDEM_MFD_CLASSIFY(0);
    else if (a.weight_type == HDEM_FLOWSUM_F32) HDEM_MFD_CLASSIFY(HDEM_FLOWSUM_F32);
    else if (a.weight_type == HDEM_FLOWSUM_U32) HDEM_MFD_CLASSIFY(HDEM_FLOWSUM_U32);
    else HDEM_MFD_CLASSIFY(HDEM_FLOWSUM_U8);
#undef HDEM_MFD_CLASSIFY
}

// The accumulation on device pointers, after mfdacc_check.  *st is filled when the launches ran,
// whatever is returned; the caller publishes it.
int mfdacc_dev(hdem_ctx *ctx, const mfdacc_call &a, const d8_grid &g, bool want_stats,
               hdem_mfdacc_stats *st)
{
    const bool weighted = a.weights != nullptr;
    const int H = a.H, W = a.W, tiles_x = g.tiles_x;
    const int64_t tiles = g.tiles, cells = (int64_t)H * W;

    // arena: counters | left, stamp, list: u32 per tile each | the working raster, u64 per
    // cell, unless the caller's sum serves
    const size_t head = 512;
    static_assert(sizeof(mfdacc_counters) <= head, "counters outgrew their block");
    const size_t per_tile = hdem_round16((size_t)tiles * 12);
    const size_t bytes = head + per_tile + (a.sum ? 0 : (size_t)cells * 8);
    char *ws = static_cast<char *>(hdem_arena(ctx, bytes));
    if (!ws) return HDEM_ERR_OOM;
    mfdacc_counters *cnt = reinterpret_cast<mfdacc_counters *>(ws);
    uint32_t *left = reinterpret_cast<uint32_t *>(ws + head);
    uint32_t *stamp = left + tiles, *list = stamp + tiles;
    uint64_t *work = a.sum ? reinterpret_cast<uint64_t *>(a.sum)
                           : reinterpret_cast<uint64_t *>(ws + head + per_tile);
    const uint64_t unit = 1ull << (weighted ? 0 : a.frac_bits);
    // the unweighted form neither zeroes nor reads the counters of the weights
    const size_t cnt_bytes = weighted ? sizeof(mfdacc_counters) : COUNTERS_UNWEIGHTED;

    hdem_event_timer<4> phases(ctx, want_stats);
    if (int rc = phases.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, cnt_bytes, ctx->stream));
    const dim3 grid((unsigned)tiles);

    phases.mark(0);
    launch_classify(ctx, a, g, work, left, stamp, list, cnt);
    phases.mark(1);
    // one host read per round: the length of the round's list, which is its grid
    mfdacc_counters host = {};
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
            hipLaunchKernelGGL(mfdacc_visit_kernel<true>, dim3(host.listed), dim3(NT), 0,
                               ctx->stream, a.words, work, H, W, tiles_x, list, (uint32_t)rounds,
                               unit, stamp, left);
        else
            hipLaunchKernelGGL(mfdacc_visit_kernel<false>, dim3(host.listed), dim3(NT), 0,
                               ctx->stream, a.words, work, H, W, tiles_x, list, (uint32_t)rounds,
                               unit, stamp, left);
        HDEM_HIP_CHECK(hipMemsetAsync(&cnt->listed, 0, sizeof(cnt->listed), ctx->stream));
        hipLaunchKernelGGL(mfdacc_schedule_kernel, dim3((unsigned)((tiles + NT - 1) / NT)),
                           dim3(NT), 0, ctx->stream, g.tiles_y, tiles_x, (uint32_t)rounds + 1,
                           left, stamp, list, cnt);
    }
    phases.mark(2);
    if (!refused) {
        hipLaunchKernelGGL(mfdacc_final_kernel, grid, dim3(NT), 0, ctx->stream, work, H, W,
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
                 "invalid MFD word in %llu cells: a word is 0, or bit 59 is set, bits 60-63 are 0 "
                 "and the seven shares in bits 0-55 sum to at most 255",
                 host.bad);
    HDEM_REQUIRE(!host.outside, HDEM_ERR_BAD_ARG,
                 "MFD words send flow outside the raster in %llu cells", host.outside);
    HDEM_REQUIRE(!host.negative && !host.infinite && !host.over, HDEM_ERR_BAD_ARG,
                 "weights out of range in %llu cells: %llu negative, %llu infinite, %llu above "
                 "2^31 - 1 once quantised (frac_bits %d)",
                 host.negative + host.infinite + host.over, host.negative, host.infinite,
                 host.over, a.frac_bits);
    HDEM_REQUIRE(host.total < TOTAL_LIMIT, HDEM_ERR_BAD_ARG,
                 "the quantised weights sum to %llu: the total must stay below 2^48 (frac_bits %d)",
                 host.total, a.frac_bits);
    HDEM_REQUIRE(!host.unresolved, HDEM_ERR_BAD_ARG,
                 "MFD words form a cycle: %llu cells never resolve", host.unresolved);
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: one symbol per operator; HDEM_ON_DEVICE in flags says the pointers are device pointers
// ---------------------------------------------------------------------------
extern "C" int hdem_mfd_f32(hdem_ctx *ctx, const float *dem, int H, int W, const uint8_t *fallback,
                            double dx, double dy, double exponent, double w_card, double w_diag,
                            uint64_t *words, float *slope, int flags, hdem_mfd_stats *stats)
{
    mfd_call a = {dem, H, W, fallback, dx, dy, exponent, w_card, w_diag, words, slope};
    int tiles_x;
    int64_t tiles;
    if (int rc = mfd_check(ctx, a, flags, stats, &tiles_x, &tiles)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    if (flags & HDEM_ON_DEVICE) return mfd_dev(ctx, a, tiles_x, tiles, stats);

    const size_t n = (size_t)H * W;
    hdem_dbuf ddem, dfb, dwords, dslope;
    if (int rc = ddem.upload(ctx, dem, n * 4)) return rc;
    if (int rc = dfb.upload(ctx, fallback, n)) return rc;
    if (int rc = dwords.alloc(ctx, n * 8)) return rc;
    if (slope)
        if (int rc = dslope.alloc(ctx, n * 4)) return rc;
    a.dem = ddem.as<const float>(), a.fallback = dfb.as<const uint8_t>();
    a.words = dwords.as<uint64_t>(), a.slope = dslope.as<float>();
    if (int rc = mfd_dev(ctx, a, tiles_x, tiles, stats)) return rc;
    if (int rc = dwords.download(words, n * 8)) return rc;
    return slope ? dslope.download(slope, n * 4) : HDEM_OK;
}

extern "C" int hdem_mfdacc_u64(hdem_ctx *ctx, const uint64_t *words, int H, int W,
                               const void *weights, int weight_type, int frac_bits, int64_t *sum,
                               float *value, int flags, hdem_mfdacc_stats *stats)
{
    mfdacc_call a = {words, H, W, weights, weight_type, frac_bits, sum, value};
    d8_grid g;
    if (int rc = mfdacc_check(ctx, a, flags, stats, &g)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_mfdacc_stats st = {};
    d8_publish(stats, st);

    const size_t n = (size_t)H * W;
    hdem_dbuf dwords, dweights, dsum, dvalue;
    if (!(flags & HDEM_ON_DEVICE)) {
        if (int rc = dwords.upload(ctx, words, n * 8)) return rc;
        if (int rc = dweights.upload(ctx, weights, n * weight_bytes(weight_type))) return rc;
        if (sum)
            if (int rc = dsum.alloc(ctx, n * 8)) return rc;
        if (value)
            if (int rc = dvalue.alloc(ctx, n * 4)) return rc;
        a.words = dwords.as<const uint64_t>(), a.weights = dweights.p;
        a.sum = dsum.as<int64_t>(), a.value = dvalue.as<float>();
    }
    const int rc = mfdacc_dev(ctx, a, g, stats != nullptr, &st);
    d8_publish(stats, st);
    if (rc || (flags & HDEM_ON_DEVICE)) return rc;
    if (sum)
        if (int rc2 = dsum.download(sum, n * 8)) return rc2;
    return value ? dvalue.download(value, n * 4) : HDEM_OK;
}
