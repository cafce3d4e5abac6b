// A14 / A23  Terrain attributes: Horn gradient, slope, aspect, D8 slope, wetness and stream power
// index from one read of the DEM (include/hydrodem_hip.h has the contract).  A23 is A14 with a
// float32 catchment area in place of the uint32 accumulation and, optionally, a given slope
// raster as the t of twi and spi: further instantiations of the one kernel.
//
// One launch in the shape of the radius-1 kernels of hdem_stencil.hip (hdem_stencil_tile.h):
// a 256-thread workgroup per 256 x 32 cell tile, tile plus halo staged in LDS, a wave owns 8
// rows x 256 columns, a lane produces 4 adjacent cells per row from three rolling rows held
// in registers and stores each wanted output as one 16-byte word.  What differs:
//   * cells outside the raster are staged as NaN, so that "a neighbour that is NaN takes the
//     value of the centre" is the rule for the raster's edge and for nodata alike;
//   * up to eight outputs: each pointer is a kernel argument and its branch is wave-uniform,
//     an output that is not wanted costs neither its store nor its math-library call; the
//     optional inputs (acc or area, given slope, codes) select the instantiation and are read
//     straight from global memory, 4 cells per lane and row;
//   * the row loop is NOT unrolled: atanf, atan2f and logf are inlined four times per row, and
//     eight copies of that (about 8 x 1100 instructions) would not fit the instruction cache;
//   * four counters, summed per lane, then per wave by shuffles, then per workgroup in LDS:
//     one global atomic per workgroup and counter that is not 0.
#include "hdem_d8tile.h"
#include "hdem_stencil_tile.h"

#include <cmath>

namespace {

enum { O_DZDX, O_DZDY, O_TANGENT, O_DEGREES, O_ASPECT, O_D8SLOPE, O_TWI, O_SPI, O_COUNT };
enum { C_NAN, C_FLAT, C_FLOORED, C_INVALID, C_COUNT, C_NONPOSITIVE = C_COUNT, C_COUNT_AREA };
// what twi and spi take as the catchment area: nothing, the uint32 accumulation (A14), the
// float32 area (A23), the float32 area beside a given slope (A23)
enum { A_NONE, A_ACC, A_AREA, A_AREA_GIVEN };

struct terrain_args {
    const float *z;
    const uint32_t *acc;            // A_AREA, A_AREA_GIVEN: the float32 area, as its bits
    const uint8_t *codes;
    float *out[O_COUNT];
    int H, W, tiles_x;
    float rx, ry;                   // z_factor / (8 dx), z_factor / (8 dy)
    float rdx, rdy, rdd;            // z_factor / dx, / dy, / sqrt(dx^2 + dy^2)
    float acell;                    // sqrt(dx dy)
    float min_slope;
    int twi_d8, vec_codes;
    unsigned long long *cnt;        // C_COUNT (A23: C_COUNT_AREA) counters, zeroed by the caller
    const float *given;             // A_AREA_GIVEN: the t of twi and spi
};

constexpr float DEG = (float)(180.0 / 3.14159265358979323846);

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void put4(float *out, size_t at, int x, int W, const float (&v)[4])
{
    float *o = out + at;
    if (x + 4 <= W) {
        hdem_f4 w = {v[0], v[1], v[2], v[3]};
        hdem_st4u(o, w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < W) o[k] = v[k];
    }
}

template <bool D8, int AREA>
__global__ __launch_bounds__(NT) void terrain_kernel(const terrain_args p)
{
    constexpr bool ACC = AREA != A_NONE, GIVEN = AREA == A_AREA_GIVEN;
    constexpr int NC = AREA >= A_AREA ? C_COUNT_AREA : C_COUNT;
    __shared__ __attribute__((aligned(16))) float t[(TH + 2) * LS];
    __shared__ unsigned int s_cnt[NC];
    const int H = p.H, W = p.W;
    const int bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int x0 = bx * TW, y0 = by * TH;
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0;
    stage_tile<float, false, true>(p.z, H, W, y0, x0, t);
    __syncthreads();

    const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int x = x0 + 4 * cg;
    const float nan = __builtin_nanf("");
    const bool t_d8 = D8 && p.twi_d8;
    const bool want_t = p.out[O_TANGENT] || p.out[O_DEGREES] ||
                        (ACC && !GIVEN && !t_d8 && (p.out[O_TWI] || p.out[O_SPI]));
    unsigned int n[NC] = {};
    if (x < W) {
        float a[6], b[6], c[6];
        read_row6(t, rg * 8 + 0, cg, a);
        read_row6(t, rg * 8 + 1, cg, b);
#pragma unroll 1
        for (int rr = 0; rr < 8; ++rr) {
            const int lr = rg * 8 + rr, y = y0 + lr;
            if (y >= H) break;
            read_row6(t, lr + 2, cg, c);
            const size_t at = (size_t)y * W + x;
            uint32_t av[4] = {0, 0, 0, 0};
            uint32_t cd[4] = {0, 0, 0, 0};
            uint32_t gv[4] = {0, 0, 0, 0};
            if (GIVEN) {
                if (x + 4 <= W) {
                    const u32x4u m = *reinterpret_cast<const u32x4u *>(p.given + at);
                    gv[0] = m[0]; gv[1] = m[1]; gv[2] = m[2]; gv[3] = m[3];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (x + k < W) gv[k] = __float_as_uint(p.given[at + k]);
                }
            }
            if (ACC) {
                if (x + 4 <= W) {
                    const u32x4u m = *reinterpret_cast<const u32x4u *>(p.acc + at);
                    av[0] = m[0]; av[1] = m[1]; av[2] = m[2]; av[3] = m[3];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (x + k < W) av[k] = p.acc[at + k];
                }
            }
            if (D8) {
                if (p.vec_codes && x + 4 <= W) {
                    const uint32_t m = *reinterpret_cast<const uint32_t *>(p.codes + at);
                    cd[0] = m & 255u; cd[1] = (m >> 8) & 255u; cd[2] = (m >> 16) & 255u; cd[3] = m >> 24;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (x + k < W) cd[k] = p.codes[at + k];
                }
            }
            float dzdx[4], dzdy[4], tang[4], deg[4], asp[4], dsl[4], twi[4], spi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool inside = x + k < W;
                const float e = b[k + 1];
                const bool hole = e != e;
                n[C_NAN] += inside && hole;
                // a neighbour outside the raster (staged as NaN) or NaN takes the centre's value
                const float wa = a[k] != a[k] ? e : a[k], wb = a[k + 1] != a[k + 1] ? e : a[k + 1];
                const float wc = a[k + 2] != a[k + 2] ? e : a[k + 2], wd = b[k] != b[k] ? e : b[k];
                const float wf = b[k + 2] != b[k + 2] ? e : b[k + 2], wg = c[k] != c[k] ? e : c[k];
                const float wh = c[k + 1] != c[k + 1] ? e : c[k + 1];
                const float wi = c[k + 2] != c[k + 2] ? e : c[k + 2];
                const float fd = wf - wd, hb = wh - wb;
                const float gx = ((wc - wa) + (fd + fd)) + (wi - wg);
                const float gy = ((wg - wa) + (hb + hb)) + (wi - wc);
                const float px = hole ? nan : gx * p.rx, py = hole ? nan : gy * p.ry;
                dzdx[k] = px;
                dzdy[k] = py;
                const bool flat = px == 0.0f && py == 0.0f;
                n[C_FLAT] += inside && flat;
                float tn = 0.0f;
                if (want_t) tn = sqrtf(px * px + py * py);
                tang[k] = tn;
                if (p.out[O_DEGREES]) deg[k] = atanf(tn) * DEG;
                if (p.out[O_ASPECT]) {
                    float d = atan2f(-px, py) * DEG;
                    if (d < 0.0f) d += 360.0f;
                    if (d == 360.0f) d = 0.0f;
                    asp[k] = flat ? -1.0f : d;
                }
                float ds = 0.0f;
                if (D8) {
                    d8_tile here = {};
                    here.y0 = y, here.x0 = x + k;
                    const d8_step s = d8_decode((uint8_t)cd[k], 0, 0, here, H, W);
                    n[C_INVALID] += inside && s.invalid;
                    if (!s.terminal) {      // the raw receiver: LDS row lr + 1 is the centre's
                        const float zr = t[(lr + 1 + s.ny) * LS + 4 + 4 * cg + k + s.nx];
                        const float rd = (s.b & 1) ? p.rdd : (s.b & 2) ? p.rdy : p.rdx;
                        ds = (e - zr) * rd;
                    }
                    if (hole) ds = nan;
                    dsl[k] = ds;
                }
                if (ACC) {
                    const float cells = AREA == A_ACC ? (float)av[k] : __uint_as_float(av[k]);
                    if (AREA >= A_AREA) n[C_NONPOSITIVE] += inside && cells <= 0.0f;
                    const float area = cells * p.acell;
                    const float tt = GIVEN ? (hole ? nan : __uint_as_float(gv[k])) : t_d8 ? ds : tn;
                    if (p.out[O_TWI]) {
                        const bool low = tt < p.min_slope;
                        n[C_FLOORED] += inside && low;
                        twi[k] = logf(area / (low ? p.min_slope : tt));
                    }
                    spi[k] = area * tt;
                }
            }
            if (p.out[O_DZDX]) put4(p.out[O_DZDX], at, x, W, dzdx);
            if (p.out[O_DZDY]) put4(p.out[O_DZDY], at, x, W, dzdy);
            if (p.out[O_TANGENT]) put4(p.out[O_TANGENT], at, x, W, tang);
            if (p.out[O_DEGREES]) put4(p.out[O_DEGREES], at, x, W, deg);
            if (p.out[O_ASPECT]) put4(p.out[O_ASPECT], at, x, W, asp);
            if (D8 && p.out[O_D8SLOPE]) put4(p.out[O_D8SLOPE], at, x, W, dsl);
            if (ACC && p.out[O_TWI]) put4(p.out[O_TWI], at, x, W, twi);
            if (ACC && p.out[O_SPI]) put4(p.out[O_SPI], at, x, W, spi);
#pragma unroll
            for (int k = 0; k < 6; ++k) { a[k] = b[k]; b[k] = c[k]; }
        }
    }
    // lane -> wave -> workgroup -> one global atomic per counter
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        unsigned int v = n[j];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[j], v);
    }
    __syncthreads();
    if (threadIdx.x < NC && s_cnt[threadIdx.x])
        atomicAdd(&p.cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

struct span {
    const char *name;
    uintptr_t lo, hi;
};

// What a call is given: A14 (acc) or A23 (area, given).  `form`: the operator in the texts.
struct terrain_call {
    const float *dem;
    int H, W;
    const uint32_t *acc;
    const float *area, *given;
    const uint8_t *d8;
    double dx, dy, z_factor, min_slope;
    float *out[O_COUNT];
    int flags;
    bool area_form;
};

template <class Stats>
int check_args(const hdem_ctx *ctx, const terrain_call &a, const Stats *stats,
               const char *stats_name, int *tiles_x, int64_t *tiles)
{
    static const char *const names[O_COUNT] = {"dzdx", "dzdy", "tangent", "degrees", "aspect",
                                               "d8_slope", "twi", "spi"};
    const int H = a.H, W = a.W, flags = a.flags;
    HDEM_REQUIRE(ctx, HDEM_ERR_BAD_ARG, "ctx is null");
    HDEM_REQUIRE(a.dem, HDEM_ERR_BAD_ARG, "null raster pointer");
    HDEM_REQUIRE(H > 0 && W > 0, HDEM_ERR_BAD_ARG, "raster dimensions must be positive, got %d x %d",
                 H, W);
    if (int rc = d8_check_stats(stats, stats_name)) return rc;
    const int known = HDEM_TERRAIN_TWI_D8 | (a.area_form ? HDEM_TERRAIN_TWI_GIVEN : 0);
    HDEM_REQUIRE((flags & ~known) == 0, HDEM_ERR_BAD_ARG,
                 "terrain attributes: unknown flags 0x%x", flags);
    bool any = false;
    for (int k = 0; k < O_COUNT; ++k) any |= a.out[k] != nullptr;
    HDEM_REQUIRE(any, HDEM_ERR_BAD_ARG, "terrain attributes: no output wanted");
    if (a.area_form) {
        HDEM_REQUIRE(a.area || (!a.out[O_TWI] && !a.out[O_SPI]), HDEM_ERR_BAD_ARG,
                     "twi and spi need the float32 area raster");
        HDEM_REQUIRE(!(flags & HDEM_TERRAIN_TWI_GIVEN) || !(flags & HDEM_TERRAIN_TWI_D8),
                     HDEM_ERR_BAD_ARG,
                     "HDEM_TERRAIN_TWI_GIVEN and HDEM_TERRAIN_TWI_D8 exclude each other");
        HDEM_REQUIRE(a.given || !(flags & HDEM_TERRAIN_TWI_GIVEN), HDEM_ERR_BAD_ARG,
                     "HDEM_TERRAIN_TWI_GIVEN needs the float32 given_slope raster");
        HDEM_REQUIRE(!a.given || (flags & HDEM_TERRAIN_TWI_GIVEN), HDEM_ERR_BAD_ARG,
                     "a given_slope raster goes with HDEM_TERRAIN_TWI_GIVEN");
    } else {
        HDEM_REQUIRE(a.acc || (!a.out[O_TWI] && !a.out[O_SPI]), HDEM_ERR_BAD_ARG,
                     "twi and spi need the uint32 accumulation raster");
    }
    HDEM_REQUIRE(a.d8 || !a.out[O_D8SLOPE], HDEM_ERR_BAD_ARG, "d8_slope needs the uint8 D8 codes");
    HDEM_REQUIRE(a.d8 || !(flags & HDEM_TERRAIN_TWI_D8), HDEM_ERR_BAD_ARG,
                 "HDEM_TERRAIN_TWI_D8 needs the uint8 D8 codes");
    HDEM_REQUIRE(positive(a.dx) && positive(a.dy), HDEM_ERR_BAD_ARG,
                 "dx and dy must be finite and positive, got %g and %g", a.dx, a.dy);
    HDEM_REQUIRE(positive(a.z_factor), HDEM_ERR_BAD_ARG,
                 "z_factor must be finite and positive, got %g", a.z_factor);
    HDEM_REQUIRE(positive(a.min_slope), HDEM_ERR_BAD_ARG,
                 "min_slope must be finite and positive, got %g", a.min_slope);
    const size_t n = (size_t)H * W;
    span s[5 + O_COUNT];
    int ns = 0;
    s[ns++] = {"dem", (uintptr_t)a.dem, (uintptr_t)a.dem + 4 * n};
    if (a.acc) s[ns++] = {"acc", (uintptr_t)a.acc, (uintptr_t)a.acc + 4 * n};
    if (a.area) s[ns++] = {"area", (uintptr_t)a.area, (uintptr_t)a.area + 4 * n};
    if (a.given) s[ns++] = {"given_slope", (uintptr_t)a.given, (uintptr_t)a.given + 4 * n};
    if (a.d8) s[ns++] = {"d8", (uintptr_t)a.d8, (uintptr_t)a.d8 + n};
    for (int k = 0; k < O_COUNT; ++k) {
        if (!a.out[k]) continue;
        const span o = {names[k], (uintptr_t)a.out[k], (uintptr_t)a.out[k] + 4 * n};
        for (int j = 0; j < ns; ++j)
            HDEM_REQUIRE(o.hi <= s[j].lo || s[j].hi <= o.lo, HDEM_ERR_BAD_ARG,
                         "terrain attributes: %s overlaps %s", o.name, s[j].name);
        s[ns++] = o;
    }
    *tiles_x = (W + TW - 1) / TW;
    *tiles = (int64_t)*tiles_x * ((H + TH - 1) / TH);
    HDEM_REQUIRE(*tiles <= INT32_MAX, HDEM_ERR_BAD_ARG,
                 "terrain attributes: %d x %d has %lld tiles of %d x %d, more than %d", H, W,
                 (long long)*tiles, TH, TW, INT32_MAX);
    return HDEM_OK;
}

template <int AREA>
void launch(hdem_ctx *ctx, bool use_d8, int64_t tiles, const terrain_args &p)
{
    const dim3 grid((unsigned)tiles), block(NT);
    if (use_d8)
        hipLaunchKernelGGL((terrain_kernel<true, AREA>), grid, block, 0, ctx->stream, p);
    else
        hipLaunchKernelGGL((terrain_kernel<false, AREA>), grid, block, 0, ctx->stream, p);
}

// Both forms on device pointers, after their checks.  *st is filled when the launch ran.
int terrain_dev(hdem_ctx *ctx, const terrain_call &a, int tiles_x, int64_t tiles, bool want_stats,
                hdem_terrain_area_stats *st)
{
    float *const twi = a.out[O_TWI], *const spi = a.out[O_SPI];
    // an input no wanted output reads is not read
    const bool twi_d8 = (a.flags & HDEM_TERRAIN_TWI_D8) && (twi || spi);
    const bool given = (a.flags & HDEM_TERRAIN_TWI_GIVEN) && (twi || spi);
    const bool use_acc = twi || spi;
    const bool use_d8 = a.out[O_D8SLOPE] || twi_d8;
    const int ncnt = a.area_form ? C_COUNT_AREA : C_COUNT;
    unsigned long long *cnt =
        static_cast<unsigned long long *>(hdem_arena(ctx, ncnt * sizeof(unsigned long long)));
    if (!cnt) return HDEM_ERR_OOM;

    terrain_args p = {};
    p.z = a.dem;
    p.acc = !use_acc ? nullptr : a.area_form ? reinterpret_cast<const uint32_t *>(a.area) : a.acc;
    p.given = given ? a.given : nullptr;
    p.codes = use_d8 ? a.d8 : nullptr;
    for (int k = 0; k < O_COUNT; ++k) p.out[k] = a.out[k];
    p.H = a.H, p.W = a.W, p.tiles_x = tiles_x;
    p.rx = (float)(a.z_factor / (8.0 * a.dx));
    p.ry = (float)(a.z_factor / (8.0 * a.dy));
    p.rdx = (float)(a.z_factor / a.dx);
    p.rdy = (float)(a.z_factor / a.dy);
    p.rdd = (float)(a.z_factor / std::sqrt(a.dx * a.dx + a.dy * a.dy));
    p.acell = (float)std::sqrt(a.dx * a.dy);
    p.min_slope = (float)a.min_slope;
    p.twi_d8 = twi_d8;
    p.vec_codes = use_d8 && a.W % 4 == 0 && (uintptr_t)a.d8 % 4 == 0;
    p.cnt = cnt;

    hdem_event_timer<2> timer(ctx, want_stats);   // around the launch
    if (int rc = timer.start()) return rc;
    HDEM_HIP_CHECK(hipMemsetAsync(cnt, 0, ncnt * sizeof(unsigned long long), ctx->stream));
    timer.mark(0);
    if (!use_acc) launch<A_NONE>(ctx, use_d8, tiles, p);
    else if (!a.area_form) launch<A_ACC>(ctx, use_d8, tiles, p);
    else if (!given) launch<A_AREA>(ctx, use_d8, tiles, p);
    else launch<A_AREA_GIVEN>(ctx, use_d8, tiles, p);
    timer.mark(1);
    HDEM_HIP_CHECK(hipGetLastError());
    unsigned long long host[C_COUNT_AREA] = {};
    HDEM_HIP_CHECK(hipMemcpyAsync(host, cnt, ncnt * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, ctx->stream));
    HDEM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    st->nan_cells = (int64_t)host[C_NAN];
    st->flat_cells = (int64_t)host[C_FLAT];
    st->floored_cells = (int64_t)host[C_FLOORED];
    st->invalid_codes = (int64_t)host[C_INVALID];
    st->nonpositive_area = (int64_t)host[C_NONPOSITIVE];
    st->ms_total = timer.ms(0, 1);
    return d8_report_invalid(host[C_INVALID]);
}

// hdem_terrain_area_stats opens with the fields of hdem_terrain_stats
static_assert(offsetof(hdem_terrain_area_stats, nonpositive_area) == sizeof(hdem_terrain_stats),
              "the area form's stats no longer open with A14's");
inline hdem_terrain_stats plain_stats(const hdem_terrain_area_stats &st)
{
    hdem_terrain_stats out;
    memcpy(&out, &st, sizeof(out));
    return out;
}

// The host form of both: upload, the device form `dev` on the buffers, download.
template <class Dev>
int terrain_host(hdem_ctx *ctx, terrain_call a, Dev dev)
{
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)a.H * a.W;
    hdem_dbuf ddem, dacc, darea, dgiven, dd8, dout[O_COUNT];
    if (int rc = ddem.upload(ctx, a.dem, n * 4)) return rc;
    if (int rc = dacc.upload(ctx, a.acc, n * 4)) return rc;
    if (int rc = darea.upload(ctx, a.area, n * 4)) return rc;
    if (int rc = dgiven.upload(ctx, a.given, n * 4)) return rc;
    if (int rc = dd8.upload(ctx, a.d8, n)) return rc;
    float *host_out[O_COUNT];
    for (int k = 0; k < O_COUNT; ++k) {
        host_out[k] = a.out[k];
        if (a.out[k])
            if (int rc = dout[k].alloc(ctx, n * 4)) return rc;
        a.out[k] = dout[k].as<float>();
    }
    a.dem = ddem.as<const float>(), a.acc = dacc.as<const uint32_t>();
    a.area = darea.as<const float>(), a.given = dgiven.as<const float>();
    a.d8 = dd8.as<const uint8_t>();
    if (int rc = dev(a)) return rc;
    for (int k = 0; k < O_COUNT; ++k)
        if (host_out[k])
            if (int rc = dout[k].download(host_out[k], n * 4)) return rc;
    return HDEM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int hdem_terrain_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W,
                                    const uint32_t *acc, const uint8_t *d8, double dx, double dy,
                                    double z_factor, double min_slope, float *dzdx, float *dzdy,
                                    float *tangent, float *degrees, float *aspect,
                                    float *d8_slope, float *twi, float *spi, int flags,
                                    hdem_terrain_stats *stats)
{
    const terrain_call a = {dem, H, W, acc, nullptr, nullptr, d8, dx, dy, z_factor, min_slope,
                            {dzdx, dzdy, tangent, degrees, aspect, d8_slope, twi, spi}, flags,
                            false};
    int tiles_x;
    int64_t tiles;
    if (int rc = check_args(ctx, a, stats, "hdem_terrain_stats", &tiles_x, &tiles)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_terrain_area_stats st = {};
    d8_publish(stats, plain_stats(st));
    const int rc = terrain_dev(ctx, a, tiles_x, tiles, stats != nullptr, &st);
    d8_publish(stats, plain_stats(st));
    return rc;
}

extern "C" int hdem_terrain_f32(hdem_ctx *ctx, const float *dem, int H, int W, const uint32_t *acc,
                                const uint8_t *d8, double dx, double dy, double z_factor,
                                double min_slope, float *dzdx, float *dzdy, float *tangent,
                                float *degrees, float *aspect, float *d8_slope, float *twi,
                                float *spi, int flags, hdem_terrain_stats *stats)
{
    const terrain_call a = {dem, H, W, acc, nullptr, nullptr, d8, dx, dy, z_factor, min_slope,
                            {dzdx, dzdy, tangent, degrees, aspect, d8_slope, twi, spi}, flags,
                            false};
    int tiles_x;
    int64_t tiles;
    if (int rc = check_args(ctx, a, stats, "hdem_terrain_stats", &tiles_x, &tiles)) return rc;
    return terrain_host(ctx, a, [&](const terrain_call &d) {
        return hdem_terrain_f32_dev(ctx, d.dem, H, W, d.acc, d.d8, dx, dy, z_factor, min_slope,
                                    d.out[0], d.out[1], d.out[2], d.out[3], d.out[4], d.out[5],
                                    d.out[6], d.out[7], flags, stats);
    });
}

extern "C" int hdem_terrain_area_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W,
                                         const float *area, const float *given_slope,
                                         const uint8_t *d8, double dx, double dy, double z_factor,
                                         double min_slope, float *dzdx, float *dzdy,
                                         float *tangent, float *degrees, float *aspect,
                                         float *d8_slope, float *twi, float *spi, int flags,
                                         hdem_terrain_area_stats *stats)
{
    const terrain_call a = {dem, H, W, nullptr, area, given_slope, d8, dx, dy, z_factor, min_slope,
                            {dzdx, dzdy, tangent, degrees, aspect, d8_slope, twi, spi}, flags,
                            true};
    int tiles_x;
    int64_t tiles;
    if (int rc = check_args(ctx, a, stats, "hdem_terrain_area_stats", &tiles_x, &tiles)) return rc;
    HDEM_HIP_CHECK(hipSetDevice(ctx->device));
    hdem_terrain_area_stats st = {};
    d8_publish(stats, st);
    const int rc = terrain_dev(ctx, a, tiles_x, tiles, stats != nullptr, &st);
    d8_publish(stats, st);
    return rc;
}

extern "C" int hdem_terrain_area_f32(hdem_ctx *ctx, const float *dem, int H, int W,
                                     const float *area, const float *given_slope,
                                     const uint8_t *d8, double dx, double dy, double z_factor,
                                     double min_slope, float *dzdx, float *dzdy, float *tangent,
                                     float *degrees, float *aspect, float *d8_slope, float *twi,
                                     float *spi, int flags, hdem_terrain_area_stats *stats)
{
    const terrain_call a = {dem, H, W, nullptr, area, given_slope, d8, dx, dy, z_factor, min_slope,
                            {dzdx, dzdy, tangent, degrees, aspect, d8_slope, twi, spi}, flags,
                            true};
    int tiles_x;
    int64_t tiles;
    if (int rc = check_args(ctx, a, stats, "hdem_terrain_area_stats", &tiles_x, &tiles)) return rc;
    return terrain_host(ctx, a, [&](const terrain_call &d) {
        return hdem_terrain_area_f32_dev(ctx, d.dem, H, W, d.area, d.given, d.d8, dx, dy, z_factor,
                                         min_slope, d.out[0], d.out[1], d.out[2], d.out[3],
                                         d.out[4], d.out[5], d.out[6], d.out[7], flags, stats);
    });
}
