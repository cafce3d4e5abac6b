/*
 * hydrodem_hip.h -- C ABI of the MI355X (gfx950) raster hot path.
 *
 * This is the drop-in boundary: plain C, caller-owned pointers and sizes, no
 * C++ or torch types, no exceptions.  Every operator entry point replaces the
 * body of one `Filter.apply(ndarray) -> ndarray` of the reference package
 * (`cguerrero/hydrodem/filters/__init__.py:23-39`); the reference-side ctypes
 * stub that binds it is shown in INTEGRATION.md.
 *
 * Conventions
 *   - rasters are C-contiguous row-major, H rows x W columns;
 *   - every function returns an hdem_status; on failure hdem_last_error()
 *     (thread local) holds a message.  Window validation uses the same two
 *     failure classes as `sliding_window.py:150-156`
 *     (HDEM_ERR_WINDOW_HIGH / HDEM_ERR_WINDOW_EVEN);
 *   - `*_f32(...)` entry points take HOST pointers, run synchronously
 *     (upload, kernels, download) and never keep or free caller memory;
 *   - `*_dev(...)` entry points take DEVICE pointers, enqueue on the context's
 *     stream and return without synchronising (except sink fill, which has to
 *     read its convergence counter);
 *   - there is no CPU fallback anywhere behind this header.
 */
#ifndef HYDRODEM_HIP_H
#define HYDRODEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdem_ctx hdem_ctx;

typedef enum hdem_status {
    HDEM_OK = 0,
    HDEM_ERR_BAD_ARG = 1,       /* null pointer, non-positive size, ...      */
    HDEM_ERR_WINDOW_EVEN = 2,   /* -> WindowSizeEvenError                    */
    HDEM_ERR_WINDOW_HIGH = 3,   /* -> WindowSizeHighError                    */
    HDEM_ERR_HIP = 4,           /* a HIP runtime call failed                 */
    HDEM_ERR_NOT_CONVERGED = 5, /* sink fill hit max_rounds                  */
    HDEM_ERR_NO_DEVICE = 6,
    HDEM_ERR_OOM = 7
} hdem_status;

/* ---- life cycle -------------------------------------------------------- */
const char *hdem_last_error(void);
int hdem_version(void);                       /* 100*major + minor          */
int hdem_device_count(int *count);
int hdem_init(int device, hdem_ctx **ctx);    /* own stream + workspace     */
int hdem_shutdown(hdem_ctx *ctx);
/* Run on a caller-provided hipStream_t (e.g. torch's current stream);
 * NULL restores the context's own stream.  When the stream changes, the new stream is
 * ordered behind everything this context has queued on the old one (an event recorded there,
 * hipStreamWaitEvent on the new stream; no host wait): the context's scratch -- the arena,
 * the Fourier scratch and plans, the fill workspace -- goes with it, and an operator that
 * returned without a host wait may still be using it.  Both streams must be alive at the
 * call.  Setting the stream that is already in use does nothing. */
int hdem_set_stream(hdem_ctx *ctx, void *hip_stream);
int hdem_synchronize(hdem_ctx *ctx);

/* ---- device memory (so that a host needs nothing but this library) ------
 * hdem_free keeps the block (up to a quarter of the device's memory, at most 64 GiB;
 * HDEM_POOL_MIB in the environment: another figure, 0 = none) and hdem_malloc hands it out
 * again for a request of that size or up to an eighth less; the new owner's stream waits
 * for whatever the context's stream held at the time of the free -- no host wait, no
 * hipMalloc / hipFree in a chain of operators that allocates at every call.  A block is
 * handed back on the context it came from; hdem_shutdown returns everything.
 * Contract (single stream): when hdem_free is called, every use of the block must have been
 * enqueued on THIS context's stream (or be complete).  A block that another context, or a
 * stream of the caller's own, still works on must be synchronised by the caller before it is
 * freed (hdem_synchronize on that context); a context whose stream was changed with
 * hdem_set_stream since the block was handed out waits for the whole device in hdem_free.
 * hdem_trim gives the cached blocks (and the scratch buffers the context keeps between calls)
 * back to the device -- for a process that shares the GPU with another allocator (a second
 * context, torch); every allocation the library makes for itself does the same before it
 * reports HDEM_ERR_OOM.  *released (may be NULL): bytes returned.  hdem_trim is safe at any
 * point between two calls: what a later call still needs stays.  While a hub start is prepared
 * (hdem_fill_hub_prepare_dev, until the fill that takes its levels) the buffer that holds it is
 * not freed and its bytes are not counted in *released. */
int hdem_malloc(hdem_ctx *ctx, size_t bytes, void **dptr);
int hdem_free(hdem_ctx *ctx, void *dptr);
int hdem_trim(hdem_ctx *ctx, size_t *released);
/* Scribble mode, for tests (off by default; byte = -1 turns it off again, 0 ... 255 on).
 * While it is on the library fills, with that byte, every block hdem_malloc hands out (fresh
 * or from the cache, its whole size), every allocation it makes for itself, and -- at each
 * call of an operator that uses it -- exactly the part of the context's scratch arena the
 * operator asks for.  Each fill runs on the context's stream and is waited for.  The sink
 * fill's workspace and its coarse and hub buffers carry state from call to call and are only
 * filled when they are allocated.  An operator whose result depends on the byte reads memory
 * it never wrote; with the mode off the only cost is a branch at those three places. */
int hdem_set_scribble(hdem_ctx *ctx, int byte);
int hdem_memcpy_h2d(hdem_ctx *ctx, void *dst, const void *src, size_t bytes);
int hdem_memcpy_d2h(hdem_ctx *ctx, void *dst, const void *src, size_t bytes);
int hdem_memcpy_d2d(hdem_ctx *ctx, void *dst, const void *src, size_t bytes);
/* A byte fill on the context's stream (0xff bytes make a raster of NaN: the canvas of
 * HydroConditioning.apply_batch). */
int hdem_memset_dev(hdem_ctx *ctx, void *dptr, int byte, size_t bytes);
/* Raster I/O seam (utils_dem.py:17-40 reads / writes whole arrays):
 * page-locked host buffers and copies ordered on the context's stream, so that a band
 * of a raster can be read into pinned memory, processed and written back while the
 * next band is in flight on another context.  hdem_synchronize() waits. */
int hdem_host_alloc(hdem_ctx *ctx, size_t bytes, void **hptr);
int hdem_host_free(hdem_ctx *ctx, void *hptr);
int hdem_memcpy_h2d_async(hdem_ctx *ctx, void *dst, const void *src, size_t bytes);
int hdem_memcpy_d2h_async(hdem_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ---- per-kernel timing (HIP events on the stream the kernels run on) ---- */
typedef enum hdem_kernel_id {
    HDEM_K_D8 = 0,
    HDEM_K_FILL_INIT = 1,
    HDEM_K_FILL_TILE = 2,     /* sink fill: asynchronous tile relaxation (dominant) */
    HDEM_K_BOXMEAN = 3,
    HDEM_K_GROVES = 4,        /* fused quadratic + groves epilogue          */
    HDEM_K_CONVOLVE = 5,
    HDEM_K_COPY = 6,          /* hdem_copy_rate_dev: the measured copy roof       */
    HDEM_K_FILL_ROUND = 7,    /* certifying stream + finishing rounds of tile visits */
    HDEM_K_BLOCKMAX = 8,      /* block-maximum coarsening (multi-GPU start values) */
    HDEM_K_FFT = 9,           /* rocFFT 2-D complex transform (forward or inverse) */
    HDEM_K_FOURIER_ROWSUM = 10, /* hollow mean, row pass                       */
    HDEM_K_FOURIER_DETECT = 11, /* hollow mean, column pass + peak decision    */
    HDEM_K_FOURIER_MASK = 12,   /* isolated points, expand, apply to spectrum  */
    HDEM_K_FOURIER_POINT = 13,  /* real->complex, |F| of a quadrant, |f|/N     */
    HDEM_K_LAGOON = 14,         /* lagoon branch: NaN repair, morphology, dilation */
    HDEM_K_MAJORITY = 15,       /* majority vote over the circular window       */
    HDEM_K_FILL_COARSE = 16,    /* sink fill: asynchronous launch of the coarse pre-solve */
    HDEM_K_FILL_FLAT = 17,      /* sink fill: interiors of the tiles that ended flat      */
    HDEM_K_ELEMENTWISE = 18,    /* element-wise operators on device rasters               */
    HDEM_K_FILL_HUB = 19,       /* sink fill: hub start (in-tile path costs + hub raster)  */
    HDEM_K_FLOWACC = 20,        /* D8 flow accumulation: its four launches together        */
    HDEM_K_COUNT = 21
} hdem_kernel_id;

typedef struct hdem_kernel_stat {
    int64_t launches;
    double  ms;               /* sum of event-timed launch durations        */
    int64_t units;            /* cells (or tile-visit cells) processed      */
} hdem_kernel_stat;

int hdem_profile_enable(hdem_ctx *ctx, int on);   /* default off            */
int hdem_profile_reset(hdem_ctx *ctx);
/* synchronises the stream, then reports the totals since the last reset */
int hdem_profile_get(hdem_ctx *ctx, int kernel_id, hdem_kernel_stat *out);

/* ---- A2  D8FlowDirection.apply  (new operator; no reference body --------
 * SURVEY F2; tie rule of custom_filters.py:193-195).  ESRI codes, uint8. */
int hdem_d8_f32(hdem_ctx *ctx, const float *z, int H, int W, uint8_t *out);
int hdem_d8_f32_dev(hdem_ctx *ctx, const float *z, int H, int W, uint8_t *out);

/* ---- A1  SinkFill.apply  (new operator; no reference body -- SURVEY F2) -- */
typedef struct hdem_fill_stats {
    int32_t rounds;           /* round-synchronous launches that had work (0: the
                                 certifying stream found the surface final)     */
    int32_t converged;        /* 1: certified fixed point                      */
    int64_t tile_visits;      /* tile visits, both drivers                     */
    int64_t tiles;            /* tiles in the raster                         */
    int32_t tile_h, tile_w;   /* tile shape in cells                         */
    int32_t visits_flat;      /* of tile_visits: tiles under one flat level, settled from
                                 their halo ring alone (no window load)         */
    int32_t async_timed_out;  /* != 0: the asynchronous launch gave up (wall-clock
                                 budget); the round driver finished the fill     */
    int64_t iterations;       /* 4-scan iterations, summed over tile visits  */
    int64_t visits_unchanged; /* visits that found nothing to lower          */
    int64_t visits_requeued;  /* visits that hit the iteration cap           */
    int64_t round_visits;     /* of tile_visits: made by the round driver    */
    int64_t pending;          /* tiles still queued when a time slice ended  */
    int32_t partial_residency;/* 1: some workgroups of the asynchronous launch were not
                                 resident within 200 us (the GPU is shared); the others
                                 started without them and took their tiles       */
    int32_t flat_unchanged;   /* of visits_flat: those that found nothing to lower (they are
                                 part of visits_unchanged as well)               */
    int64_t deferred_visits;  /* of tile_visits / visits_unchanged: made by HDEM_FILL_DEFER  */
    int64_t deferred_unchanged; /* calls before this one, which is the first to report them */
} hdem_fill_stats;

#define HDEM_FILL_INIT        0x0  /* w is output only: pinned ring <- z, rest from above */
#define HDEM_FILL_WARM        0x1  /* w holds a valid upper bound; the one-cell ring of w
                                      is the Dirichlet boundary (never written)           */
#define HDEM_FILL_ACT_ALL     0x0  /* WARM: every tile starts active                      */
#define HDEM_FILL_ACT_TOP     0x2  /* WARM: only tiles touching row 1 ...                 */
#define HDEM_FILL_ACT_BOTTOM  0x4  /* ... and/or row H-2 start active (after a halo       */
                                   /* exchange replaced ghost row 0 / H-1)                */
#define HDEM_FILL_SYNC_ONLY   0x40 /* skip the asynchronous phase (round-synchronous only) */
#define HDEM_FILL_NO_VERIFY   0x80 /* skip the certifying pass behind the asynchronous
                                      phase: for intermediate solves of a halo-exchange loop
                                      whose last solve is a verifying one                  */
#define HDEM_FILL_RESUME      0x100 /* WARM: keep the worklist the previous call on this context
                                      left (a time slice that ended with tiles queued);
                                      ACT_TOP / ACT_BOTTOM add the tile rows next to a replaced
                                      ghost row.  Implies NO_VERIFY.                      */
#define HDEM_FILL_GHOST_TOP   0x10 /* INIT: row 0 / row H-1 is a ghost row owned by the   */
#define HDEM_FILL_GHOST_BOTTOM 0x20 /* neighbouring row block: starts at +inf, not at Z    */
#define HDEM_FILL_NO_COARSE   0x400 /* INIT: start every free cell at +inf.  Without this flag a
                                      raster of >= 6000^2 cells (eps = 0, no ghost rows) is first
                                      filled on its 16 x 16 block maxima -- 1/256 of the cells --
                                      and the free cells start at their block's filled level, an
                                      upper bound of the fill: same bits, ~15 % less time.     */
#define HDEM_FILL_GHOST_GIVEN 0x200 /* INIT with GHOST_TOP / GHOST_BOTTOM: the ghost rows of w
                                      already hold upper bounds of the filled surface (the
                                      caller's guess, e.g. from a coarse solve): start from
                                      those instead of +inf.  Must be >= the true fill.    */

#define HDEM_FILL_DEFER       0x800 /* WARM | RESUME: enqueue the solve and return without
                                      waiting for it and without reading anything back: for the
                                      correcting solves of a halo-exchange loop that keeps its
                                      decisions on the device (hdem_set_fill_seam_words).  The
                                      call's counters are added to those of the next call on this
                                      problem that does wait; stats->pending is -1.          */

/* eps = 0 gives flats (exact, order-independent, bit-reproducible);
 * eps > 0 is the Planchon-Darboux gradient.  max_rounds <= 0 -> default.
 *
 * Input contract of the three fill entry points: every elevation of z is a finite float32, or
 * NaN for nodata.  Any sign and any magnitude up to FLT_MAX is supported and gives the bits of
 * the definition (negative and zero-crossing terrain, +0 / -0, relief far below or eps far
 * below one ulp, elevations above 3.0e38: tests/test_gpu_elevation_regimes.py).  +inf and
 * -inf are NOT supported: +inf is what a tile visit reads a nodata wall as, so an interior
 * +inf cell comes back as NaN from a tile that was visited and as +inf from one that never
 * was -- the result depends on the visit history.  Replace infinities by NaN (nodata) or by a
 * finite value before the call. */
int hdem_sinkfill_f32(hdem_ctx *ctx, const float *z, int H, int W, float eps,
                      int max_rounds, float *w, hdem_fill_stats *stats);
int hdem_sinkfill_f32_dev(hdem_ctx *ctx, const float *z, int H, int W,
                          float eps, int max_rounds, int flags, float *w,
                          hdem_fill_stats *stats);
/* Sink fill and D8 of the filled surface in one call (what HydroConditioning and the
 * headline benchmark run).  The certifying pass of the fill streams over Z and W once;
 * with this entry point it writes the flow directions on the way instead of a second pass
 * over w (same codes as hdem_d8_f32_dev, bit for bit; falls back to that kernel when the
 * call has no certifying pass over the whole raster). */
int hdem_sinkfill_d8_f32_dev(hdem_ctx *ctx, const float *z, int H, int W, float eps,
                             int max_rounds, int flags, float *w, uint8_t *d8,
                             hdem_fill_stats *stats);
/* Time slice of the asynchronous phase in microseconds (0 = run to convergence, the
 * default).  With a slice, an INIT/WARM call that has HDEM_FILL_NO_VERIFY returns
 * HDEM_OK with stats->pending > 0 when the slice ended first; continue with
 * HDEM_FILL_WARM | HDEM_FILL_RESUME.  This is what lets row blocks on different
 * GPUs trade ghost rows every millisecond instead of once per local convergence. */
int hdem_set_fill_slice_us(hdem_ctx *ctx, int microseconds);
/* Seam words of a halo-exchange loop that does not come back to the host between a seam
 * exchange and the solve behind it (new work; partition.py).  `words`: three ints in
 * device memory, owned by the caller, valid until the next call replaces them (NULL: none):
 *   words[1], words[2]   written by the caller on the stream before a HDEM_FILL_DEFER call:
 *                        non-zero = ghost row 0 / H-1 was replaced by different values.  The
 *                        call's HDEM_FILL_ACT_TOP / ACT_BOTTOM then only act when the word is set;
 *   words[0]             written by every HDEM_FILL_DEFER call, on the stream, when its launch has
 *                        ended: 1 = tiles are still queued (a time slice ended first), else 0.
 * The words are read and written by kernels on the context's stream, never by the host. */
int hdem_set_fill_seam_words(hdem_ctx *ctx, int *words);
/* The bookkeeping of one seam exchange as one launch on the context's stream (device pointers):
 * recv_top / recv_bot (W floats each, NULL: no such neighbour) replace row 0 / row H-1 of w;
 * words[1] / words[2] <- that row's bits changed; words[0] <- pending > 0 when pending >= 0
 * (pending < 0: words[0] is what the last deferred call left there); words[3] <- any of
 * words[0..2], the word the ranks MAX-reduce.  `words`: four ints, the first three as above. */
int hdem_fill_seam_apply_dev(hdem_ctx *ctx, float *w, int H, int W, const float *recv_top,
                             const float *recv_bot, int64_t pending, int *words);

/* Hub start of a row-block partition (new work; no reference counterpart -- SURVEY 8e).  The
 * single-GPU fill starts from a graph of tile hubs (one hub per 62 x 62 tile, path costs d to
 * it inside the tile, cheapest crossings between hubs of neighbouring tiles, the graph filled
 * exactly as a small raster: hdem_sinkfill.hip).  A partition builds ONE such graph:
 *   hdem_fill_hub_prepare_dev   d of this block into the interior of w (flags: GHOST_TOP /
 *                               GHOST_BOTTOM as for the fill); the caller then puts the rows of
 *                               the neighbours' d that are its ghost rows into w's ghost rows;
 *   hdem_fill_hub_raster_dev    this block's hub raster, (2 ty + 1) x (2 tx + 1) floats with
 *                               ty x tx = ceil((H - 2) / 62) x ceil((W - 2) / 62) tiles: hubs at
 *                               odd/odd, crossings between them; the first (last) row holds the
 *                               crossings to the raster's first (last) row, or -- ghost row -- to
 *                               the neighbouring block's hubs;
 *   hdem_set_fill_hub_levels    the filled levels of this block's part of the stacked raster
 *                               (same shape), for the next INIT fill of the same z / w: that fill
 *                               skips its own start-value work; with GHOST_GIVEN the ghost rows
 *                               of w are the caller's upper bounds.  Used once: the next call of
 *                               hdem_sinkfill_f32_dev or hdem_sinkfill_d8_f32_dev on this context
 *                               takes them, whether it is refused or not (a
 *                               fill of another z / w, shape or kind is refused).
 * A context holds one preparation, in a buffer that its own fills use too.  When a fill that
 * takes a hub start of its own, or a preparation of another block, has used that buffer since
 * the prepare, hdem_fill_hub_raster_dev returns HDEM_ERR_BAD_ARG ("the prepared hub start was
 * overwritten") and drops the preparation: prepare again.  Once the raster is made the buffer is
 * free: the fill of the (stacked) hub raster may take a hub start of its own, and
 * hdem_set_fill_hub_levels and the fill behind it work as before. */
int hdem_fill_hub_prepare_dev(hdem_ctx *ctx, const float *z, int H, int W, int flags, float *w);
int hdem_fill_hub_raster_dev(hdem_ctx *ctx, float *raster);
int hdem_set_fill_hub_levels(hdem_ctx *ctx, const float *levels);
/* Start values for the NEXT hdem_sinkfill_f32_dev INIT call with eps = 0 on this context:
 * coarse_filled is the sink fill of a block-maximum raster (hdem_blockmax_f32_dev) that
 * covers this raster -- ch x cw floats on the device, block a power of two in 4..256;
 * free cells (and ghost rows) start at max(z, coarse level of their block).  row_map
 * (device, H ints, or NULL for y / block) gives the coarse row of each raster row: a row
 * block of a partitioned raster points into the stacked coarse raster of all ranks.
 * The fill that takes the start returns HDEM_ERR_BAD_ARG, before any launch, when the coarse
 * raster does not cover its raster: (W - 1) / block >= cw, or -- without a row map --
 * (H - 1) / block >= ch.  With a row map the rows cannot be checked on the host: every entry
 * of the map must be in 0 .. ch - 1, which is the caller's responsibility.
 * Used once: the next call of hdem_sinkfill_f32_dev or hdem_sinkfill_d8_f32_dev on this
 * context takes it, whether it is refused or not, and whether it is a call
 * that can start from it or not; NULL clears it. */
int hdem_set_fill_coarse_start(hdem_ctx *ctx, const float *coarse_filled, int ch, int cw,
                               int block, const int32_t *row_map);

/* Block maximum: out[i][j] = max of z over rows [i*b, (i+1)*b) x columns [j*b, (j+1)*b)
 * (clipped to the raster; a block with a NaN cell gives FLT_MAX), b a power of two in
 * 4..256, out is ceil(H/b) x ceil(W/b).  The sink fill of this coarse raster bounds the
 * sink fill of z from above cell by cell -- the multi-GPU path uses it as the start value
 * of the ghost rows (new work; the reference is single process). */
int hdem_blockmax_f32_dev(hdem_ctx *ctx, const float *z, int H, int W, int b, float *out);

/* Measurement aid ("report % of measured copy bandwidth as well as % of
 * nominal"): a plain 16-byte-per-lane device copy of `bytes` bytes (a multiple of 16,
 * both pointers 16-byte aligned), timed under HDEM_K_COPY (units = bytes copied); it moves
 * 2 * bytes through HBM.  bench.py quotes every kernel against the rate it reaches. */
int hdem_copy_rate_dev(hdem_ctx *ctx, const void *src, void *dst, size_t bytes);

/* ---- element-wise operators ------------------------------------
 * LowerThan / GreaterThan / BooleanToInteger / ProductFilter / AdditionFilter /
 * SubtractionFilter.apply, simple_filters.py:7-275, on device rasters, so that the
 * orchestration's algebra (hydro_dem_process.py:60-91, and the three-term sum in front
 * of PostProcessingFinal, :148-149) stays in HBM between the stencils:
 *     out[i] = op(image[i], operand ? operand[i] : scalar),  i < n.
 * Rasters are HDEM_T_F32 / HDEM_T_F64 / HDEM_T_U8 (masks); evaluated in double, stored
 * as out_type (comparisons and NONZERO give 0 / 1). */
typedef enum hdem_ew_op {
    HDEM_EW_MUL = 0,      /* operand * image      ProductFilter     :165-180 */
    HDEM_EW_ADD = 1,      /* operand + image      AdditionFilter    :214-229 */
    HDEM_EW_RSUB = 2,     /* operand - image      SubtractionFilter :261-275 */
    HDEM_EW_GT = 3,       /* image > operand      GreaterThan       :81-96   */
    HDEM_EW_LT = 4,       /* image < operand      LowerThan         :35-50   */
    HDEM_EW_NONZERO = 5   /* image != 0           BooleanToInteger  :113-131 (bool * 1) */
} hdem_ew_op;
typedef enum hdem_dtype { HDEM_T_F32 = 0, HDEM_T_F64 = 1, HDEM_T_U8 = 2, HDEM_T_I64 = 3 } hdem_dtype;
int hdem_elementwise_dev(hdem_ctx *ctx, int op, const void *image, int image_type,
                         const void *operand, int operand_type, double scalar, int64_t n,
                         void *out, int out_type);

/* ---- A8  Fourier destripe ------------------------------------
 * DetectApplyFourier.apply, custom_filters.py:1083-1101, with FourierInitial
 * (:834-877), FourierProcessQuarters (:880-1050) and MaskFourier (:537-561)
 * inside: out = | ifft2( (1 - mask) * fft2(dem) ) |, the mask found on the
 * magnitude of the two upper quadrants of the shifted spectrum.  float32 /
 * complex64 throughout (scipy.fftpack keeps float32 input single; the reference
 * then drifts to complex128 for the inverse: values agree to ~1e-5 m).
 * mask (optional, H*W bytes): the reference's masks_fourier in shifted
 * coordinates.  Quadrants smaller than the 55-cell window give
 * HDEM_ERR_WINDOW_HIGH, as the reference's window constructor does. */
int hdem_fourier_destripe_f32(hdem_ctx *ctx, const float *dem, int H, int W,
                              float *out, uint8_t *mask);
int hdem_fourier_destripe_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W,
                                  float *out, uint8_t *mask);
/* BlanksFourier.apply (:400-429), `window` odd in 7..201 (the reference's pipeline: 55),
 * inner 5, factor 4: found[i] = 1 where q > 4 x hollow mean; q is rewritten as
 * q * (1 - found). */
int hdem_blanks_fourier_f32_dev(hdem_ctx *ctx, float *q, int h, int w, int window,
                                uint8_t *found);
/* IsolatedPoints.apply (:344-366) and ExpandFilter.apply (:103-125) on byte masks. */
int hdem_isolated_points_u8_dev(hdem_ctx *ctx, const uint8_t *mask, int h, int w,
                                int window, uint8_t *out);
int hdem_expand_u8_dev(hdem_ctx *ctx, const uint8_t *mask, int h, int w, int window,
                       uint8_t *out);
/* FourierTransform / FourierITransform (extension_filters.py:348-414) on an
 * interleaved complex64 H x W array, in place; the inverse is unnormalised
 * (scipy's ifft2 = this / (H*W)). */
int hdem_fft2_c2c_f32_dev(hdem_ctx *ctx, float *data, int H, int W, int inverse);
/* ... and on an interleaved complex128 array: what scipy.fftpack computes for float64 /
 * complex128 input (extension_filters.py:379,414).  Plan made and released per call. */
int hdem_fft2_c2c_f64_dev(hdem_ctx *ctx, double *data, int H, int W, int inverse);

/* ---- SURVEY 8f-3  HydroSHEDS / lagoon branch --------------------------------
 * CorrectNANValues.apply (custom_filters.py:287-317): cells < 0 whose `window` (odd, 3..11;
 * the reference's pipeline: 3) fits <- float32 mean of the window's other cells >= 0, summed
 * as NumPy sums them (NaN when there is none). */
int hdem_correct_nan_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W, int window,
                             float *out);
/* MajorityFilter.apply (:44-73): value held by > 70 % of (window^2 - 1) cells of the
 * window minus its corners, else 0; window odd, 3..15. */
int hdem_majority_f32_dev(hdem_ctx *ctx, const float *img, int H, int W, int window,
                          float *out);
/* scipy.ndimage.binary_erosion(iterations) / binary_closing(structure)
 * (extension_filters.py:187-293): byte masks, border_value 0; structure = sh x sw bytes,
 * odd sizes up to 7, NULL = the 3 x 3 cross.  tmp: a scratch mask of the same size
 * (may be NULL for a single erosion). */
int hdem_binary_erosion_u8_dev(hdem_ctx *ctx, const uint8_t *mask, int H, int W,
                               const uint8_t *structure, int sh, int sw, int iterations,
                               uint8_t *tmp, uint8_t *out);
int hdem_binary_closing_u8_dev(hdem_ctx *ctx, const uint8_t *mask, int H, int W,
                               const uint8_t *structure, int sh, int sw, uint8_t *tmp,
                               uint8_t *out);
/* scipy.ndimage.grey_dilation(size=(sy, sx)) (extension_filters.py:296-345): flat
 * maximum filter, mode 'reflect', odd sizes. */
int hdem_grey_dilation_f32_dev(hdem_ctx *ctx, const float *img, int H, int W, int sy, int sx,
                               float *out);
int hdem_grey_dilation_f64_dev(hdem_ctx *ctx, const double *img, int H, int W, int sy, int sx,
                               double *out);
/* TidyingLagoons.apply (:564-610) and LagoonsDetection.apply (:613-661), device
 * resident.  fixed / values (may be NULL): the reference's hsheds_nan_fixed and
 * lagoons_values; mask: 1 where lagoons_values > 0. */
int hdem_tidying_lagoons_f32_dev(hdem_ctx *ctx, const float *img, int H, int W, float *out);
int hdem_lagoons_detection_f32_dev(hdem_ctx *ctx, const float *hsheds, int H, int W,
                                   float *fixed, float *values, uint8_t *mask);

/* ---- A5  Convolve.apply + Around.apply -----------------------------------
 * extension_filters.py:166-184 (scipy.ndimage.convolve, mode='reflect',
 * double accumulation, result / weights.size) and :113-130 (np.around).
 * boxmean3 is the ones((3,3)) default fused with the optional rounding
 * (PostProcessingFinal, custom_filters.py:1124-1125). */
int hdem_boxmean3_f32(hdem_ctx *ctx, const float *x, int H, int W,
                      int do_round, float *out);
int hdem_boxmean3_f64(hdem_ctx *ctx, const double *x, int H, int W,
                      int do_round, double *out);
int hdem_boxmean3_f32_dev(hdem_ctx *ctx, const float *x, int H, int W,
                          int do_round, float *out);
int hdem_boxmean3_f64_dev(hdem_ctx *ctx, const double *x, int H, int W,
                          int do_round, double *out);
/* general odd kh x kw weights (host pointer, row-major doubles), <= 15x15 */
int hdem_convolve_f32(hdem_ctx *ctx, const float *x, int H, int W,
                      const double *weights, int kh, int kw, float *out);
int hdem_convolve_f64(hdem_ctx *ctx, const double *x, int H, int W,
                      const double *weights, int kh, int kw, double *out);
int hdem_around_f32(hdem_ctx *ctx, const float *x, int64_t n, float *out);
int hdem_around_f64(hdem_ctx *ctx, const double *x, int64_t n, double *out);

/* ---- A3  QuadraticFilter.apply  (custom_filters.py:226-257) -------------
 * ws odd and <= min(H, W) (sliding_window.py:150-156); border ring of ws/2
 * cells is returned unchanged (custom_filters.py:249). */
int hdem_quadratic_f32(hdem_ctx *ctx, const float *dem, int H, int W, int ws,
                       float *out);
int hdem_quadratic_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W,
                           int ws, float *out);

/* ---- A4  GrovesCorrection / GrovesCorrectionsIter.apply -----------------
 * custom_filters.py:708-732,755-767 with MaskTallGroves :533-534 fused:
 *   smooth = quadratic(img); hl = img - smooth; m = groves && hl > thr;
 *   out = m ? smooth : hl + smooth;   repeated `iters` times.
 * groves: uint8, non-zero = groves class.  scratch_dev (iters > 1) is a
 * second H*W float device buffer for the ping-pong; may be NULL for the
 * host-pointer variant. */
int hdem_groves_f32(hdem_ctx *ctx, const float *img, const uint8_t *groves,
                    int H, int W, int ws, float thr, int iters, float *out);
int hdem_groves_f32_dev(hdem_ctx *ctx, const float *img, const uint8_t *groves,
                        int H, int W, int ws, float thr, int iters,
                        float *scratch_dev, float *out);

/* ---- A5  FlowAccumulation.apply  (new operator: D8 flow accumulation) ---
 * d8: uint8 ESRI codes as hdem_d8_f32 writes them (E=1, SE=2, S=4, SW=8, W=16, NW=32,
 * N=64, NE=128).  Code 0, or a code pointing outside the raster, makes a cell terminal;
 * any other byte is invalid.  out: uint32, acc[c] = the number of cells whose D8 path
 * passes through c, c itself included (every cell >= 1): the unique solution of
 * acc[c] = 1 + sum acc[d] over the neighbours d whose code points at c.  Nodata cells of
 * a DEM get code 0 from D8 and are never chosen as a receiver, so they read 1.  Integers:
 * bit-exact and run-to-run identical.
 * HDEM_ERR_BAD_ARG, in bounded time, for an invalid byte, for codes that form a cycle
 * ("flow directions form a cycle: N cells never drain"; the codes of hdem_d8_f32 always
 * point to a strictly lower cell and cannot), and -- before any allocation or launch --
 * for H * W > 2^32 - 1.  On error the contents of out are unspecified.
 * Workspace: about 1.5 B per cell from the context's arena.  The _dev form synchronises
 * the context's stream to read its validity counters (as sink fill does).  stats may be
 * NULL; the three phase times are filled only while profiling is on
 * (hdem_profile_enable), and the whole call is timed under HDEM_K_FLOWACC. */
typedef struct hdem_flowacc_stats {
    int64_t exits;       /* nodes of the exit forest (cells draining into another tile) */
    int32_t max_hops;    /* longest walk of phase B (tile crossings)                    */
    int32_t tile_h, tile_w;
    float ms_tile;       /* phase A: in-tile pass (HIP events; profiling only)          */
    float ms_forest;     /* phase B: exit forest                                        */
    float ms_final;      /* phase C: in-tile pass again, writes out                     */
} hdem_flowacc_stats;
int hdem_flowacc_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, uint32_t *out,
                    hdem_flowacc_stats *stats);          /* host pointers, synchronous */
int hdem_flowacc_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, uint32_t *out,
                        hdem_flowacc_stats *stats);      /* device pointers */

/* ---- A6  Watersheds.apply  (new operator: D8 watershed labelling) -------
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).  out: uint32 labels.
 *   seeds == NULL, flags == 0   outlet mode: label[c] = 1 + flat index (y * W + x) of the
 *       terminal cell that c's D8 path ends in; a terminal cell labels itself.
 *   seeds != NULL               pour-point mode: seeds is uint32 H x W, 0 = no pour point,
 *       anything else that cell's label.  label[c] = the seed of the first seeded cell on
 *       c's path, c included; 0 when the path reaches a terminal cell without meeting one.
 *   flags == HDEM_WS_COMPACT    outlet mode with labels 1 ... K, K = stats.basins = the
 *       number of terminal cells, and outlets[k - 1] = flat index of the outlet of label k.
 *       outlets is required then (and only then) and must have room for H * W entries
 *       (every cell may be terminal); the host form writes K of them.  The numbering
 *       is by tile (row-major), then row-major inside a 64 x 64 tile: fixed for a raster,
 *       the same from both entry points, not row-major over the raster.
 * Exact integers, identical from run to run.  HDEM_ERR_BAD_ARG, in bounded time, for an
 * invalid byte, for codes that form a cycle ("N cells never resolve"; in pour-point mode
 * a loop that holds a seeded cell resolves there and is legal), for compact together with
 * seeds, for unknown flags and -- before any allocation or launch -- for
 * H * W > 2^32 - 1.  On error the contents of out and outlets are unspecified.
 * Workspace: about 2.1 B per cell from the context's arena.  The _dev form synchronises
 * the context's stream to read its validity counters.  stats may be NULL; otherwise the
 * caller sets stats->struct_size = sizeof(hdem_watershed_stats) first (48 bytes in this
 * version; a shorter struct is filled as far as it goes).  The three phase times are
 * filled only while profiling is on (hdem_profile_enable); the call has no kernel id. */
#define HDEM_WS_COMPACT 1
typedef struct hdem_watershed_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_watershed_stats), set by the caller          */
    int32_t forest_rounds;  /* pointer-jumping launches of phase B that had work to do      */
    int64_t basins;         /* terminal cells: K, the number of basins of the outlet modes  */
    int64_t exits;          /* unseeded cells draining into another tile                    */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: in-tile pointer doubling (HIP events; profiling)    */
    float ms_forest;        /* phase B: the forest of perimeter slots                       */
    float ms_final;         /* phase C: labels written                                      */
    int32_t reserved;       /* 0                                                            */
} hdem_watershed_stats;     /* sizeof == 48 */
int hdem_watershed_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const uint32_t *seeds,
                      int flags, uint32_t *out, uint32_t *outlets,
                      hdem_watershed_stats *stats);      /* host pointers, synchronous */
int hdem_watershed_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W,
                          const uint32_t *seeds, int flags, uint32_t *out, uint32_t *outlets,
                          hdem_watershed_stats *stats);  /* device pointers */

/* ---- A7  FlowDistance.apply / HeightAboveDrainage.apply  (new operators: D8 flow trace) --
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).
 * A stop is a terminal cell or, when streams are given, a stream cell.  For every cell c the
 * call follows c's D8 path, c included, to the first stop s(c) and counts the cardinal
 * (E, S, W, N) and diagonal (SE, SW, NW, NE) steps taken, ncard(c) and ndiag(c); a stop has
 * s = itself and both counts 0.
 *   stream_kind == HDEM_FT_STREAMS_NONE     streams == NULL, threshold == 0: every path ends at
 *       a terminal cell (distance to the outlet); no cell is unreached.
 *   stream_kind == HDEM_FT_STREAMS_MASK_U8  streams is uint8 H x W, non-zero = stream;
 *       threshold == 0.
 *   stream_kind == HDEM_FT_STREAMS_ACC_U32  streams is uint32 H x W (a flow accumulation as
 *       hdem_flowacc_u8 writes it), stream <=> streams[c] >= threshold, threshold >= 1.
 * With streams, a cell whose stop is a terminal cell that is no stream cell is unreached, and
 * so is that terminal cell.
 * Outputs, all H x W, each may be NULL (not wanted), at least one must not be:
 *   stop      uint32   1 + flat index (y * W + x) of s(c); 0 for an unreached cell
 *   ncard     uint32   cardinal steps; for an unreached cell those to the terminal cell the
 *   ndiag     uint32   diagonal steps    path ends in
 *   distance  float32  (float)((double)ncard * cellsize + (double)ndiag * (cellsize * sqrt(2.0))),
 *                      one rounding per operation, no fused multiply-add; NaN when unreached
 *   hand      float32  dem[c] - dem[s(c)], one float32 subtraction; NaN when unreached.  Needs
 *                      dem, float32 H x W; NaN in dem propagates by arithmetic.
 * dem may be NULL when hand is.  cellsize must be finite and > 0.  flags must be 0.
 * Exact, identical from run to run.  HDEM_ERR_BAD_ARG, in bounded time, for an invalid byte,
 * for codes that form a cycle ("N cells never resolve"; a loop that holds a stream cell ends
 * there and is legal), for the argument combinations excluded above and -- before any
 * allocation or launch -- for H * W > 2^32 - 1.  On error the contents of the outputs are
 * unspecified.
 * Workspace: about 8.0 B per cell from the context's arena (6 B per cell, two arrays of
 * 16-byte nodes per tile-perimeter slot).  The _dev form synchronises the context's stream to
 * read its validity counters.  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_flowtrace_stats) first (56 bytes in this version; a shorter
 * struct is filled as far as it goes).  The three phase times are filled only while profiling
 * is on (hdem_profile_enable); the call has no kernel id. */
#define HDEM_FT_STREAMS_NONE 0
#define HDEM_FT_STREAMS_MASK_U8 1
#define HDEM_FT_STREAMS_ACC_U32 2
typedef struct hdem_flowtrace_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_flowtrace_stats), set by the caller          */
    int32_t forest_rounds;  /* pointer-jumping launches of phase B that had work to do      */
    int64_t stops;          /* stop cells: stream cells and terminal cells                  */
    int64_t unreached;      /* cells whose path ends in a terminal cell that is no stream   */
    int64_t exits;          /* cells that are no stop and drain into another tile           */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: in-tile pointer doubling (HIP events; profiling)    */
    float ms_forest;        /* phase B: the forest of perimeter slots                       */
    float ms_final;         /* phase C: outputs written                                     */
    int32_t reserved;       /* 0                                                            */
} hdem_flowtrace_stats;     /* sizeof == 56 */
int hdem_flowtrace_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                      int stream_kind, uint32_t threshold, const float *dem, double cellsize,
                      uint32_t *stop, uint32_t *ncard, uint32_t *ndiag, float *distance,
                      float *hand, int flags,
                      hdem_flowtrace_stats *stats);      /* host pointers, synchronous */
int hdem_flowtrace_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                          int stream_kind, uint32_t threshold, const float *dem,
                          double cellsize, uint32_t *stop, uint32_t *ncard, uint32_t *ndiag,
                          float *distance, float *hand, int flags,
                          hdem_flowtrace_stats *stats);  /* device pointers */

/* ---- A8  ResolveFlats.apply  (new operator: D8 directions across flats) --
 * d8: uint8 ESRI codes as hdem_d8_f32 writes them; dem: the float32 H x W raster they were
 * made on, NaN = nodata.  hdem_d8_f32 only routes strictly downhill, so every cell of a flat
 * (all of a filled depression after an epsilon = 0 sink fill) has code 0.  This call points
 * the cells of a flat towards the nearest way out of it.  "Equal" is float ==: -0.0 equals
 * 0.0, NaN equals nothing.
 *   drains S   non-NaN cells with a code != 0, or on the one-cell raster ring, or with a NaN
 *              8-neighbour
 *   flat   F   every other non-NaN cell (interior, code 0, no nodata neighbour)
 *   dist[c]    c in F: the length k >= 1 of the shortest 8-connected path c = p0, ..., pk with
 *              every dem[pi] == dem[c], p0 ... p(k-1) in F and pk in S; infinite when there is
 *              no such path (a pit of an unfilled DEM)
 *   out[c]     c in F with finite dist: the code of the first neighbour n in D8 window order
 *              (NW, N, NE, W, E, SW, S, SE) with dem[n] == dem[c] and dist[n] == dist[c] - 1,
 *              cells of S counting as 0; every other cell: d8[c]
 * dist strictly decreases along the new codes, so out is acyclic whenever d8 is.  It is the
 * unique solution of dist[c] = 1 + min over equal neighbours (0 in S, else dist), which the
 * call checks at every flat cell before it returns.  After an epsilon = 0 fill no cell is
 * unresolved and the interior cells left at 0 are the nodata cells and their neighbours.
 * Rasters of H < 3 or W < 3 have no flat cell: out = d8.
 * dist (may be NULL): uint32 H x W, 0 outside F, k at resolved cells, 0xFFFFFFFF at unresolved
 * ones.  out may be d8 itself (in place); no other overlap between the rasters is allowed.
 * flags must be 0.  Exact integers, identical from run to run and independent of the schedule.
 * HDEM_ERR_BAD_ARG for a byte that is not 0 or a power of two (the text of the other D8
 * operators), for unknown flags and -- before any allocation or launch -- for
 * H * W > 2^32 - 1; HDEM_ERR_NOT_CONVERGED if the check of the local equation fails.  On error
 * the contents of out and dist are unspecified.
 * Workspace from the context's arena: 4 B per cell (the distances) when dist is NULL, else
 * nothing per cell -- dist is worked in; 12 B per 64 x 64 tile either way.  The _dev form
 * synchronises the context's stream once per relaxation round (it reads how many tiles the
 * next round has).  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_resolve_flats_stats) first (64 bytes in this version; a
 * shorter struct is filled as far as it goes).  The three phase times are filled only while
 * profiling is on (hdem_profile_enable); the call has no kernel id. */
typedef struct hdem_resolve_flats_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_resolve_flats_stats), set by the caller      */
    int32_t rounds;         /* relaxation rounds that had work (launches of tile visits)    */
    int64_t flat_cells;     /* cells of F                                                   */
    int64_t unresolved;     /* cells of F with no path to a drain                           */
    int64_t tile_visits;    /* tiles relaxed, summed over the rounds                        */
    uint32_t max_distance;  /* the largest finite dist                                      */
    int32_t active_tiles;   /* tiles that hold a cell of F: the visits of the first round   */
    int32_t tile_h, tile_w;
    float ms_classify;      /* F and S told apart (HIP events; profiling only)              */
    float ms_relax;         /* the rounds, host reads included                              */
    float ms_final;         /* codes written, result checked                                */
    int32_t reserved;       /* 0                                                            */
} hdem_resolve_flats_stats; /* sizeof == 64 */
int hdem_resolve_flats_u8(hdem_ctx *ctx, const uint8_t *d8, const float *dem, int H, int W,
                          uint8_t *out, uint32_t *dist, int flags,
                          hdem_resolve_flats_stats *stats);      /* host pointers, synchronous */
int hdem_resolve_flats_u8_dev(hdem_ctx *ctx, const uint8_t *d8, const float *dem, int H, int W,
                              uint8_t *out, uint32_t *dist, int flags,
                              hdem_resolve_flats_stats *stats);  /* device pointers */

/* ---- A9  Depressions.apply / DepressionInventory.apply  (new operators: depression
 *          labelling and inventory) ------------------------------------------------------
 * dem, filled: float32 H x W; any such pair is legal, not only a raster and its sink fill.
 *   raised(c)    filled[c] > dem[c], a float compare: false when either value is NaN
 *   depression   an 8-connected component D of raised cells; first(D) is its smallest flat
 *                index y * W + x
 * hdem_depressions_f32 writes uint32 labels:
 *   flags == 0                   label[c] = 1 + first(D) for c in D, 0 where c is not raised
 *   flags == HDEM_DEPR_COMPACT   the depressions numbered 1 ... K in ascending order of first
 *       (K = stats.depressions): the numbering of scipy.ndimage.label with the 3 x 3
 *       structure, which numbers components in scan order of their first cell.
 * hdem_depression_table_f32 takes the compact labels of that pair and K and writes one row per
 * label k = 1 ... K into the columns (index k - 1); each column may be NULL (not wanted), at
 * least one must not be:
 *   first       uint32   first(D)
 *   area        uint32   the number of cells
 *   level       float32  the minimum of filled over D (after an epsilon = 0 fill every cell of
 *                        a depression holds it)
 *   max_depth   float32  the maximum of filled[c] - dem[c], one float32 subtraction per cell
 *   volume_q20  uint64   the sum of min(rint((double)(filled[c] - dem[c]) * 2^20), 2^31 - 1):
 *                        depth in fixed point with a quantum of 2^-20, round to nearest even,
 *                        saturating just under 2048; an integer sum cannot overflow here
 *                        (2^32 cells x 2^31 < 2^63)
 * K == 0 is legal and launches nothing.  Labels and every column are an order-independent
 * reduction (min, max, integer add): exact, identical from run to run and independent of the
 * schedule, and so are the three counters of the stats.
 * HDEM_ERR_BAD_ARG for unknown flags, for H * W > 2^32 - 1 -- before any allocation or launch
 * -- and, from the table call, in bounded time, for a label > K and for a labelled cell that
 * is not raised ("the labels do not belong to these rasters: N cells").  Every loop of the
 * union-find carries an iteration cap; HDEM_ERR_NOT_CONVERGED if one is ever reached.  On
 * error the contents of the outputs are unspecified.
 * Workspace from the context's arena: none per cell for the labelling (the label raster is
 * its own union-find forest), 12 B per 64 cells (0.19 B per cell) more for the compact
 * numbering, 512 B for the table.  The _dev forms synchronise the context's stream to read K
 * and their validity counters.  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_depressions_stats) first (56 bytes in this version; a
 * shorter struct is filled as far as it goes).  The three phase times are filled only while
 * profiling is on (hdem_profile_enable); the calls have no kernel id. */
#define HDEM_DEPR_COMPACT 1
typedef struct hdem_depressions_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_depressions_stats), set by the caller        */
    int32_t reserved;       /* 0                                                            */
    int64_t depressions;    /* K                                                            */
    int64_t raised_cells;
    int64_t tile_components; /* components of phase A, summed over the 64 x 64 tiles        */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: components inside a tile (HIP events; profiling)    */
    float ms_seam;          /* phase B: unions across the tile seams                        */
    float ms_final;         /* phase C: roots flattened, labels written and numbered        */
    int32_t reserved2;      /* 0                                                            */
} hdem_depressions_stats;   /* sizeof == 56 */
int hdem_depressions_f32(hdem_ctx *ctx, const float *dem, const float *filled, int H, int W,
                         int flags, uint32_t *labels,
                         hdem_depressions_stats *stats);         /* host pointers, synchronous */
int hdem_depressions_f32_dev(hdem_ctx *ctx, const float *dem, const float *filled, int H, int W,
                             int flags, uint32_t *labels,
                             hdem_depressions_stats *stats);     /* device pointers */
int hdem_depression_table_f32(hdem_ctx *ctx, const float *dem, const float *filled,
                              const uint32_t *labels, int H, int W, int64_t K, uint32_t *first,
                              uint32_t *area, float *level, float *max_depth,
                              uint64_t *volume_q20);             /* host pointers, synchronous */
int hdem_depression_table_f32_dev(hdem_ctx *ctx, const float *dem, const float *filled,
                                  const uint32_t *labels, int H, int W, int64_t K,
                                  uint32_t *first, uint32_t *area, float *level,
                                  float *max_depth, uint64_t *volume_q20);  /* device pointers */

/* ---- A10  UpstreamFlowLength.apply  (new operator: longest upstream D8 flow length) --
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).
 * A donor of c is a neighbour whose code points at c.  For every cell
 *   up(c) = (0, 0)                                   if c has no donor
 *   up(c) = max over donors d of  up(d) + step(d)    otherwise
 *   step(d) = (1, 0) for E, S, W, N;  (0, 1) for SE, SW, NW, NE
 * the (cardinal, diagonal) steps of the longest D8 path that ends in c.  Pairs (ncard, ndiag)
 * are ordered by the real number ncard + ndiag * sqrt(2), and that order is decided exactly,
 * in integers: with da = a1 - a2 and db = b1 - b2, both >= 0: greater unless both are 0; both
 * <= 0: not greater; mixed signs: da^2 against 2 db^2.  sqrt(2) is irrational, so two
 * different pairs never tie, and no float key is ever compared ((8119, 0) and (0, 5741) have
 * the same float32 length).
 * Outputs, all H x W, each may be NULL (not wanted), at least one must not be:
 *   ncard     uint32   the components of up(c)
 *   ndiag     uint32
 *   length    float32  (float)((double)ncard * cellsize + (double)ndiag * (cellsize * sqrt(2.0))),
 *                      one rounding per operation, no fused multiply-add: hdem_flowtrace_u8's
 *                      distance formula
 * cellsize must be finite and > 0.  flags must be 0.
 * Exact integers, identical from run to run and independent of the schedule.
 * HDEM_ERR_BAD_ARG, in bounded time, for an invalid byte, for codes that form a cycle
 * ("N cells never drain"), for the argument combinations excluded above and -- before any
 * allocation or launch -- for H * W > 2^32 - 1.  Every retry loop carries a cap;
 * HDEM_ERR_NOT_CONVERGED if one is ever reached.  On error the contents of the outputs are
 * unspecified.
 * Workspace: 36 B per tile-perimeter slot, about 2.2 B per cell, from the context's arena.
 * The _dev form synchronises the context's stream once to read its counters.  stats may be
 * NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_upstream_stats) first (48
 * bytes in this version; a shorter struct is filled as far as it goes).  The three phase times
 * are filled only while profiling is on (hdem_profile_enable); the call has no kernel id. */
typedef struct hdem_upstream_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_upstream_stats), set by the caller           */
    int32_t max_hops;       /* tile crossings of the longest walk over the exit forest      */
    int64_t exits;          /* cells that drain into another tile: nodes of the exit forest */
    int64_t heads;          /* cells without a donor                                        */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: in-tile walks, perimeter paths (HIP events; profiling) */
    float ms_forest;        /* phase B: the exit forest                                     */
    float ms_final;         /* phase C: seeded in-tile walks, outputs written               */
    int32_t reserved;       /* 0                                                            */
} hdem_upstream_stats;      /* sizeof == 48 */
int hdem_upstream_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, double cellsize,
                     uint32_t *ncard, uint32_t *ndiag, float *length, int flags,
                     hdem_upstream_stats *stats);        /* host pointers, synchronous */
int hdem_upstream_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, double cellsize,
                         uint32_t *ncard, uint32_t *ndiag, float *length, int flags,
                         hdem_upstream_stats *stats);    /* device pointers */

/* ---- A11  StreamOrder.apply  (new operator: Strahler order, Shreve magnitude, stream links) --
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).
 * The stream set S is given as hdem_flowtrace_u8 takes its streams:
 *   stream_kind == HDEM_FT_STREAMS_NONE     streams == NULL, threshold == 0: every cell is in S
 *   stream_kind == HDEM_FT_STREAMS_MASK_U8  streams is uint8 H x W, non-zero = in S; threshold 0
 *   stream_kind == HDEM_FT_STREAMS_ACC_U32  streams is uint32 H x W, in S where >= threshold;
 *                                           threshold >= 1
 * A stream donor of c is a neighbour in S whose code points at c.  For c not in S all three
 * outputs are 0.  For c in S:
 *   order(c)      1 without a stream donor; else, with m the greatest order among its stream
 *                 donors, m + 1 when two or more of them have order m, else m (orders 2, 2, 2
 *                 give 3; 2, 2, 3 give 3; eight donors of order 1 give 2)
 *   magnitude(c)  1 without a stream donor, else the sum of its stream donors' magnitudes: the
 *                 number of heads (stream cells without a stream donor) upstream, c included
 *   link(c)       1 + the flat index of the last cell of c's link: the first cell b on c's D8
 *                 path (c included) that is terminal, or whose receiver is not in S, or whose
 *                 receiver has two or more stream donors.  Order and magnitude are constant on
 *                 a link; the ids are pour points as hdem_watershed_u8 takes them
 * Outputs, all H x W, each may be NULL (not wanted), at least one must not be:
 *   order      uint8    (at most 33 for H * W <= 2^32 - 1)
 *   magnitude  uint32
 *   link       uint32
 * flags must be 0.  Exact integers, identical from run to run and independent of the schedule.
 * HDEM_ERR_BAD_ARG, in bounded time, for an invalid byte, for codes that form a cycle (a loop
 * of stream cells, with or without a tributary joining it, and a loop that holds no stream
 * cell; a loop that leaves the streams and comes back is cut where it leaves them, as
 * hdem_flowtrace_u8 cuts a loop that holds a stream cell), for the argument combinations
 * excluded above and -- before any allocation or launch -- for
 * H * W > 2^32 - 1.  Every retry loop carries a cap; HDEM_ERR_NOT_CONVERGED if one is ever
 * reached.  On error the contents of the outputs are unspecified.
 * Workspace, from the context's arena: 10 B per cell (14 B when link is NULL) next to the
 * flow trace's own 6 B per cell and 32 B per tile-perimeter slot.
 * The _dev form synchronises the context's stream twice (after the first-stop trace, which
 * is hdem_flowtrace_u8_dev's, and to read its own counters).  stats may be NULL; otherwise the
 * caller sets stats->struct_size = sizeof(hdem_streamorder_stats) first (64 bytes in this
 * version; a shorter struct is filled as far as it goes).  The three phase times are filled
 * only while profiling is on (hdem_profile_enable); the call has no kernel id. */
typedef struct hdem_streamorder_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_streamorder_stats), set by the caller          */
    int32_t max_order;      /* the greatest order (0 without a stream cell)                   */
    int64_t stream_cells;   /* cells in S                                                     */
    int64_t heads;          /* stream cells without a stream donor                            */
    int64_t junctions;      /* stream cells with two or more stream donors                    */
    int64_t links;          /* links: nodes of the link graph                                 */
    int32_t max_hops;       /* links of the longest walk over the link graph                  */
    int32_t tile_h, tile_w;
    float ms_nodes;         /* node pass + first stop of every cell (HIP events; profiling)   */
    float ms_walk;          /* the walk over the link graph                                   */
    float ms_gather;        /* outputs written                                                */
} hdem_streamorder_stats;   /* sizeof == 64 */
int hdem_streamorder_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                        int stream_kind, uint32_t threshold, uint8_t *order,
                        uint32_t *magnitude, uint32_t *link, int flags,
                        hdem_streamorder_stats *stats);      /* host pointers, synchronous */
int hdem_streamorder_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                            int stream_kind, uint32_t threshold, uint8_t *order,
                            uint32_t *magnitude, uint32_t *link, int flags,
                            hdem_streamorder_stats *stats);  /* device pointers */

/* ---- A12  StreamNetwork.apply  (new operator: the stream network as a table, one row per link) --
 * d8, streams, stream_kind, threshold: the codes and the stream set S exactly as A11 takes
 * them; stream donors, nin(c) (their number), links and link ends as A11 defines them.
 * link (required): the uint32 H x W link raster hdem_streamorder_u8 wrote for these codes and
 * this S; K = its hdem_streamorder_stats.links.  order_raster (uint8), magnitude_raster
 * (uint32) of that call and dem (float32), all H x W, may be NULL; cellsize is finite and > 0.
 * The links are numbered 0 ... K - 1 in ascending flat index of their end cell b, the cell c
 * with link[c] == 1 + c.  Row r of every column describes link r.  The columns, K entries each:
 *   end        uint32   flat index of b (the link id is 1 + end)
 *   top        uint32   flat index of the link's first cell: its one cell with nin != 1 (a head,
 *                       nin = 0, or a junction cell, nin >= 2)
 *   down       uint32   the row of the link that holds b's receiver when that receiver is in S;
 *                       0xFFFFFFFF when b is terminal or its receiver is off S
 *   order      uint8    order_raster[b]      (needs order_raster)
 *   magnitude  uint32   magnitude_raster[b]  (needs magnitude_raster)
 *   cells      uint32   the number of cells of the link
 *   ncard      uint32   cardinal and diagonal steps of the D8 path from top to b, plus b's own
 *   ndiag      uint32   step when down is a link: every step between two stream cells belongs
 *                       to exactly one link, ncard + ndiag == cells - 1 + (down is a link), and
 *                       lengths add up along down
 *   length     float32  (float)((double)ncard * cellsize + (double)ndiag * (cellsize * sqrt(2.0))),
 *                       one rounding per operation, no fused multiply-add: hdem_flowtrace_u8's
 *                       distance formula
 *   catchment  uint32   the number of cells, on or off S, whose first stream cell on their D8
 *                       path (themselves included) lies in the link: the area of the catchment
 *                       hdem_watershed_u8 draws with the link ids as pour points.  A cell whose
 *                       path never meets a stream counts nowhere
 *   z_top      float32  dem[top]   (needs dem; NaN passes through)
 *   z_end      float32  dem[end]
 * and one raster, row (uint32 H x W): 1 + r on the cells of link r, 0 off the streams -- the
 * compact link ids, pour points whose watershed labels index the table.
 * Each column and row may be NULL (not wanted), at least one of the thirteen must not be.
 * flags must be 0.  K == 0 is legal: row is zeroed when wanted and nothing else is launched.
 * Every column is an integer sum, a count or a gather: exact, identical from run to run and
 * independent of the schedule.
 * HDEM_ERR_BAD_ARG -- before any allocation or launch -- for H * W > 2^32 - 1, unknown flags, a
 * cellsize that is not finite and > 0, K outside 0 ... H * W, z_top or z_end without dem,
 * order or magnitude without its raster, and no output at all.  HDEM_ERR_BAD_ARG in bounded
 * time (counters read at the call's synchronisations; there is no walk) for an invalid byte
 * and with "the links do not belong to these codes and streams" for a link raster that fails
 * one of: link[c] == 0 off S; on S a link id that is not 0, lies inside the raster and names a
 * cell that is its own end; a stream cell that is no end hands its id to a receiver in S; a
 * stream cell with one stream donor carries that donor's id (so no end drains into a cell with
 * nin < 2); the number of ends and the number of stream cells with nin != 1 both equal K.  A
 * rank is compared with K before it indexes a column: a wrong K writes nowhere outside them.
 * HDEM_ERR_NOT_CONVERGED if a probe of the per-tile table ever reaches its cap (the table
 * size).  On error the contents of the outputs are unspecified.
 * Workspace, from the context's arena: 12 B per 64 cells (0.19 B per cell); with catchment and
 * a stream set other than every cell, 4 B per cell next to the flow trace's own 6 B per cell
 * and 32 B per tile-perimeter slot; 8 B per link when length is wanted without ncard and ndiag.
 * The _dev form synchronises the context's stream once to read its counters, and once more
 * inside hdem_flowtrace_u8_dev when that runs (catchment wanted, stream_kind not
 * HDEM_FT_STREAMS_NONE: where every cell is a stream cell, each is its own first stream cell).
 * stats may be NULL; otherwise the caller sets stats->struct_size =
 * sizeof(hdem_streamlinks_stats) first (64 bytes in this version; a shorter struct is filled as
 * far as it goes).  The four step times are filled only while profiling is on
 * (hdem_profile_enable); the call has no kernel id. */
typedef struct hdem_streamlinks_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_streamlinks_stats), set by the caller         */
    int32_t reserved;        /* 0                                                             */
    int64_t links;           /* cells that are their own end: K for a link raster that fits   */
    int64_t stream_cells;    /* cells in S                                                    */
    int64_t catchment_cells; /* cells that reach a stream (the sum of catchment); counted     */
                             /* only when catchment is wanted                                 */
    int64_t tops;            /* stream cells with nin != 1: K again                           */
    int32_t tile_h, tile_w;
    float ms_rank;           /* ends, scan (HIP events; profiling)                            */
    float ms_trace;          /* first stream cell of every cell; 0 when it does not run       */
    float ms_tile;           /* the tile pass                                                 */
    float ms_final;          /* the end pass and length                                       */
} hdem_streamlinks_stats;    /* sizeof == 64 */
int hdem_streamlinks_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                        int stream_kind, uint32_t threshold, const uint32_t *link,
                        const uint8_t *order_raster, const uint32_t *magnitude_raster,
                        const float *dem, double cellsize, int64_t K, uint32_t *end,
                        uint32_t *top, uint32_t *down, uint8_t *order, uint32_t *magnitude,
                        uint32_t *cells, uint32_t *ncard, uint32_t *ndiag, float *length,
                        uint32_t *catchment, float *z_top, float *z_end, uint32_t *row,
                        int flags, hdem_streamlinks_stats *stats);  /* host pointers, synchronous */
int hdem_streamlinks_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                            int stream_kind, uint32_t threshold, const uint32_t *link,
                            const uint8_t *order_raster, const uint32_t *magnitude_raster,
                            const float *dem, double cellsize, int64_t K, uint32_t *end,
                            uint32_t *top, uint32_t *down, uint8_t *order, uint32_t *magnitude,
                            uint32_t *cells, uint32_t *ncard, uint32_t *ndiag, float *length,
                            uint32_t *catchment, float *z_top, float *z_end, uint32_t *row,
                            int flags, hdem_streamlinks_stats *stats);  /* device pointers */

/* ---- A13  ZonalStatistics.apply  (new operator: zonal statistics, one row per zone) --
 * zones: a uint32 H x W label raster, 0 = no zone.  The ids lie in 1 ... H * W, which every
 * label raster of this library satisfies (outlet labels 1 + flat index, compact labels, link
 * ids, the row raster of A12, depression labels in both modes); a caller with arbitrary
 * pour-point labels relabels first.  values (may be NULL): an H x W raster of value_type.
 * The K ids present are numbered 0 ... K - 1 in ascending order (the order of np.unique); row r
 * of every column describes the r-th id.  The columns, K entries each:
 *   id         uint32   the zone's id
 *   count      uint32   its cells
 *   first      uint32   its smallest flat index y * W + x
 *   row_min, row_max, col_min, col_max   uint32   its bounding box, inclusive
 * and, with values:
 *   valid      uint32   its cells whose value is not NaN (integer types: == count)
 *   min, max   the value type   ordered by the order-preserving integer key of float32 (-0.0
 *                       below +0.0, +-inf take part); NaN (float32) or 0 (integer types) for a
 *                       zone with valid == 0
 *   at_min, at_max   uint32   the flat index of a cell that holds the min / max, the smallest
 *                       on ties; 0xFFFFFFFF where valid == 0.  Gathered as one 64-bit word per
 *                       row: key << 32 | index under an unsigned min, key << 32 | ~index under
 *                       an unsigned max
 *   sum        uint64   the exact sum of uint8 / uint32 values; for float32 the int64 sum of
 *                       q(v) = clamp(llrint((double)v * 2^frac_bits), +-(2^31 - 1)), rounding
 *                       to nearest even; NaN cells add nothing, cells that clamp are counted
 *                       (stats.clamped).  2^32 - 1 cells of 2^31 cannot overflow it.
 * frac_bits is 0 ... 30 (16 resolves 1.5e-5 and holds |v| < 32768); it is ignored for the
 * integer types.  The mean is not a column: sum / 2^frac_bits / valid.
 * hdem_zonal_count_u32 returns K (in *K, may be NULL, and in stats.zones); the table call takes
 * it, as A12 takes its count, and redoes the ranks (one more read of zones, one bitmap) rather
 * than keeping state in the context between two calls.  Every column pointer may be NULL (not
 * wanted), at least one must not be; flags must be 0.  K == 0 is legal when the raster holds no
 * zone: nothing is written.  Every column is a count, a min, a max or an integer sum: exact,
 * identical from run to run, independent of the schedule and of what the workspace held.
 * hdem_zonal_broadcast_dev: out[c] = column[row of zones[c]] for a column of K 4-byte words
 * (device pointer), fill where zones[c] == 0: the raster form.
 * HDEM_ERR_BAD_ARG -- before any allocation or launch -- for H * W > 2^32 - 1, unknown flags or
 * value type, values without a type or a type without values, a value column without values,
 * frac_bits or K out of range, no column at all.  HDEM_ERR_BAD_ARG in bounded time (counters
 * read at the call's one synchronisation; there is no walk) for an id above H * W (the message
 * names the number of cells and the largest id) and for a K that is not the number of ids
 * present; a rank is compared with K before it indexes a column, so such a call writes nothing
 * outside the columns.  HDEM_ERR_NOT_CONVERGED if a probe of the per-tile id set ever reaches
 * its cap (its size, which a tile cannot fill).  On error the contents of the outputs are
 * unspecified.
 * Workspace, from the context's arena: 12 B per 64 cells (0.19 B per cell), 16 B per zone when
 * min, max, at_min or at_max is wanted.  Each _dev call synchronises the context's stream once.
 * stats may be NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_zonal_stats)
 * first (80 bytes in this version; a shorter struct is filled as far as it goes).  The step
 * times are filled only while profiling is on; the calls have no kernel id. */
typedef enum hdem_zonal_value_type {
    HDEM_ZONAL_NONE = 0,
    HDEM_ZONAL_F32 = 1,
    HDEM_ZONAL_U32 = 2,
    HDEM_ZONAL_U8 = 3
} hdem_zonal_value_type;
typedef struct hdem_zonal_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_zonal_stats), set by the caller               */
    int32_t reserved;        /* 0                                                             */
    int64_t zones;           /* K: the ids present                                            */
    int64_t unzoned;         /* cells with id 0                                               */
    int64_t clamped;         /* float32 cells whose q(v) was clamped (table call, sum or not) */
    int64_t overflow;        /* cells whose run found no slot in its tile's table and added   */
                             /* to the columns directly (legal; table call)                   */
    int64_t over_range;      /* cells with an id above H * W: refused                         */
    int64_t capped;          /* probes of the id set that reached their cap: refused          */
    uint32_t max_id;         /* the largest id                                                */
    int32_t tile_h, tile_w;
    float ms_rank;           /* bitmap, counts, scan (HIP events; profiling)                  */
    float ms_tile;           /* column init and the tile pass                                 */
    float ms_final;          /* min / max unpacking and the ids                               */
} hdem_zonal_stats;          /* sizeof == 80 */
int hdem_zonal_count_u32(hdem_ctx *ctx, const uint32_t *zones, int H, int W, int64_t *K,
                         hdem_zonal_stats *stats);  /* host pointers, synchronous */
int hdem_zonal_count_u32_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W, int64_t *K,
                             hdem_zonal_stats *stats);  /* device pointer */
int hdem_zonal_table_u32(hdem_ctx *ctx, const uint32_t *zones, int H, int W, const void *values,
                         int value_type, int frac_bits, int64_t K, uint32_t *id, uint32_t *count,
                         uint32_t *first, uint32_t *row_min, uint32_t *row_max, uint32_t *col_min,
                         uint32_t *col_max, uint32_t *valid, void *min, void *max,
                         uint32_t *at_min, uint32_t *at_max, void *sum, int flags,
                         hdem_zonal_stats *stats);  /* host pointers, synchronous */
int hdem_zonal_table_u32_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W,
                             const void *values, int value_type, int frac_bits, int64_t K,
                             uint32_t *id, uint32_t *count, uint32_t *first, uint32_t *row_min,
                             uint32_t *row_max, uint32_t *col_min, uint32_t *col_max,
                             uint32_t *valid, void *min, void *max, uint32_t *at_min,
                             uint32_t *at_max, void *sum, int flags,
                             hdem_zonal_stats *stats);  /* device pointers */
int hdem_zonal_broadcast_dev(hdem_ctx *ctx, const uint32_t *zones, int H, int W, int64_t K,
                             const void *column, uint32_t fill, void *out);  /* device pointers */

/* ---- A14  TerrainAttributes.apply  (new operator: slope, aspect, D8 slope, wetness index) ----
 * dem: float32 H x W, NaN is nodata, +-inf are ordinary values.  One launch of a radius-1
 * stencil writes any subset of eight float32 H x W rasters from one read of the DEM.
 * Window of a cell e, rows growing southwards:   a b c / d e f / g h i.
 * Edge rule: a neighbour outside the raster or NaN takes the value of e; a NaN e gives NaN in
 * every output.
 * Float32 throughout, one rounding per operation in exactly this order, no fused multiply-add;
 * the scale factors are computed in double and rounded once: rx = (float)(z_factor / (8 dx)),
 * ry = (float)(z_factor / (8 dy)).
 *   gx = ((c - a) + ((f - d) + (f - d))) + (i - g)        dzdx = gx * rx
 *   gy = ((g - a) + ((h - b) + (h - b))) + (i - c)        dzdy = gy * ry
 *   s2 = dzdx * dzdx + dzdy * dzdy                         tangent = sqrtf(s2)
 *   degrees = atanf(tangent) * (float)(180 / pi)
 *   aspect  = atan2f(-dzdx, dzdy) * (float)(180 / pi), + 360.0f where negative, 0 where that
 *             rounds to 360, -1 where dzdx == 0 && dzdy == 0: the compass direction of the
 *             steepest descent, clockwise from north
 *   d8_slope = (e - z_r) * rd with z_r the raw value of the cell the D8 code of e points at (not
 *             centre-replaced: NaN if it is NaN) and rd = (float)(z_factor / dx), (z_factor / dy)
 *             or (z_factor / sqrt(dx^2 + dy^2)) for an E / W, N / S or diagonal step; 0 for
 *             code 0 and for a code pointing outside the raster
 *   a   = (float)acc * (float)sqrt(dx * dy)                t = tangent, or d8_slope with
 *                                                          HDEM_TERRAIN_TWI_D8
 *   twi = logf(a / (t < min_slope ? min_slope : t))        (a NaN t stays NaN)
 *   spi = a * t
 * acc (uint32, hdem_flowacc_u8's raster) and d8 (uint8 ESRI codes) are optional inputs: twi and
 * spi need acc, d8_slope and HDEM_TERRAIN_TWI_D8 need d8.  Every output pointer may be NULL (not
 * wanted: no store, no math-library call), at least one must not be.
 * HDEM_ERR_BAD_ARG before any launch: no output, twi / spi without acc, d8_slope or the flag
 * without d8, unknown flags, dx, dy, z_factor or min_slope not finite and > 0, an output that
 * overlaps an input or another output.  HDEM_ERR_BAD_ARG after the launch when d8 was read and
 * holds a byte that is no D8 code (stats.invalid_codes says in how many cells); the outputs
 * are unspecified then.
 * dzdx, dzdy, d8_slope and tangent (sqrtf is correctly rounded) are the same bits from run to
 * run and equal to the formulas above evaluated in IEEE float32; degrees, aspect and twi carry
 * the error of the device math library's atanf, atan2f and logf.  A subset of the outputs
 * holds the bytes the call for all of them writes.
 * No workspace but 32 bytes of counters from the context's arena.  The _dev form synchronises
 * the context's stream once to read them.  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_terrain_stats) first (40 bytes in this version; a shorter
 * struct is filled as far as it goes).  ms_total is filled only while profiling is on
 * (hdem_profile_enable); the call has no kernel id. */
#define HDEM_TERRAIN_TWI_D8 1    /* twi and spi take d8_slope as their t */
typedef struct hdem_terrain_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_terrain_stats), set by the caller             */
    float ms_total;          /* the launch (HIP events; profiling)                            */
    int64_t nan_cells;       /* cells whose dem is NaN                                        */
    int64_t flat_cells;      /* cells with dzdx == 0 && dzdy == 0 (aspect -1)                 */
    int64_t floored_cells;   /* cells whose t was below min_slope (counted when twi is wanted) */
    int64_t invalid_codes;   /* cells whose d8 byte is no D8 code: refused                    */
} hdem_terrain_stats;        /* sizeof == 40 */
int hdem_terrain_f32(hdem_ctx *ctx, const float *dem, int H, int W, const uint32_t *acc,
                     const uint8_t *d8, double dx, double dy, double z_factor, double min_slope,
                     float *dzdx, float *dzdy, float *tangent, float *degrees, float *aspect,
                     float *d8_slope, float *twi, float *spi, int flags,
                     hdem_terrain_stats *stats);        /* host pointers, synchronous */
int hdem_terrain_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W, const uint32_t *acc,
                         const uint8_t *d8, double dx, double dy, double z_factor,
                         double min_slope, float *dzdx, float *dzdy, float *tangent,
                         float *degrees, float *aspect, float *d8_slope, float *twi, float *spi,
                         int flags, hdem_terrain_stats *stats);    /* device pointers */

/* ---- A15  Proximity.apply  (new operator: Euclidean distance, allocation, stream burning) ----
 * The exact Euclidean distance transform of a source set S in the plane of the raster, and what
 * is built on the nearest source: where the D8 operators answer "where does the water of this
 * cell go", this one answers "which source is this cell next to, and how far away is it".
 * sources, source_kind, threshold: the set S, given as A7 gives its stream set, plus one kind:
 *   HDEM_FT_STREAMS_MASK_U8      sources is uint8 H x W, non-zero = in S; threshold 0
 *   HDEM_FT_STREAMS_ACC_U32      sources is uint32 H x W, in S where >= threshold; threshold >= 1
 *   HDEM_PX_SOURCES_LABELS_U32   sources is uint32 H x W, non-zero = in S (and the cell's label);
 *                                threshold 0
 * "Every cell" (HDEM_FT_STREAMS_NONE) is not a kind here.
 * For a cell c = (r, x), n(c) is the source (r', x') that minimises
 *   d2 = (r - r')^2 + (x - x')^2,
 * and AMONG SOURCES AT EQUAL d2 THE ONE WITH THE SMALLEST FLAT INDEX r' * W + x': the tie rule
 * is part of the contract.  Integers decide n(c); no float comparison does.
 * max_distance (cells; 0: none): a cell with d2 > max_distance^2 is out of reach, and so is
 * every cell when S is empty.  The search is not bounded by it.
 * Outputs, all H x W, each may be NULL, at least one must not be:
 *   d2       uint32  the squared distance in cells, exact               0xFFFFFFFF out of reach
 *   nearest  uint32  the flat index of n(c)                             0xFFFFFFFF
 *   label    uint32  sources[n(c)]; HDEM_PX_SOURCES_LABELS_U32 only     0
 *   distance float32 (float)(sqrt((double)d2) * cellsize); square cells NaN
 *   rise     float32 dem[c] - dem[n(c)], one float32 subtraction: the   NaN
 *                    Euclidean counterpart of HAND; needs dem
 *   burned   float32 the dem lowered towards S inside a buffer (AGREE); dem[c]
 *                    needs dem
 * burned, with bf = (float)buffer, sm = (float)smooth, sh = (float)sharp and
 * inv = (float)(1.0 / buffer), in float32, one rounding per operation, no fused multiply-add:
 *   d = (float)sqrt((double)d2)        t = 1 - d * inv
 *   burned = (dem - sm * t) - (d2 == 0 ? sh : 0)   where d < bf,   burned = dem elsewhere.
 * NaN in dem passes through rise and burned by arithmetic.
 * HDEM_ERR_BAD_ARG before any allocation or launch: H * W > 2^32 - 1; (H-1)^2 + (W-1)^2 >
 * 2^32 - 2 (d2 would not fit beside its sentinel); H or W > 65535 (the row pass keeps a column
 * index in 16 bits beside its sentinel, so (1, 65536), which the second bound alone would admit,
 * is refused like (1, 65537); 32768 x 32768 passes); an unknown kind, a threshold that does not
 * go with the kind; no output; label without label sources; rise or burned without dem;
 * cellsize not finite and > 0 when distance is wanted; buffer not finite and > 0 or smooth or
 * sharp not finite and >= 0 when burned is wanted; an output that overlaps an input or another
 * output.
 * Every output is the same bytes from run to run, whatever the schedule; a subset of the outputs
 * holds the bytes the call for all of them writes.
 * Workspace from the context's arena: 4 bytes per cell (the nearest source column of every
 * cell in its row and the nearest row of every cell in its column, both uint16 and both kept
 * column-major) plus 12 bytes per 64 cells (source bits and row carries) and 16 bytes of
 * counters.  The _dev form synchronises the context's stream once, to read the counters.
 * stats may be NULL; otherwise the caller sets stats->struct_size =
 * sizeof(hdem_proximity_stats) first (32 bytes in this version; a shorter struct is filled as
 * far as it goes).  The ms_* fields are filled only while profiling is on
 * (hdem_profile_enable); the call has no kernel id. */
#define HDEM_PX_SOURCES_LABELS_U32 3    /* beside HDEM_FT_STREAMS_MASK_U8 and _ACC_U32 */
typedef struct hdem_proximity_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_proximity_stats), set by the caller         */
    float ms_row;            /* source bits, row carries, row pass (HIP events; profiling)  */
    float ms_column;         /* the column pass                                             */
    float ms_final;          /* the launch that writes the outputs                          */
    int64_t sources;         /* cells of S                                                  */
    int64_t unreached;       /* cells out of reach                                          */
} hdem_proximity_stats;      /* sizeof == 32 */
int hdem_proximity(hdem_ctx *ctx, const void *sources, int source_kind, uint32_t threshold,
                   int H, int W, const float *dem, double cellsize, uint32_t max_distance,
                   double buffer, double smooth, double sharp, uint32_t *d2, uint32_t *nearest,
                   uint32_t *label, float *distance, float *rise, float *burned,
                   hdem_proximity_stats *stats);        /* host pointers, synchronous */
int hdem_proximity_dev(hdem_ctx *ctx, const void *sources, int source_kind, uint32_t threshold,
                       int H, int W, const float *dem, double cellsize, uint32_t max_distance,
                       double buffer, double smooth, double sharp, uint32_t *d2,
                       uint32_t *nearest, uint32_t *label, float *distance, float *rise,
                       float *burned, hdem_proximity_stats *stats);    /* device pointers */

/* ---- A16  WeightedFlowAccumulation.apply  (new operator: weighted D8 flow accumulation) ----
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).
 * A donor of c is a neighbour whose code points at c.  For every cell
 *   S[c] = q(w[c]) + sum of S[d] over the donors d of c,
 * the sum of the quantised weights of every cell whose D8 path passes through c, c included.
 * weights is H x W of weight_type:
 *   HDEM_FLOWSUM_U8, HDEM_FLOWSUM_U32   q(w) = w; frac_bits must be 0
 *   HDEM_FLOWSUM_F32                    q(w) = (int64)rint((double)w * 2^frac_bits), frac_bits
 *                                       0 ... 30: the exact double product rounded once, to
 *                                       nearest even (A13's rule); -0.0 counts as 0
 * A NaN weight contributes 0 and is counted in stats->nan_weights.  A negative or infinite
 * weight, and any q(w) > 2^31 - 1, is refused: HDEM_ERR_BAD_ARG with their count, after the
 * call's one synchronisation.  With q < 2^31 and H * W < 2^32 every sum is below 2^63.
 * Outputs, all H x W, each may be NULL (not wanted), at least one must not be; all are written
 * by the last launch from one walk:
 *   sum     int64    S
 *   value   float32  (float)((double)S * 2^-frac_bits), two roundings to nearest even
 *   mask    uint8    1 where S >= threshold, else 0; threshold >= 1 (in units of q) with mask,
 *                    0 without.  Goes as it is wherever HDEM_FT_STREAMS_MASK_U8 is taken.
 * Integer adds only: identical from run to run, whatever the schedule, and between the host
 * and device forms.
 * HDEM_ERR_BAD_ARG before any allocation or launch: H * W > 2^32 - 1; an unknown weight_type;
 * frac_bits out of range or not 0 with integer weights; no output; mask without threshold >= 1
 * or a threshold without mask; an output that overlaps an input or another output.  After the
 * launches, in bounded time: an invalid byte, codes that form a cycle ("N cells never drain"),
 * weights out of range.  On error the contents of the outputs are unspecified.
 * Workspace: 28 B per tile-perimeter slot, about 1.7 B per cell, from the context's arena.
 * The _dev form synchronises the context's stream once to read its counters.  stats may be
 * NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_flowsum_stats) first (48
 * bytes in this version; a shorter struct is filled as far as it goes).  The three phase times
 * are filled only while profiling is on (hdem_profile_enable); the call has no kernel id. */
typedef enum hdem_flowsum_weight_type {   /* numbered as the zonal value types are */
    HDEM_FLOWSUM_F32 = 1,
    HDEM_FLOWSUM_U32 = 2,
    HDEM_FLOWSUM_U8 = 3
} hdem_flowsum_weight_type;
typedef struct hdem_flowsum_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_flowsum_stats), set by the caller            */
    int32_t max_hops;       /* tile crossings of the longest walk over the exit forest      */
    int64_t exits;          /* cells that drain into another tile: nodes of the exit forest */
    int64_t nan_weights;    /* NaN weights: each contributed 0                              */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: weights quantised, in-tile walks, perimeter paths
                               (HIP events; profiling)                                      */
    float ms_forest;        /* phase B: the exit forest                                     */
    float ms_final;         /* phase C: seeded in-tile walks, outputs written               */
    int32_t reserved;       /* 0                                                            */
} hdem_flowsum_stats;       /* sizeof == 48 */
int hdem_flowsum_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *weights,
                    int weight_type, int frac_bits, int64_t threshold, int64_t *sum,
                    float *value, uint8_t *mask,
                    hdem_flowsum_stats *stats);        /* host pointers, synchronous */
int hdem_flowsum_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *weights,
                        int weight_type, int frac_bits, int64_t threshold, int64_t *sum,
                        float *value, uint8_t *mask,
                        hdem_flowsum_stats *stats);    /* device pointers */

/* ---- A17  UpstreamExtreme.apply  (new operator: upstream D8 minimum / maximum) ----
 * d8: uint8 ESRI codes exactly as hdem_flowacc_u8 takes them (0, or a code pointing outside
 * the raster, is terminal; any byte that is not a code is invalid).
 * U(c) is c together with every cell whose D8 path passes through c.  values is H x W of
 * value_type HDEM_UPEXT_F32 or HDEM_UPEXT_U32.  A float32 NaN is absent: it takes no part and
 * is counted in stats->absent.  Floats are ordered by their bits as a sign-magnitude number,
 *   -inf < ... < -0.0 < +0.0 < ... < +inf,
 * uint32 values as they are, and all of those are present.  For every cell
 *   E[c] = best(v[c], E[d] over the donors d of c),
 * the least (HDEM_UPEXT_MIN) or greatest (HDEM_UPEXT_MAX) present value over U(c).  Where
 * several cells of U(c) hold it with the same bits, the one with the smallest flat index is the
 * holder, in both modes.
 * Outputs, both H x W, each may be NULL (not wanted), at least one must not be:
 *   extreme  of the values' type   E[c], the holder's own bits; for float32 the quiet NaN
 *                                  0x7FC00000 where nothing in U(c) is present
 *   where    uint32                the holder's flat index, 0xFFFFFFFF where nothing is present
 *                                  (H * W <= 2^32 - 1 keeps that value free)
 * One reduction over a 64-bit word per cell, key << 32 | index under unsigned min or
 * key << 32 | ~index under unsigned max: idempotent, commutative and associative on a total
 * order, so the result is identical from run to run, whatever the schedule, and between the
 * host and device forms.
 * HDEM_ERR_BAD_ARG before any allocation or launch: H * W > 2^32 - 1; an unknown value_type or
 * mode; null values; no output; an output that overlaps an input or the other output.  After
 * the launches, in bounded time: an invalid byte, codes that form a cycle ("N cells never
 * drain").  On error the contents of the outputs are unspecified; the context stays usable.
 * Workspace: 28 B per tile-perimeter slot, about 1.7 B per cell, from the context's arena.
 * The _dev form synchronises the context's stream once to read its counters.  stats may be
 * NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_upextreme_stats) first (48
 * bytes in this version; a shorter struct is filled as far as it goes).  The three phase times
 * are filled only while profiling is on (hdem_profile_enable); the call has no kernel id. */
typedef enum hdem_upext_value_type {   /* numbered as the flowsum weight types are */
    HDEM_UPEXT_F32 = 1,
    HDEM_UPEXT_U32 = 2
} hdem_upext_value_type;
typedef enum hdem_upext_mode {
    HDEM_UPEXT_MIN = 0,
    HDEM_UPEXT_MAX = 1
} hdem_upext_mode;
typedef struct hdem_upextreme_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_upextreme_stats), set by the caller          */
    int32_t max_hops;       /* tile crossings of the longest walk over the exit forest      */
    int64_t exits;          /* cells that drain into another tile: nodes of the exit forest */
    int64_t absent;         /* NaN values: they took no part                                */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: values read, in-tile walks, perimeter paths
                               (HIP events; profiling)                                      */
    float ms_forest;        /* phase B: the exit forest                                     */
    float ms_final;         /* phase C: seeded in-tile walks, outputs written               */
    int32_t reserved;       /* 0                                                            */
} hdem_upextreme_stats;     /* sizeof == 48 */
int hdem_upextreme_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *values,
                      int value_type, int mode, void *extreme, uint32_t *where,
                      hdem_upextreme_stats *stats);        /* host pointers, synchronous */
int hdem_upextreme_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *values,
                          int value_type, int mode, void *extreme, uint32_t *where,
                          hdem_upextreme_stats *stats);    /* device pointers */

/* ---- A18  BreachDepressions.apply  (new operator: depression breaching, "carving") ----
 * dem: float32, H x W.  d8: a forest over it, any valid acyclic codes as A17 takes them.
 * A pit is a non-NaN cell that is not on the raster's one-cell ring, has no NaN 8-neighbour
 * and no 8-neighbour whose elevation is strictly lower (float <).  Cells on the ring and cells
 * next to nodata are the fill's outlets and never pits.
 *   t[c]       A17 in min mode over (pit ? dem : absent): the lowest pit upstream of c
 *   carved[c]  t[c] where it is present and t[c] < dem[c] (float <), else dem[c] bit for bit,
 *              NaN payloads included
 *   source[c]  uint32, optional (NULL): the flat index of the pit whose level c was lowered
 *              to, 0xFFFFFFFF where c is unchanged
 * A trench is cut at the pit's level from each pit down its D8 path to where the terrain is
 * lower again; the rest of the depression stays.  An outlet on the ring that a trench reaches
 * is lowered like any other cell.
 * Guarantee: when d8 are the A12 (ResolveFlats) codes of the eps = 0 fill of the same DEM,
 * carved has no sinks (its eps = 0 fill is itself) and carving it again changes nothing.  A
 * local minimum c of carved that is no outlet has no lower neighbour in dem either (carved <=
 * dem), so it is a pit, t[c] <= dem[c] and carved[c] = t[c]; for its receiver r, U(r) contains
 * U(c), so carved[r] <= t[r] <= t[c]: every cell has a non-ascending path to an outlet.  The
 * forest of a sink-free DEM never ascends, so no upstream pit is lower than the cell.
 * The launches are A17's after one radius-1 stencil launch that writes the seeds; the last
 * launch writes carved and source.  Errors as A17 (dem and carved must not be NULL), and carved
 * or source overlapping dem, d8 or each other.
 * Workspace: A17's plus the seed raster, 4 B per cell, from the context's arena.
 * stats as A17's with the pit count and the cells lowered; absent counts the cells that are
 * not pits.  sizeof(hdem_breach_stats) is 64 in this version. */
typedef struct hdem_breach_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_breach_stats), set by the caller             */
    int32_t max_hops;
    int64_t exits;
    int64_t absent;         /* cells that are not pits                                      */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A, the pit stencil included                            */
    float ms_forest;
    float ms_final;
    int32_t reserved;       /* 0                                                            */
    int64_t pits;           /* pits                                                         */
    int64_t lowered;        /* cells of carved below dem                                    */
} hdem_breach_stats;        /* sizeof == 64 */
int hdem_breach_f32(hdem_ctx *ctx, const float *dem, const uint8_t *d8, int H, int W,
                    float *carved, uint32_t *source,
                    hdem_breach_stats *stats);        /* host pointers, synchronous */
int hdem_breach_f32_dev(hdem_ctx *ctx, const float *dem, const uint8_t *d8, int H, int W,
                        float *carved, uint32_t *source,
                        hdem_breach_stats *stats);    /* device pointers */

/* ---- A19  FlowPathSum.apply / FlowPathExtreme.apply  (new operators: downstream D8 path
 *           sums and extremes) ----
 * d8, streams, stream_kind and threshold exactly as hdem_flowtrace_u8 (A7) takes them, and a
 * stop, a dry terminal cell and an unreached cell are what they are there.  Write the D8 path
 * of c as p_0 = c -> p_1 -> ... -> p_k = s(c), its first stop (for an unreached cell: the dry
 * terminal cell it ends in).
 * mode HDEM_FLOWPATH_SUM:  S(c) = sum over i < k of q(p_i), the quantised cost of the step that
 *   leaves each cell of the path; a stop has S = 0.  values are the weights, H x W of
 *   value_type; q is an integer made once per cell:
 *     per HDEM_FLOWPATH_PER_STEP    HDEM_FLOWPATH_U8, _U32: q = w, frac_bits must be 0
 *                                   HDEM_FLOWPATH_F32: q = (int64)rint((double)w * 2^frac_bits),
 *                                   A16's rule.  values must not be NULL, step_len must be.
 *     per HDEM_FLOWPATH_PER_LENGTH  q = (int64)rint(((double)w * len) * 2^frac_bits): one
 *                                   rounding in the product, an exact scaling, one rint to
 *                                   nearest even.  len is the length of the step leaving the
 *                                   cell, read from step_len, 3 * H doubles: for the leaving
 *                                   cell's row y, step_len[3 * y + 0 ... 2] = {east-west,
 *                                   north-south, diagonal}.  Integer weights take any
 *                                   frac_bits.  values may be NULL with HDEM_FLOWPATH_NONE:
 *                                   w = 1, the flow length on an anisotropic grid.  A cell
 *                                   without a direction (code 0, an invalid byte) has q = 0.
 *   frac_bits is 0 ... 30.  -0.0 counts as 0.  A NaN weight costs 0 and is counted in
 *   stats->nan_weights.  A negative or infinite weight and any q > 2^31 - 1, in any cell of the
 *   raster (stops too, so that the refusal does not depend on the streams), is refused:
 *   HDEM_ERR_BAD_ARG with their count, after the call's one synchronisation.  With q < 2^31
 *   and H * W < 2^32 every sum is below 2^63.
 *   step_len is a host pointer in both forms; the call copies it.  An entry that is not finite
 *   and positive is HDEM_ERR_BAD_ARG, with their count, before any launch.
 * mode HDEM_FLOWPATH_MIN, HDEM_FLOWPATH_MAX:  the least / greatest present value over
 *   {p_0, ..., p_k}, c and the stop included.  values is H x W of HDEM_FLOWPATH_F32 or _U32 and
 *   A17's contract holds: a float32 NaN is absent and counted in stats->absent, floats are
 *   ordered by their bits as a sign-magnitude number (-0.0 below +0.0), among equal bits the
 *   smallest flat index is the holder in both modes.  per and frac_bits must be 0, step_len
 *   NULL.
 * Outputs, all H x W, each may be NULL (not wanted), at least one must not be, and an output
 * of the other mode must be NULL:
 *   stop     uint32   1 + flat index of s(c); 0 for an unreached cell, as A7 writes it
 *   sum      int64    SUM: S(c); for an unreached cell the sum to the dry terminal cell
 *   value    float32  SUM: (float)((double)S * 2^-frac_bits), two roundings to nearest even;
 *                     NaN where unreached
 *   extreme  of the values' type   MIN / MAX: the holder's own bits; for float32 the quiet NaN
 *                     0x7FC00000 where nothing on the path is present.  For an unreached cell
 *                     the path to the dry terminal cell is reduced: stop = 0 says so.
 *   where    uint32   MIN / MAX: the holder's flat index, 0xFFFFFFFF where nothing is present
 * Integer adds and min / max on a total order only: identical from run to run and between the
 * host and device forms.
 * HDEM_ERR_BAD_ARG before any allocation or launch: H * W > 2^32 - 1; an unknown mode, per,
 * value_type, stream_kind or non-zero flags; an operand that the mode misses or does not take
 * (as above); frac_bits out of range; no output; an output that overlaps an input or another
 * output; a bad step_len entry.  After the launches, in bounded time: an invalid byte, weights
 * out of range, codes that form a cycle ("N cells never resolve"; a loop that holds a stream
 * cell ends there and is legal).  On error the contents of the outputs are unspecified; the
 * context stays usable.
 * Three phases as A7: A per 64 x 64 tile, B the forest of perimeter slots, C one streaming
 * launch that writes every wanted output.
 * Workspace: 8 B per cell, 32 B per tile-perimeter slot (2.0 B per cell) and 24 B per row for
 * the table, about 10.0 B per cell, from the context's arena.  The _dev form synchronises the
 * context's stream once to read its counters.  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_flowpath_stats) first (72 bytes in this version; a shorter
 * struct is filled as far as it goes).  The three phase times are filled only while profiling
 * is on (hdem_profile_enable); the call has no kernel id. */
typedef enum hdem_flowpath_mode {
    HDEM_FLOWPATH_SUM = 0,
    HDEM_FLOWPATH_MIN = 1,
    HDEM_FLOWPATH_MAX = 2
} hdem_flowpath_mode;
typedef enum hdem_flowpath_per {
    HDEM_FLOWPATH_PER_STEP = 0,
    HDEM_FLOWPATH_PER_LENGTH = 1
} hdem_flowpath_per;
typedef enum hdem_flowpath_value_type {   /* numbered as the flowsum weight types are */
    HDEM_FLOWPATH_NONE = 0,
    HDEM_FLOWPATH_F32 = 1,
    HDEM_FLOWPATH_U32 = 2,
    HDEM_FLOWPATH_U8 = 3
} hdem_flowpath_value_type;
typedef struct hdem_flowpath_stats {
    uint32_t struct_size;   /* in: sizeof(hdem_flowpath_stats), set by the caller           */
    int32_t forest_rounds;  /* pointer-jumping launches of phase B that had work to do      */
    int64_t stops;          /* stop cells: stream cells and terminal cells                  */
    int64_t unreached;      /* cells whose path ends in a terminal cell that is no stream   */
    int64_t exits;          /* cells that are no stop and drain into another tile           */
    int64_t nan_weights;    /* SUM: NaN weights, each cost 0                                */
    int64_t absent;         /* MIN / MAX: NaN values, they took no part                     */
    int32_t tile_h, tile_w;
    float ms_tile;          /* phase A: costs made, in-tile pointer doubling (HIP events;
                               profiling)                                                   */
    float ms_forest;        /* phase B: the forest of perimeter slots                       */
    float ms_final;         /* phase C: outputs written                                     */
    int32_t reserved;       /* 0                                                            */
} hdem_flowpath_stats;      /* sizeof == 72 */
int hdem_flowpath_u8(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                     int stream_kind, uint32_t threshold, int mode, const void *values,
                     int value_type, int per, int frac_bits, const double *step_len,
                     uint32_t *stop, int64_t *sum, float *value, void *extreme,
                     uint32_t *where, int flags,
                     hdem_flowpath_stats *stats);      /* host pointers, synchronous */
int hdem_flowpath_u8_dev(hdem_ctx *ctx, const uint8_t *d8, int H, int W, const void *streams,
                         int stream_kind, uint32_t threshold, int mode, const void *values,
                         int value_type, int per, int frac_bits, const double *step_len,
                         uint32_t *stop, int64_t *sum, float *value, void *extreme,
                         uint32_t *where, int flags,
                         hdem_flowpath_stats *stats);  /* device pointers; step_len host */

/* ---- A20  DInfFlowDirection.apply  (new operator: Tarboton's D-infinity flow direction) ----
 * The D-infinity word, one uint32 per cell, is what A20 writes and A21 reads:
 *   bits 0-15   q, 0 ... 32768: the share of the cell's outflow that goes to the DIAGONAL
 *               receiver, in units of 2^-15
 *   bits 16-19  facet, 0 ... 8; every other bit is 0
 * facet 0: no outflow, and then q = 0.  Facets 1 ... 8 (Tarboton 1997) as (cardinal neighbour e1,
 * diagonal neighbour e2, ac, af), north = row - 1:
 *   1 (E, NE, 0, +1)   2 (N, NE, 1, -1)   3 (N, NW, 1, +1)   4 (W, NW, 2, -1)
 *   5 (W, SW, 2, +1)   6 (S, SW, 3, -1)   7 (S, SE, 3, +1)   8 (E, SE, 4, -1)
 * q = 0 sends everything to e1, q = 32768 everything to e2, anything else to both; a receiver
 * whose share is 0 is no receiver.
 *
 * dem: float32 H x W, NaN is nodata.  All arithmetic is float64 on the float32 elevations, one
 * rounding per operation, no fused multiply-add.  For an interior cell with a non-NaN centre e0,
 * each facet k = 1 ... 8 in order whose e1 and e2 are both non-NaN gives, with d1 the spacing
 * towards e1 (dx for E / W, dy for N / S) and d2 the other one:
 *   s1 = (e0 - e1) / d1                    s2 = (e1 - e2) / d2
 *   s2 <= 0:              s = s1,                             q = 0
 *   s2 * d1 >= s1 * d2:   s = (e0 - e2) / sqrt(d1^2 + d2^2),  q = 32768
 *   otherwise:            s = sqrt(s1^2 + s2^2), r = atan2(s2, s1),
 *                         q = rint(r / atan2(d2, d1) * 32768)
 * The first facet with the strictly greatest s > 0 wins; atan2(s2, s1) is evaluated once, for the
 * winner (atan2(d2, d1) is worked out by the host).  Cells on the raster ring, NaN centres and
 * cells where no facet has a positive slope get word 0.
 * fallback (optional, uint8 ESRI D8 codes, H x W): a cell that would get word 0 and whose code is
 * not 0 takes that direction as a canonical word: E -> facet 1, N -> 2, W -> 4, S -> 6 with q = 0;
 * NE -> facet 1, NW -> 3, SW -> 5, SE -> 7 with q = 32768.  With the A8 (ResolveFlats) codes of an
 * eps = 0 fill the flats keep draining and the combined graph stays acyclic: elevation, then flat
 * distance, decreases along every edge.
 * Optional float32 outputs (NULL: no store):
 *   angle   af * r + ac * pi / 2, radians counter-clockwise from east, with r = 0 and
 *           r = atan2(d2, d1) in the first two cases; a result >= 2 pi reads 0; -1 where the word
 *           is 0; the D8 direction's multiple of pi / 4 in a fallback cell
 *   slope   (float)s of the winner; 0 where none won, NaN at a NaN centre
 * One radius-1 stencil launch on the tile staging of A14.  words and slope are the same bits
 * from run to run and equal to the formulas above in IEEE float64 up to the device library's
 * atan2, which reaches q only through a quotient rounded to 15 bits.
 * HDEM_ERR_BAD_ARG before the launch: a null dem or words, dx or dy not finite and > 0, unknown
 * flags; after it: a fallback byte that is no D8 code.  No workspace but 32 bytes of counters.
 * The _dev form synchronises the context's stream once to read them.  stats may be NULL;
 * otherwise the caller sets stats->struct_size first; ms_total is filled while profiling is on. */
typedef struct hdem_dinf_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_dinf_stats), set by the caller               */
    float ms_total;          /* the launch (HIP events; profiling)                           */
    int64_t no_flow;         /* cells whose word is 0                                        */
    int64_t fallback_cells;  /* cells that took their direction from fallback                */
} hdem_dinf_stats;           /* sizeof == 24 */
int hdem_dinf_f32(hdem_ctx *ctx, const float *dem, int H, int W, const uint8_t *fallback,
                  double dx, double dy, uint32_t *words, float *angle, float *slope, int flags,
                  hdem_dinf_stats *stats);             /* host pointers, synchronous */
int hdem_dinf_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W, const uint8_t *fallback,
                      double dx, double dy, uint32_t *words, float *angle, float *slope,
                      int flags, hdem_dinf_stats *stats);         /* device pointers */

/* ---- A21  DInfFlowAccumulation.apply  (new operator: D-infinity flow accumulation) ----
 * words: uint32 H x W, the D-infinity words of A20.  A donor of a cell c is an 8-neighbour whose
 * word names c with a non-zero share.  With U = 2^frac_bits, frac_bits 0 ... 16:
 *   A[c] = U + sum over the donors d of c of share(d -> c)
 *   to_diag(d) = (A[d] * q[d]) >> 15   (uint64)        to_card(d) = A[d] - to_diag(d)
 * Integer adds only: every cell's outflow is conserved to the last unit, the sum of A over the
 * cells with facet 0 is H * W * U exactly, and the result is the same from run to run and in
 * whichever order the cells are taken.  H * W <= 2^32 - 1 keeps A < 2^48 and the product
 * below 2^63.
 *   sum     int64, A
 *   value   float32, (float)((double)A * 2^-frac_bits): the area in cells
 * At least one of the two is wanted.
 * Accumulation over a DAG, in the structure of A8: classify (words validated, the working raster
 * initialised, every tile listed), then rounds of tile visits -- a 64 x 64 tile and its one-cell
 * halo in LDS, a cell whose donors are all final becomes final with its sum, until the tile
 * stops changing; a tile runs again when one of its eight neighbours finalised a frame cell in
 * the round before -- and a streaming pass that writes the outputs.  The host reads one word per
 * round.  The working raster is one uint64 per cell (bit 63: final): the caller's sum, or 8 B per
 * cell of the context's arena, beside 16 B per tile.
 * HDEM_ERR_BAD_ARG before any launch: a null words, neither output, frac_bits outside 0 ... 16,
 * unknown flags, more than 2^32 - 1 cells; after classify, with the count in the text: an
 * invalid word (facet > 8, q > 32768, facet 0 with q != 0, stray bits), a receiver outside the
 * raster; after the last round: words that form a cycle ("N cells never resolve"; only
 * user-supplied words can).  The outputs are unspecified then.
 * rounds and tile_visits depend on the schedule; every other count does not. */
typedef struct hdem_dinfacc_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_dinfacc_stats), set by the caller            */
    int32_t rounds;          /* rounds of tile visits that had work                          */
    int64_t tile_visits;     /* workgroups launched over all rounds                          */
    int64_t split_cells;     /* cells with two receivers (0 < q < 32768)                     */
    int64_t terminal_cells;  /* cells with facet 0                                           */
    int64_t invalid;         /* invalid words: refused                                       */
    int64_t outside;         /* cells with a receiver outside the raster: refused            */
    int64_t unresolved;      /* cells that never became final (a cycle): refused             */
    int32_t tile_h, tile_w;
    float ms_classify;       /* (HIP events; profiling)                                      */
    float ms_relax;          /* all rounds, the host reads included                          */
    float ms_final;
    int32_t reserved;        /* 0                                                            */
} hdem_dinfacc_stats;        /* sizeof == 80 */
int hdem_dinfacc_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W, int frac_bits,
                     int64_t *sum, float *value, int flags,
                     hdem_dinfacc_stats *stats);       /* host pointers, synchronous */
int hdem_dinfacc_u32_dev(hdem_ctx *ctx, const uint32_t *words, int H, int W, int frac_bits,
                         int64_t *sum, float *value, int flags,
                         hdem_dinfacc_stats *stats);   /* device pointers */

/* ---- A22  WeightedDInfFlowAccumulation.apply  (new operator: weighted D-infinity accumulation) ----
 * words: uint32 H x W, the D-infinity words of A20, validated exactly as A21 validates them (the
 * same refusals, the same counts).  weights is H x W of weight_type (hdem_flowsum_weight_type):
 *   HDEM_FLOWSUM_F32                    q(w) = (int64)rint((double)w * 2^frac_bits), frac_bits
 *                                       0 ... 30: the exact double product rounded once, to
 *                                       nearest even (A13's rule); -0.0 counts as 0
 *   HDEM_FLOWSUM_U8, HDEM_FLOWSUM_U32   q(w) = w << frac_bits, frac_bits 0 ... 16.  A deliberate
 *                                       difference from A16, which takes integer weights at
 *                                       frac_bits 0 only: a D-infinity cell splits its load, so
 *                                       an integer load still needs resolution below one unit.
 * A NaN weight contributes 0 and is counted in stats->nan_weights.  A negative or infinite
 * weight, and any q(w) > 2^31 - 1, is refused with their count (stats->bad_weights).
 * total = sum of q(w) over the raster is summed exactly in uint64 while the words are classified
 * (fewer than 2^32 cells, each below 2^31: no overflow) and total >= 2^48 is refused with the
 * total in the text.  That is what keeps the share product below 2^63: a cell's A is a sum of
 * parts of distinct cells' q, so A <= total < 2^48, and q of a word is <= 2^15.  total is also the
 * conservation check: the sum of A over the cells with facet 0 equals it.
 *   A[c] = q(w[c]) + sum over the donors d of c of share(d -> c)
 *   to_diag(d) = (A[d] * q[d]) >> 15   (uint64)        to_card(d) = A[d] - to_diag(d)
 * as in A21.  Integer adds only: identical from run to run, whatever the schedule, and between
 * the host and device forms.  With uint8 weights of 1 the result is A21's at the same frac_bits.
 *   sum     int64, A
 *   value   float32, (float)((double)A * 2^-frac_bits)
 * At least one of the two is wanted.  sum may serve as the working raster, as in A21: the
 * kernels are A21's, instantiated with the cell's own term read from its working word (classify
 * writes q(w) there, bit 63 clear) instead of the constant U.
 * HDEM_ERR_BAD_ARG before any launch: a null words or weights, neither output, an unknown
 * weight_type, frac_bits out of range for the type, unknown flags, more than 2^32 - 1 cells, an
 * output that overlaps words, weights or the other output.  After classify, in one read of the
 * counters and in this order: invalid words, receivers outside the raster, weights out of range,
 * a total of 2^48 or more.  After the last round: words that form a cycle.  The outputs are
 * unspecified then.
 * Workspace and synchronisation as A21.  stats may be NULL; otherwise the caller sets
 * stats->struct_size = sizeof(hdem_dinfsum_stats) first (104 bytes in this version; a shorter
 * struct is filled as far as it goes).  The struct opens with the fields of hdem_dinfacc_stats.
 * rounds and tile_visits depend on the schedule; every other count does not. */
typedef struct hdem_dinfsum_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_dinfsum_stats), set by the caller            */
    int32_t rounds;          /* rounds of tile visits that had work                          */
    int64_t tile_visits;     /* workgroups launched over all rounds                          */
    int64_t split_cells;     /* cells with two receivers (0 < q < 32768)                     */
    int64_t terminal_cells;  /* cells with facet 0                                           */
    int64_t invalid;         /* invalid words: refused                                       */
    int64_t outside;         /* cells with a receiver outside the raster: refused            */
    int64_t unresolved;      /* cells that never became final (a cycle): refused             */
    int32_t tile_h, tile_w;
    float ms_classify;       /* (HIP events; profiling)                                      */
    float ms_relax;          /* all rounds, the host reads included                          */
    float ms_final;
    int32_t reserved;        /* 0                                                            */
    int64_t nan_weights;     /* NaN weights: each contributed 0                              */
    int64_t bad_weights;     /* negative, infinite or above 2^31 - 1 once quantised: refused */
    uint64_t total;          /* the sum of q(w) over the raster; >= 2^48: refused            */
} hdem_dinfsum_stats;        /* sizeof == 104 */
int hdem_dinfsum_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W, const void *weights,
                     int weight_type, int frac_bits, int64_t *sum, float *value, int flags,
                     hdem_dinfsum_stats *stats);       /* host pointers, synchronous */
int hdem_dinfsum_u32_dev(hdem_ctx *ctx, const uint32_t *words, int H, int W, const void *weights,
                         int weight_type, int frac_bits, int64_t *sum, float *value, int flags,
                         hdem_dinfsum_stats *stats);   /* device pointers */

/* ---- A23  AreaWetnessIndex.apply  (new operator: A14 on a float32 catchment area) ----
 * A sibling of A14: the same launch, edge rule, order of float32 operations and eight outputs.
 * Two inputs differ.
 * area (float32 H x W, in place of acc): the catchment area in cells, e.g. the value output of
 * A21 or A22.   a = area * (float)sqrt(dx * dy).   A NaN area gives NaN twi and spi.  Zero and
 * negative areas are not refused: they go through the IEEE arithmetic as they are (twi of a
 * zero area is -inf, of a negative one NaN) and are counted in stats->nonpositive_area.  With an
 * integer-valued area below 2^24 the call writes the bytes A14 writes for the uint32 acc of the
 * same values.
 * given_slope (float32 H x W, optional) with HDEM_TERRAIN_TWI_GIVEN: twi and spi take
 * t = given_slope[c] as it is (the slope output of A20; NaN where the dem is NaN, as every
 * output there).  The floor applies as in A14,
 * t < min_slope ? min_slope : t, a NaN t stays NaN, and floored_cells counts.  The flag excludes
 * HDEM_TERRAIN_TWI_D8; the flag without the raster and the raster without the flag are refused.
 * twi and spi need area; d8_slope and HDEM_TERRAIN_TWI_D8 need d8.  Everything else -- refusals,
 * exactness, subsets of outputs, the synchronisation -- is A14's.  stats may be NULL; otherwise
 * the caller sets stats->struct_size = sizeof(hdem_terrain_area_stats) first (48 bytes in this
 * version; a shorter struct is filled as far as it goes). */
#define HDEM_TERRAIN_TWI_GIVEN 2    /* twi and spi take given_slope as their t */
typedef struct hdem_terrain_area_stats {
    uint32_t struct_size;     /* in: sizeof(hdem_terrain_area_stats), set by the caller       */
    float ms_total;           /* the launch (HIP events; profiling)                           */
    int64_t nan_cells;        /* cells whose dem is NaN                                       */
    int64_t flat_cells;       /* cells with dzdx == 0 && dzdy == 0 (aspect -1)                */
    int64_t floored_cells;    /* cells whose t was below min_slope (counted when twi is wanted) */
    int64_t invalid_codes;    /* cells whose d8 byte is no D8 code: refused                   */
    int64_t nonpositive_area; /* cells whose area is <= 0 (counted when twi or spi is wanted) */
} hdem_terrain_area_stats;    /* sizeof == 48 */
int hdem_terrain_area_f32(hdem_ctx *ctx, const float *dem, int H, int W, const float *area,
                          const float *given_slope, const uint8_t *d8, double dx, double dy,
                          double z_factor, double min_slope, float *dzdx, float *dzdy,
                          float *tangent, float *degrees, float *aspect, float *d8_slope,
                          float *twi, float *spi, int flags,
                          hdem_terrain_area_stats *stats);    /* host pointers, synchronous */
int hdem_terrain_area_f32_dev(hdem_ctx *ctx, const float *dem, int H, int W, const float *area,
                              const float *given_slope, const uint8_t *d8, double dx, double dy,
                              double z_factor, double min_slope, float *dzdx, float *dzdy,
                              float *tangent, float *degrees, float *aspect, float *d8_slope,
                              float *twi, float *spi, int flags,
                              hdem_terrain_area_stats *stats);    /* device pointers */

/* ---- A24  MFDFlowDirection.apply  (new operator: multiple-flow-direction flow direction) ----
 * Quinn 1991, Freeman 1991, Holmgren 1994: a cell sends flow to every lower neighbour.
 * The MFD word, one uint64 per cell, is what A24 writes and A25 reads.  Directions are numbered as
 * in A20's kernels, counter-clockwise from east: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW,
 * 6 = S, 7 = SE; north is row - 1.
 *   bit 59      the cell has outflow; if it is 0 the whole word is 0
 *   bits 56-58  m, the direction of the main receiver
 *   bits 0-55   seven 8-bit fields p_1 ... p_7 (p_j in bits 8 (j - 1) ... 8 j - 1): the share, in
 *               units of 2^-8, of the neighbour in direction (m + j) & 7; 0: no flow that way
 *   bits 60-63  0
 * A word is valid when it is 0, or bit 59 is set, bits 60-63 are 0 and p_1 + ... + p_7 <= 255.
 * A cell with amount A sends (A * p_j) >> 8 to each receiver with p_j > 0 and A minus the sum of
 * those to the main receiver: every unit is conserved and the arithmetic is shifts only.  The
 * canonical word of a D8 code is m = its direction with every p_j = 0.  The 8-bit resolution is
 * deliberate -- eight shares have to fit 64 bits -- and a share below 1 / 512 is lost to the main
 * receiver.
 *
 * dem: float32 H x W, NaN is nodata.  All arithmetic is float64 on the float32 elevations, one
 * rounding per operation, no fused multiply-add.  For a cell with a finite elevation z0:
 *   1. for each direction d whose neighbour z_d is inside the raster and not NaN, with
 *      drop = z0 - z_d > 0:  s_d = drop / dist_d, dist_d = dx (E, W), dy (N, S) or
 *      diag = sqrt(dx * dx + dy * dy) (the host computes diag once); s_d = 0 otherwise
 *   2. no s_d > 0: the word is 0 (stats->no_flow), unless fallback (optional, uint8 ESRI D8 codes,
 *      H x W) holds a code other than 0 for the cell: then the code's canonical word
 *      (stats->fallback_cells).  A fallback byte that is no D8 code is counted and refused as in
 *      A20.  A cell whose elevation is NaN or infinite goes this way too.
 *   3. s_max = the greatest s_d;  t_d = 1 where s_d == s_max, else s_d / s_max
 *   4. f_d = c_d * pw(t_d, exponent) with c_d = w_card for even d, w_diag for odd d; pw is skipped
 *      (f_d = c_d * t_d) when exponent == 1.0; f_d = 0 where s_d = 0 or t_d < 2^-64
 *   5. m = the direction of the greatest f_d, the lowest d among equals
 *   6. F = ((((((f_0 + f_1) + f_2) + f_3) + f_4) + f_5) + f_6) + f_7
 *   7. for d != m with f_d > 0:  p = (uint64)floor((256.0 * f_d) / F + 0.5), the field of
 *      j = (d - m) & 7.  f_d <= f_m gives p <= 128, and the non-main shares sum to at most
 *      256 * 7 / 8 + 3.5, so the sum of the fields stays <= 255.  Two equal receivers get 128 each.
 * pw(t, e) is not the math library's pow: two libraries a last-place unit apart would disagree on
 * whole families of symmetric cells, where a quotient lands on a rounding boundary.  It is this
 * sequence of float64 operations (constants written 1.0 / n are the correctly rounded quotients):
 *   (m, k) = frexp(t)                          t = m * 2^k, m in [0.5, 1)
 *   if m < 0.7071067811865476:  m = m * 2.0, k = k - 1
 *   s = (m - 1.0) / (m + 1.0);   s2 = s * s
 *   r = 1.0 / 15.0;   then for n = 13, 11, 9, 7, 5, 3, 1:  r = r * s2 + 1.0 / n
 *   l2 = (double)k + ((2.0 * s) * r) * 1.4426950408889634
 *   y = e * l2;   n = floor(y + 0.5);   u = (y - n) * 0.6931471805599453
 *   p = 1.0;   then for i = 12, 11, ..., 2:  p = 1.0 + (u * p) * (1.0 / i);   p = 1.0 + u * p
 *   pw = ldexp(p, (int)n)
 * pw(1, e) is 1 exactly (s = 0, k = 0, y = 0).  For t in [2^-64, 1] and e in [0.25, 16] the
 * truncation of the two series is below 1e-12 and the rounding of y (|y| <= 1024) below 1e-12:
 * pw is within 1e-9 of the real power with a wide margin, where a share is quantised in steps of
 * 2^-9 of the total.
 * Optional float32 output (NULL: no store):
 *   slope   (float)s_max; 0 where no neighbour lies lower (a fallback cell too, as in A20), NaN
 *           where the dem is NaN.  It is what A23 takes as given_slope.
 * One radius-1 stencil launch on the tile staging of A14.  The words and slope are the same bits
 * from run to run, between the host and device forms, and equal to the formulas above evaluated
 * in IEEE float64.  The combined graph is acyclic for A20's reason: every receiver with a share
 * is strictly lower, and fallback steps (A8) lower the flat distance.
 *
 * One symbol, no _dev twin: the pointers are host pointers by default (staged through device
 * buffers of the context, synchronous) and device pointers when flags has HDEM_ON_DEVICE; both
 * run the same body behind the same checks.  HDEM_ERR_BAD_ARG before the launch: a null context,
 * dem or words, dx or dy not finite and > 0, exponent outside [0.25, 16], w_card or w_diag not
 * finite and > 0, unknown flags; after it: a fallback byte that is no D8 code.  No workspace but
 * 32 bytes of counters; the call synchronises the context's stream once to read them.  stats may
 * be NULL; otherwise the caller sets stats->struct_size first; ms_total is filled while profiling
 * is on. */
#define HDEM_ON_DEVICE 0x40000000    /* A24, A25: the raster pointers are device pointers */
typedef struct hdem_mfd_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_mfd_stats), set by the caller                */
    float ms_total;          /* the launch (HIP events; profiling)                           */
    int64_t no_flow;         /* cells whose word is 0                                        */
    int64_t fallback_cells;  /* cells that took their direction from fallback                */
    int64_t split_cells;     /* cells with more than one receiver                            */
} hdem_mfd_stats;            /* sizeof == 32 */
int hdem_mfd_f32(hdem_ctx *ctx, const float *dem, int H, int W, const uint8_t *fallback, double dx,
                 double dy, double exponent, double w_card, double w_diag, uint64_t *words,
                 float *slope, int flags, hdem_mfd_stats *stats);

/* ---- A25  MFDFlowAccumulation.apply  (new operator: MFD flow accumulation, weighted or not) ----
 * words: uint64 H x W, the MFD words of A24.  A donor of a cell c is an 8-neighbour whose word
 * names c: as its main receiver, or with a share field > 0.
 *   A[c] = own(c) + sum over the donors d of c of what d sends to c      (A24: shifts only)
 * weights NULL (weight_type 0): own = 2^frac_bits, frac_bits 0 ... 16.  Otherwise own = q(w[c])
 * exactly as A22 quantises it: the types, the frac_bits ranges, the NaN rule, the refusals and
 * the total-below-2^48 rule are A22's.  A < 2^48 and a share field <= 255 keep every product
 * below 2^56.  Integer adds only: identical from run to run, whatever the schedule, and between
 * the host and device forms; the sum of A over the cells with word 0 is the total of the own
 * terms.  On canonical words the result is A21's on the canonical D-infinity words of the same
 * codes, and with uint8 weights of 1 it is the unweighted result at the same frac_bits.
 *   sum     int64, A          (may serve as the working raster, as in A21)
 *   value   float32, (float)((double)A * 2^-frac_bits)
 * At least one of the two is wanted.  The scheme is A21's -- classify, rounds of tile visits, a
 * schedule kernel, a streaming final pass, one host read per round -- with the routing of the MFD
 * word; a tile visit holds 16 B per cell of LDS (a uint64 value and a uint64 word).
 * One symbol, as A24: host pointers, or device pointers with HDEM_ON_DEVICE in flags.
 * HDEM_ERR_BAD_ARG before any launch: a null context or words, neither output, a weight type
 * without weights or an unknown one, frac_bits out of range, unknown flags, more than 2^32 - 1
 * cells, an output that overlaps an input or the other output.  After classify, with the count
 * in the text and in this order: invalid words, receivers outside the raster, weights out of
 * range, a total of 2^48 or more.  After the last round: words that form a cycle ("N cells never
 * resolve"; the rounds are bounded by H * W + 1).  The outputs are unspecified then.
 * stats: the struct of A22 (104 bytes; a shorter one is filled as far as it goes); split_cells
 * counts the cells with more than one receiver, terminal_cells those with word 0. */
typedef hdem_dinfsum_stats hdem_mfdacc_stats;
int hdem_mfdacc_u64(hdem_ctx *ctx, const uint64_t *words, int H, int W, const void *weights,
                    int weight_type, int frac_bits, int64_t *sum, float *value, int flags,
                    hdem_mfdacc_stats *stats);

/* ---- A26  DInfDistanceDown.apply  (new operator: D-infinity distance down and HAND) ----
 * TauDEM's dinfdistdown: the distance from every cell down its D-infinity paths to a stop set S,
 * measured horizontally, vertically (the drop: with a stream set, the D-infinity height above the
 * nearest drainage) or along the surface, and combined over the two receivers of a split cell
 * as the average weighted by the flow proportions, the minimum or the maximum.
 * words: uint32 H x W, the D-infinity words of A20, validated exactly as A21 validates them (the
 * same refusals, the same counts, stop cells included).
 * The stop set S is given as hdem_flowtrace_u8 (A7) takes its streams:
 *   stream_kind == HDEM_FT_STREAMS_NONE     streams == NULL, threshold == 0: S is the cells with
 *                                           facet 0 (the distance to the outlet)
 *   stream_kind == HDEM_FT_STREAMS_MASK_U8  streams is uint8 H x W, non-zero = in S; threshold 0
 *   stream_kind == HDEM_FT_STREAMS_ACC_U32  streams is uint32 H x W (a D8 accumulation as A2
 *                                           writes it), in S where >= threshold; threshold >= 1
 * dem: float32 H x W; required for HDEM_DD_VERTICAL and HDEM_DD_SURFACE, NULL for
 * HDEM_DD_HORIZONTAL.  dx, dy: the cell's extent eastwards and northwards, finite and > 0.
 *
 * All arithmetic is float64, one rounding per operation, no fused multiply-add.
 *   c in S:                       D[c] = 0, whatever its word: a cycle that holds a stop cell is
 *                                 cut there, as A7 cuts it
 *   c not in S, facet 0:          D[c] = NaN: its path ends without a stop
 *   otherwise c has the cardinal receiver r1 with share 32768 - q and the diagonal receiver r2
 *   with share q; a receiver whose share is 0 is no receiver.  The step to receiver i costs
 *     HDEM_DD_HORIZONTAL   h_i = dx (E, W), dy (N, S), or diag = sqrt(dx * dx + dy * dy) for the
 *                          diagonal, which the host works out once
 *     HDEM_DD_VERTICAL     v_i = (double)dem[c] - (double)dem[r_i]
 *     HDEM_DD_SURFACE      sqrt(h_i * h_i + v_i * v_i)
 *   and a_i = cost_i + D[r_i].  Then
 *     one receiver:                 D[c] = a_i
 *     two, HDEM_DD_AVERAGE:         D[c] = ((double)(32768 - q) * a1 + (double)q * a2) * 2^-15
 *                                   (two products, their sum, one product, in this order): NaN
 *                                   if either a_i is NaN -- TauDEM's rule, a cell is reported
 *                                   only if every path from it reaches a stop
 *     two, HDEM_DD_MAXIMUM:         NaN if either a_i is NaN, else a2 > a1 ? a2 : a1
 *     two, HDEM_DD_MINIMUM:         a2 if a1 is NaN, a1 if a2 is NaN (NaN if both are), else
 *                                   a2 < a1 ? a2 : a1
 *   distance[c] = (float)D[c].  Every NaN is stored as the one canonical quiet NaN (float64
 *   0x7FF8000000000000 on the way, float32 0x7FC00000 in distance): one NaN bit pattern.
 * A NaN or infinite elevation goes through this arithmetic as it is.  With one receiver
 * everywhere (the canonical words of D8 codes) the three statistics agree bit for bit; the
 * vertical distance is then a telescoping sum of float32 differences.
 *
 * A cell's value is a function of its receivers' final values alone, so the result is the same
 * bits from run to run, whatever the schedule, and between host and device pointers.  The scheme
 * is A21's with the dependency reversed -- classify (words validated, the working raster set to
 * 0, NaN or "not final", every tile listed), rounds of tile visits (a 64 x 64 tile and its halo
 * in LDS; a cell whose receivers are all final becomes final; a tile runs again when one of its
 * eight neighbours finalised a frame cell in the round before), a streaming pass that writes
 * distance.  The host reads one word per round.  The working raster is one uint64 per cell (the
 * bits of D; "not final" is a reserved NaN pattern no result is stored as): 8 B per cell of the
 * context's arena beside 16 B per tile.
 * One symbol, as A24: host pointers (staged through device buffers of the context, synchronous),
 * or device pointers with HDEM_ON_DEVICE in flags.
 * HDEM_ERR_BAD_ARG before any launch: a null context, words or distance, a dem missing (vertical,
 * surface) or surplus (horizontal), an unknown kind, statistic, stream_kind or flag, streams
 * and threshold that do not go with the stream_kind (a threshold without an accumulation among
 * them), dx or dy not finite and > 0, more than 2^32 - 1 cells.  After classify, with the count
 * in the text: an invalid word, a receiver outside the raster.  After the last round: a cycle
 * without a stop cell ("N cells never resolve"; only user-supplied words can form one; the rounds
 * are bounded by H * W + 1).  distance is unspecified then.
 * stats may be NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_dinfdist_stats)
 * first (96 bytes in this version; a shorter struct is filled as far as it goes).  rounds and
 * tile_visits depend on the schedule; every other count does not. */
#define HDEM_DD_HORIZONTAL 0
#define HDEM_DD_VERTICAL 1
#define HDEM_DD_SURFACE 2
#define HDEM_DD_AVERAGE 0
#define HDEM_DD_MINIMUM 1
#define HDEM_DD_MAXIMUM 2
typedef struct hdem_dinfdist_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_dinfdist_stats), set by the caller           */
    int32_t rounds;          /* rounds of tile visits that had work                          */
    int64_t tile_visits;     /* workgroups launched over all rounds                          */
    int64_t split_cells;     /* cells with two receivers (0 < q < 32768)                     */
    int64_t terminal_cells;  /* cells with facet 0                                           */
    int64_t stop_cells;      /* cells of the stop set                                        */
    int64_t unreached_cells; /* cells whose distance is NaN                                  */
    int64_t invalid;         /* invalid words: refused                                       */
    int64_t outside;         /* cells with a receiver outside the raster: refused            */
    int64_t unresolved;      /* cells that never became final (a cycle without a stop): refused */
    int32_t tile_h, tile_w;
    float ms_classify;       /* (HIP events; profiling)                                      */
    float ms_relax;          /* all rounds, the host reads included                          */
    float ms_final;
    int32_t reserved;        /* 0                                                            */
} hdem_dinfdist_stats;       /* sizeof == 96 */
int hdem_dinfdist_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W, const void *streams,
                      int stream_kind, uint32_t threshold, const float *dem, double dx, double dy,
                      int kind, int statistic, float *distance, int flags,
                      hdem_dinfdist_stats *stats);

/* ---- A27  DInfDistanceUp.apply  (new operator: D-infinity distance up to the ridge) ----
 * TauDEM's dinfdistup: the distance from every cell up its D-infinity paths to the ridge,
 * measured horizontally, vertically (the rise) or along the surface, and combined over the cells
 * that drain into it as the average weighted by the entering flow proportions, the minimum or
 * the maximum.  With A26 on the same words: hillslope length, slope position down / (down + up).
 * words: uint32 H x W, the D-infinity words of A20, validated exactly as A21 and A26 validate
 * them (the same refusals, the same counts).
 * dem: float32 H x W; required for HDEM_DD_VERTICAL and HDEM_DD_SURFACE, NULL for
 * HDEM_DD_HORIZONTAL.  dx, dy: the cell's extent eastwards and northwards, finite and > 0.
 * kind and statistic: the HDEM_DD_* of A26.
 *
 * A donor of a cell c is an 8-neighbour d inside the raster whose word names c: as its cardinal
 * receiver, with share p = 32768 - q, or as its diagonal receiver, with share p = q, in units of
 * 2^-15; a share of 0 is no link.  A donor is COUNTED when p >= min_share, min_share an integer
 * in 1 ... 32768: TauDEM's proportion threshold as an exact integer comparison, so that a cell
 * which receives a sliver of dispersed flow is not taken to lie below its neighbour.  A cell
 * without a counted donor is a ridge cell.
 *
 * All arithmetic is float64, one rounding per operation, no fused multiply-add.
 *   c without a counted donor:    D[c] = 0
 *   otherwise the counted donors are taken in the order of their position around c, A20's
 *   direction numbering: 0 = E, counter-clockwise, to 7 = SE.  The step from d down to c costs
 *     HDEM_DD_HORIZONTAL   h = dx (E, W), dy (N, S), or diag = sqrt(dx * dx + dy * dy) for the
 *                          diagonal, which the host works out once
 *     HDEM_DD_VERTICAL     v = (double)dem[d] - (double)dem[c]
 *     HDEM_DD_SURFACE      sqrt(h * h + v * v)
 *   and a_d = cost(d, c) + D[d].  Then
 *     one counted donor:            D[c] = a_d: no product, no quotient
 *     several, HDEM_DD_AVERAGE:     num = the sum, from left to right in that order, of
 *                                   (double)p_d * a_d; den = (double)(the sum of the p_d, in
 *                                   integers); D[c] = num / den.  NaN if any a_d is NaN
 *     several, HDEM_DD_MAXIMUM:     NaN if any a_d is NaN, else the running a > m ? a : m in
 *                                   that order, from m = the first a_d
 *     several, HDEM_DD_MINIMUM:     over the a_d that are not NaN, the running a < m ? a : m in
 *                                   that order, from m = the first of them; NaN if all are NaN
 *   distance[c] = (float)D[c].  Every NaN is stored as the one canonical quiet NaN (float64
 *   0x7FF8000000000000 on the way, float32 0x7FC00000 in distance): one NaN bit pattern.
 * A NaN or infinite elevation goes through this arithmetic as it is.
 * The average weighs each counted donor by the share it sends to c, normalised by the sum of the
 * counted shares that enter c.  This weighting is this project's contract; it is not claimed to
 * reproduce TauDEM's dinfdistup bit for bit.
 *
 * A cell's value is a function of its counted donors' final values alone, and which donors are
 * counted follows from the words and min_share alone, so the result is the same bits from run
 * to run, whatever the schedule, and between host and device pointers.  The scheme is A21's
 * dependency on A26's values -- classify (words validated, links counted, the working raster
 * set to "not final", every tile listed), rounds of tile visits (a 64 x 64 tile and its halo in
 * LDS; each cell's counted donors as a bit mask; a cell without one becomes final with 0, a cell
 * whose counted donors are all final becomes final; a tile runs again when one of its eight
 * neighbours finalised a frame cell in the round before), a streaming pass that writes
 * distance.  The host reads one word per round.  The working raster is one uint64 per cell (the
 * bits of D; "not final" is a reserved NaN pattern no result is stored as): 8 B per cell of the
 * context's arena beside 16 B per tile.
 * One symbol, as A26: host pointers (staged through device buffers of the context, synchronous),
 * or device pointers with HDEM_ON_DEVICE in flags.
 * HDEM_ERR_BAD_ARG before any launch: a null context, words or distance, a dem missing (vertical,
 * surface) or surplus (horizontal), an unknown kind, statistic or flag, min_share outside
 * 1 ... 32768, dx or dy not finite and > 0, more than 2^32 - 1 cells, a distance that overlaps
 * words or dem.  After classify, with the count in the text: an invalid word, a receiver outside
 * the raster.  After the last round: a cycle of counted links, and every cell that waits on one
 * ("N cells never resolve"; only user-supplied words can form one; the rounds are bounded by
 * H * W + 1).  distance is unspecified then.
 * stats may be NULL; otherwise the caller sets stats->struct_size = sizeof(hdem_dinfdistup_stats)
 * first (104 bytes in this version; a shorter struct is filled as far as it goes).  rounds and
 * tile_visits depend on the schedule; every other count does not. */
typedef struct hdem_dinfdistup_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_dinfdistup_stats), set by the caller         */
    int32_t rounds;          /* rounds of tile visits that had work                          */
    int64_t tile_visits;     /* workgroups launched over all rounds                          */
    int64_t ridge_cells;     /* cells without a counted donor: distance 0                    */
    int64_t counted_links;   /* (donor, cell) links with share >= min_share                  */
    int64_t ignored_links;   /* (donor, cell) links with share 1 ... min_share - 1           */
    int64_t merge_cells;     /* cells with more than one counted donor                       */
    int64_t nan_cells;       /* cells whose distance is NaN                                  */
    int64_t invalid;         /* invalid words: refused                                       */
    int64_t outside;         /* cells with a receiver outside the raster: refused            */
    int64_t unresolved;      /* cells that never became final (a cycle of counted links): refused */
    int32_t tile_h, tile_w;
    float ms_classify;       /* (HIP events; profiling)                                      */
    float ms_relax;          /* all rounds, the host reads included                          */
    float ms_final;
    int32_t reserved;        /* 0                                                            */
} hdem_dinfdistup_stats;     /* sizeof == 104 */
int hdem_dinfdistup_u32(hdem_ctx *ctx, const uint32_t *words, int H, int W, const float *dem,
                        double dx, double dy, int kind, int statistic, uint32_t min_share,
                        float *distance, int flags, hdem_dinfdistup_stats *stats);

/* ---- A28  CostDistance.apply / CostAllocation.apply  (new operator: cost distance, back link,
 *           allocation) ----
 * ArcGIS Cost Distance / Cost Back Link / Cost Allocation, Whitebox CostDistance, GRASS r.cost:
 * the least accumulated cost from every cell to a source set when crossing a cell has a price.
 * Everything is integers after one rounding per cell, so the result is the same bytes from run to
 * run, whatever the schedule, and between host and device pointers.
 * cost: float32 H x W, the price per cell length of crossing the cell.
 * sources, source_kind, threshold: the set S exactly as A15 takes it (HDEM_FT_STREAMS_MASK_U8,
 * HDEM_FT_STREAMS_ACC_U32 with threshold >= 1, HDEM_PX_SOURCES_LABELS_U32).
 * frac_bits: 0 ... 16.  cellsize: square cells, finite and > 0.  max_units: >= 0, 0 = no limit.
 *
 * Quantisation (A13's and A16's rule: the exact double product, rounded once to nearest even):
 *   q(c) = (int64)rint((double)cost[c] * 2^frac_bits)
 * A NaN cost is a BARRIER: the cell is not in the graph, even when it is in S.  A negative or
 * infinite cost, q == 0 (a step costs at least 1, so distances strictly decrease along back
 * links) and q > 2^28 - 1 (with H * W < 2^32 every path sum then stays below 2^62) are refused
 * with their count.
 * Graph: the non-barrier cells, 8-connected; a diagonal step needs only its two end cells
 * (cutting the corner of a barrier is legal).  Step weights, symmetric, in units of
 * 2^-(frac_bits+1) cost * cell, with s = q(a) + q(b) <= 2^29:
 *   cardinal   w = s
 *   diagonal   w = (s * 3037000500 + 2^30) >> 31 in uint64: s * sqrt(2) rounded to nearest with
 *              the constant round(sqrt(2) * 2^31)
 * D[c]: the least sum of step weights over all paths from c to a non-barrier cell of S; 0 there;
 * "out of reach" at barriers, at cells with no path, and at cells with D > max_units when a limit
 * is given (the search itself is not bounded by the limit).  D is the unique solution of
 * D[src] = 0, D[c] = min over neighbours n of D[n] + w(c, n).
 * Back link of a reached cell outside S: the ESRI code of the FIRST neighbour n in D8 window
 * order (NW, N, NE, W, E, SW, S, SE) with D[n] + w(c, n) == D[c]; 0 in S and out of reach.  The
 * tie rule is part of the contract.  D strictly decreases along back links: the codes are valid,
 * acyclic A5 / A6 / A7 / A16 / A19 input whose paths end in S.
 * Outputs, all H x W, each may be NULL, at least one must not be:       out of reach
 *   units     int64    D                                                  -1
 *   distance  float32  (float)((double)D * ldexp(cellsize, -(frac_bits+1)))  NaN (0x7FC00000)
 *   backlink  uint8    as above                                           0
 *   nearest   uint32   flat index of the cell of S the back-link path ends in   0xFFFFFFFF
 *   label     uint32   sources[nearest]; HDEM_PX_SOURCES_LABELS_U32 only  0
 * A subset of the outputs holds the bytes the call for all of them writes.
 *
 * The scheme is A8's with weights: classify (costs validated and counted, the working raster
 * uint64 D = 0 in S, 2^64 - 1 elsewhere, the tiles that hold a source listed and, where one lies
 * on the tile's frame, stamped so that the neighbours run in the next round), rounds of tile
 * visits (a 64 x 64 tile and its halo in LDS, four directional sweeps racing through 64-bit LDS
 * atomic min until the tile stops changing; a tile runs again when one of its eight neighbours
 * changed a frame cell in the round before), a streaming pass that writes units, distance and
 * backlink and checks the local equation at every non-barrier cell (HDEM_ERR_NOT_CONVERGED on a
 * violation, or past H * W rounds), and -- only when nearest or label is wanted -- A7's trace
 * (hdem_flowtrace_u8_dev) over the back links with S as its streams.  The host reads one word per
 * round.  Workspace from the context's arena: 8 B per cell and 8 B per tile; with nearest or
 * label A7's 8 B per cell more, 1 B per cell when backlink is not wanted, 4 B per cell when
 * nearest is not.
 * One symbol, as A24 - A27: host pointers (staged through device buffers of the context,
 * synchronous), or device pointers with HDEM_ON_DEVICE in flags; any other flag is refused.
 * HDEM_ERR_BAD_ARG before any allocation or launch: a null context, cost or sources, more than
 * 2^32 - 1 cells, an unknown kind or a threshold that does not go with it, frac_bits outside
 * 0 ... 16, cellsize not finite and > 0 when distance is wanted, max_units < 0, no output, label
 * without label sources, an output that overlaps an input or another output, a stats struct_size
 * of 0.  After the call's first synchronisation: "cost out of range in N cells: ...".
 * stats may be NULL; otherwise the caller sets stats->struct_size =
 * sizeof(hdem_costdistance_stats) first (96 bytes in this version; a shorter struct is filled as
 * far as it goes).  rounds and tile_visits depend on the schedule; every other count does not. */
typedef struct hdem_costdistance_stats {
    uint32_t struct_size;    /* in: sizeof(hdem_costdistance_stats), set by the caller       */
    int32_t rounds;          /* rounds of tile visits that had work                          */
    int64_t tile_visits;     /* workgroups launched over all rounds                          */
    int64_t sources;         /* cells of S that are no barrier                               */
    int64_t barriers;        /* cells whose cost is NaN                                      */
    int64_t unreached;       /* non-barrier cells out of reach                               */
    int64_t tie_cells;       /* reached cells outside S where several neighbours attain D    */
    int64_t invalid;         /* costs out of range: refused                                  */
    int64_t max_units;       /* the largest D of a reached cell                              */
    int32_t tile_h, tile_w;
    float ms_classify;       /* (HIP events; profiling)                                      */
    float ms_relax;          /* all rounds, the host reads included                          */
    float ms_final;
    float ms_trace;          /* 0 when neither nearest nor label is wanted                   */
    int32_t reserved[2];     /* 0                                                            */
} hdem_costdistance_stats;   /* sizeof == 96 */
int hdem_costdistance_f32(hdem_ctx *ctx, const float *cost, int H, int W, const void *sources,
                          int source_kind, uint32_t threshold, int frac_bits, double cellsize,
                          int64_t max_units, int64_t *units, float *distance, uint8_t *backlink,
                          uint32_t *nearest, uint32_t *label, int flags,
                          hdem_costdistance_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* HYDRODEM_HIP_H */
