"""
Elevation regimes for the filter branch: inputs for tests/test_filter_regimes.py (the CPU
references among themselves) and tests/test_gpu_filter_regimes.py (the HIP kernels against
them).  A plain helper module: rasters, cached oracle results and mirrored kernel constants.

The filter kernels -- QuadraticFilter / GrovesCorrection (A3/A4), the box mean and Around
(A5), Convolve -- are the ones whose results depend on floating-point magnitude, and every
other raster they are tested on lies at about 100 m.  The regimes are those of
tests/elevation_regimes.py plus ``steep_x30`` (z * 30: hundreds of metres of relief inside one
strip of the streaming groves kernel).

The bar everywhere: ``1e-6 * max|z|`` over the finite cells that can reach the compared
outputs -- the project's TOL = 1e-4 m at 100 m and its 5e-3 m at 5000 m are the same number.
For a raster with one planted outlier the outlier is left out of the maximum: the compared
cells do not see it.
"""
import functools

import numpy as np

import hdem_synth
import oracle
from oracle import c_oracle
from elevation_regimes import REGIMES, _frozen

# ---------------------------------------------------------------------------
# the kernels' constants, each with the line it mirrors (hdem_groves.hip)
# ---------------------------------------------------------------------------
GTW = 64                    # `constexpr int GTW = 64` (tiled kernel: output tile width)
GTH = 32                    # `constexpr int GTH = 32` (tiled kernel: output tile height)
SW_COLS = 256               # `constexpr int SW_COLS = 256` (streaming kernel: strip width)
STREAM_WS = (3, 9, 15)      # launch_ws `if constexpr (WS == 15 || WS == 9 || WS == 3)`
STRIP_ROWS = (96, 192)      # launch_ws `for (int cand = 96; cand <= 192; ++cand)`
PLACES_PER_CU = 8           # launch_ws `places = ctx->num_cus * (... : 8)`
CUS = (64, 256, 304)        # compute-unit counts the predicate is checked at; the MI355X has 256

THRESHOLD = 1.5             # MaskTallGroves: highlight > 1.5 m


def strip_rows(shape, ws, cus):
    """launch_ws: among the strip heights of 96 ... 192 rows the one whose last round of the
    machine is fullest, ties to the taller (``if (eff >= best)``)."""
    h, w = shape
    sx = -(-w // SW_COLS)
    places = cus * PLACES_PER_CU
    rows, best = 128, -1.0
    for cand in range(STRIP_ROWS[0], STRIP_ROWS[1] + 1):
        strips = sx * -(-h // cand)
        rounds = -(-strips // places)
        eff = float(h) * sx / (float(rounds) * places * (cand + 2 * (ws // 2)))
        if eff >= best:
            best, rows = eff, cand
    return rows


def stream_offset_cells(shape, ws, cus=256):
    """The cells the streaming kernel of the parent commit took its strip offset c0 from:
    ``img[min(y0 + strip_rows / 2, H - 1)][min(x0 + SW_COLS / 2, W - 1)]``, one per strip."""
    h, w = shape
    rows = strip_rows(shape, ws, cus)
    return sorted({(min(y0 + rows // 2, h - 1), min(x0 + SW_COLS // 2, w - 1))
                   for y0 in range(0, h, rows) for x0 in range(0, w, SW_COLS)})


def tiled_offset_cells(shape):
    """The same of the tiled kernel: ``img[min(y0 + GTH / 2, H - 1)][min(x0 + GTW / 2, W - 1)]``,
    one per 64 x 32 tile."""
    h, w = shape
    return sorted({(min(y0 + GTH // 2, h - 1), min(x0 + GTW // 2, w - 1))
                   for y0 in range(0, h, GTH) for x0 in range(0, w, GTW)})


def offset_cells(shape, ws):
    return stream_offset_cells(shape, ws) if ws in STREAM_WS else tiled_offset_cells(shape)


# ---------------------------------------------------------------------------
# regimes and the bar
# ---------------------------------------------------------------------------
FILTER_REGIMES = dict(REGIMES, steep_x30=lambda z: z * np.float32(30.0))
# A3/A4: ``near_max`` overflows the reference's own sums (tests/test_filter_regimes.py asserts
# it) and the ulp ladder is a raster for order, not for magnitude
QUADRATIC_REGIMES = ("below_sea", "zero_cross", "high_8000", "milli", "tiny", "huge_1e30",
                     "steep_x30")
QUADRATIC_SHAPES = ((90, 300), (128, 203))
QUADRATIC_WINDOWS = (15, 9, 7, 21)           # two of the streaming kernel, two of the tiled one
QUIET_REGIMES = ("milli", "tiny")            # no highlight reaches 1.5: groves corrects nothing

OUTLIERS = (-32768.0, 9999.0, 1e30, -1e30)
OUTLIER_CASES = (((90, 300), 15), ((90, 300), 9), ((70, 150), 7), ((70, 150), 21))
LATTICE = 8


def bar(z, without=None):
    """1e-6 * max|z| over the finite cells; ``without``: a boolean raster of cells left out."""
    a = np.abs(np.asarray(z, np.float64))
    keep = np.isfinite(a)
    if without is not None:
        keep &= ~without
    return 1e-6 * float(a[keep].max())


def ulp_of_max(z):
    return float(np.spacing(np.float32(np.abs(z[np.isfinite(z)]).max())))


def groves_delta(z):
    """Half-width of the band round the threshold inside which a groves cell is excused: the
    1e-3 m of tests/test_gpu_parity.py, or 64 ulp of max|z| where that is more."""
    return max(1e-3, 64.0 * ulp_of_max(z))


def far_from(shape, cells, reach):
    """Cells farther than ``reach`` (Chebyshev) from every cell of ``cells``."""
    far = np.ones(shape, bool)
    for y, x in cells:
        far[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1] = False
    return far


def lattice(shape, stride=LATTICE):
    return [(y, x) for y in range(0, shape[0], stride) for x in range(0, shape[1], stride)]


def block_3x4(centre, shape):
    """The 3 x 4 block of cells centred on ``centre`` (hdem_synth.synth_hsheds plants voids of
    this size), clipped to the raster."""
    y, x = centre
    return [(yy, xx) for yy in range(max(y - 1, 0), min(y + 2, shape[0]))
            for xx in range(max(x - 2, 0), min(x + 2, shape[1]))]


# ---------------------------------------------------------------------------
# rasters and their oracle results (computed once, read-only)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dem(name, shape):
    """``synth_dem`` of ``shape`` in the regime ``name`` (``base``: as it is)."""
    z = hdem_synth.synth_dem(*shape)
    if name != "base":
        with np.errstate(over="ignore"):
            z = FILTER_REGIMES[name](z)
    assert z.dtype == np.float32 and z.shape == tuple(shape)
    return _frozen(np.ascontiguousarray(z))


@functools.lru_cache(maxsize=None)
def bumpy(name, shape):
    """The raster of test_groves_matches_reference_restatement (4 % of the cells raised by
    1 ... 6 m) in the regime ``name``, and its groves mask."""
    img = hdem_synth.synth_dem(*shape)
    rng = np.random.default_rng(11)
    img = (img + np.where(rng.random(shape) < 0.04, rng.uniform(1, 6, shape), 0)
           ).astype(np.float32)
    if name != "base":
        img = FILTER_REGIMES[name](img)
    return _frozen(np.ascontiguousarray(img, np.float32), hdem_synth.synth_groves(*shape))


@functools.lru_cache(maxsize=None)
def quadratic_case(name, shape, ws):
    """(raster, quadratic_exact64, the bit-faithful quadratic_ref)."""
    z = dem(name, shape)
    with np.errstate(all="ignore"):
        return _frozen(z, oracle.quadratic_exact64(z, ws), c_oracle.quadratic_ref(z, ws))


@functools.lru_cache(maxsize=None)
def groves_case(name, shape, ws):
    """(image, mask, groves_ref x 3, groves_exact64 x 3, its three highlights, its masks)."""
    img, groves = bumpy(name, shape)
    with np.errstate(all="ignore"):
        want = c_oracle.groves_ref(img, groves, 3, ws)
        exact, stages = oracle.groves_exact64(img, groves, 3, ws)
    return (img, groves) + _frozen(want, exact) + (
        tuple(_frozen(s[0]) for s in stages), tuple(_frozen(s[1]) for s in stages))


def references_decide_differently(name, shape, ws):
    """The cells at which ``groves_ref`` and ``groves_exact64`` correct in different passes --
    the ground truth of a flip between the two references -- and, per cell, the first such
    pass (3 where there is none)."""
    img, groves, _, _, _, masks = groves_case(name, shape, ws)
    _, ref_masks = c_oracle.groves_ref(img, groves, 3, ws, masks=True)
    first = np.full(shape, 3, np.int64)
    for k in (2, 1, 0):
        first[(ref_masks[k] != 0) != (masks[k] != 0)] = k
    return first < 3, first


# The two cases in which the restatement and exact math -- and so a kernel that follows exact
# math and the restatement -- fail the rule of ``groves_compare`` through no cell of their own:
# one band cell is corrected by the one and not by the other in the second pass (its highlight
# is 2 and 4 ulp from 1.5), differs by its highlight of 1.5 m after that pass, and in the third
# pass every output whose window holds it differs by 1.5 m times a kernel weight: up to 3.5e-2
# m, ten times the bar, at cells that are in no band -- and at two that are (window 21).
SURROUNDINGS_OF_A_FLIP = (("steep_x30", (90, 300), 9), ("steep_x30", (90, 300), 21))


def largest_kernel_weight(ws):
    """max |K|, K = a (xx^2 + yy^2) + b: the correlation kernel of the quadratic filter."""
    v, _, (a, b) = oracle.quadratic_constants(ws)
    xx, yy = np.meshgrid(v, v)
    return float(np.abs(a * (xx * xx + yy * yy) + b).max())


def surroundings_of_a_flip(name, shape, ws):
    """The explicit, bounded exception for SURROUNDINGS_OF_A_FLIP, from the two references
    alone: (cells, bound).  ``cells``: the cells other than the flipped one whose window holds
    it in the pass after the flip; ``bound``: there, the flipped cell's highlight at the pass
    of the flip times the largest kernel weight (6.5e-2 m at window 9, 1.3e-2 m at window 21;
    measured between the references: 3.5e-2 and 1.2e-2 m).  None for every other case."""
    if (name, shape, ws) not in SURROUNDINGS_OF_A_FLIP:
        return None
    highlights = groves_case(name, shape, ws)[4]
    differ, first = references_decide_differently(name, shape, ws)
    cells, bound = np.zeros(shape, bool), np.zeros(shape)
    for y, x in np.argwhere(differ):
        assert first[y, x] == 1, "a flip in the first pass reaches two windows: not bounded here"
        near = ~far_from(shape, [(y, x)], ws // 2)
        near[y, x] = False
        cells |= near
        bound[near] = np.maximum(bound[near], abs(float(highlights[1][y, x]))
                                 * largest_kernel_weight(ws))
    return cells, bound


def groves_compare(got, want64, highlight, tol, delta, thr=THRESHOLD, surroundings=None):
    """``_groves_compare`` of tests/test_gpu_parity.py with its two constants as arguments:
    <= tol everywhere except cells whose highlight is within delta of the threshold in some
    iteration; returns (such excused cells, cells of the band).  ``surroundings``: what
    ``surroundings_of_a_flip`` returned -- those cells may be off by their bound instead."""
    err = np.abs(np.asarray(got, np.float64) - want64)
    bad = err > tol
    if surroundings is not None:
        cells, bound = surroundings
        bad &= ~(cells & (err <= bound))
    band = np.zeros_like(bad)
    for hl in highlight:
        band |= np.abs(hl - thr) < delta
    wrong = bad & ~band
    assert not wrong.any(), \
        f"max err {err[wrong].max():.3e} > {tol:.3e} at {int(wrong.sum())} cells"
    return int((bad & band).sum()), int(band.sum())


def excused_limit(img):
    """``_groves_excused_limit`` of tests/test_gpu_parity.py."""
    return max(2, img.size // 20000)


# ---------------------------------------------------------------------------
# box mean, Around, Convolve
# ---------------------------------------------------------------------------
BOX_SHAPES = ((33, 1030), (31, 257))
BOX_REGIMES = tuple(n for n in REGIMES if n != "ulp_ladder") + ("steep_x30",)
BOX_INTEGER = ("below_sea", "zero_cross")    # integer metres: ties at negative values, -0.0


@functools.lru_cache(maxsize=None)
def box_raster(name, shape, dtype, integer=False):
    """The regime raster for the box mean; ``integer``: from the integer-metre variant, so
    that sum / 9 has round-half-even ties and results in (-0.5, 0); float64: with noise
    below float32's resolution, as test_boxmean_matches_oracle has it."""
    z = hdem_synth.synth_dem(*shape, variant="srtm" if integer else "rough")
    if name == "near_max" and float(z.max()) > float(np.finfo(np.float32).max) / 3.0e36:
        # (33 x 1030 reaches 114 m, which times 3.0e36 is past FLT_MAX: the highest cell at 3.3e38)
        z = z * np.float32(3.3e38 / float(z.max()))
        assert np.isfinite(z).all()
    else:
        with np.errstate(over="ignore"):
            z = FILTER_REGIMES[name](z)
    if integer and name == "zero_cross":
        z = z.copy()
        z[3:6, 4:9] = [[-1, -1, -1, 0, 0], [-1, 0, 0, 0, 0], [0, 0, 0, 0, 0]]   # sums -4 ... 0
    x = z.astype(dtype)
    if dtype == np.float64 and not integer:
        x = x * (1.0 + np.random.default_rng(1).standard_normal(shape) * 1e-9)
    return _frozen(np.ascontiguousarray(x))


def halves(x):
    """An integer raster over two: round-half-even ties of both signs, and -0.5 -> -0.0."""
    return _frozen(np.ascontiguousarray(x * x.dtype.type(0.5)))


def bits(a):
    """The bit patterns of a float raster, every NaN as one pattern."""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = 0
    return u


# ---------------------------------------------------------------------------
# Fourier destripe
# ---------------------------------------------------------------------------
FOURIER_REGIMES = ("base", "below_sea", "zero_cross", "high_8000", "milli", "huge_1e30")
FOURIER_SHAPES = ((256, 300), (256, 256))    # rocFFT's 2-D inverse; the split inverse
FOURIER_MIXED = ((141, 156), (150, 155))     # odd x even, even x odd: the goldens have neither


@functools.lru_cache(maxsize=None)
def fourier_case(name, shape, seed=1):
    """(striped float32 raster in the regime, the oracle's result on the raster cast to
    float64 -- complex128 throughout --, its mask, the number of threshold-borderline cells of
    its margins by the rule of test_destripe_on_a_larger_raster_against_the_oracle)."""
    from oracle import hdem_oracle_fourier as F
    dem = F.synth_striped_dem(*shape, seed=seed)
    if name != "base":
        dem = np.ascontiguousarray(FILTER_REGIMES[name](dem), np.float32)
    want, mask, stages = F.detect_apply_fourier(dem.astype(np.float64))
    borderline = sum(int((np.abs(g) <= 1e-4 * np.abs(g).max()).sum())
                     for pair in stages["margins"] for g in pair)
    return _frozen(dem, want, mask) + (borderline,)


# ---------------------------------------------------------------------------
# lagoon branch: power-of-two scalings
# ---------------------------------------------------------------------------
LAGOON_SHAPE = (131, 157)
LAGOON_POWERS = (0, 6, -100, 100)


@functools.lru_cache(maxsize=None)
def lagoon_case(power):
    """(synth_hsheds with its non-void cells times 2^power, the oracle's mask, its stages
    plus ``GreyDilation``: the 7 x 7 dilation of the repaired raster)."""
    from oracle import hdem_oracle_lagoons as L
    hs = L.synth_hsheds(*LAGOON_SHAPE, seed=4)
    void = hs < 0
    assert void.any() and (hs[~void] > 0).all()
    hs = np.where(void, hs, np.ldexp(hs, power)).astype(np.float32)
    assert np.isfinite(hs).all() and (hs[~void] >= np.finfo(np.float32).tiny).all()
    mask, stages = L.lagoons_detection(hs)
    # (a void without a neighbour >= 0 is repaired to NaN, and the maximum of a window that
    # holds a NaN is whatever order SciPy compares in: the dilation's input keeps the void code)
    fixed = stages["CorrectNANValues"]
    grey_in = np.where(np.isnan(fixed), hs, fixed)
    assert np.isnan(fixed).any() and (grey_in < 0).any()
    stages = dict(stages, GreyDilationInput=grey_in,
                  GreyDilation=L.grey_dilation(grey_in, (7, 7)))
    return _frozen(hs, mask), {k: _frozen(v) for k, v in stages.items()}


@functools.lru_cache(maxsize=None)
def lagoon_specials():
    """The same raster with a plateau of +inf and a lake of -0.0 (not a void: -0.0 < 0 is
    false), both wide enough to win an 11 x 11 majority."""
    from oracle import hdem_oracle_lagoons as L
    hs = L.synth_hsheds(*LAGOON_SHAPE, seed=4).copy()
    hs[20:45, 30:60] = np.inf
    hs[70:100, 90:125] = -0.0
    with np.errstate(invalid="ignore"):
        fixed = L.correct_nan_values(hs)
        major = L.majority_filter(fixed, 11)
        grey = L.grey_dilation(fixed, (7, 7))
    return _frozen(hs, fixed, major, grey)


def convolve_weights():
    """The 5 x 3 and 15 x 15 random weights of test_convolve_general_weights."""
    rng = np.random.default_rng(3)
    w = {shape: rng.standard_normal(shape) for shape in [(3, 3), (5, 3), (1, 7), (15, 15)]}
    return w[(5, 3)], w[(15, 15)]
