"""
Regimes of the Fourier destripe: inputs for tests/test_fourier_cases.py (the predicates, on the
CPU oracle alone) and tests/test_gpu_fourier_regimes.py (the HIP kernels on them).
A plain helper module: the launch geometry of ``blanks_pass`` restated, the rule by which a
block of the second detection pass is skipped, builders of the rasters that reach the far side
of each decision, and the oracle's answers, each made once and frozen.

  decision (hdem_fourier.hip)                          trivial until        predicate
  a block of the second pass returns at once when no   (terrain spectra:    visited,
    first-pass peak lies in the occupancy cells of       nearly every        visited_without_rows,
    its 512 columns and its rows +- R                    block is visited)   visited_without_context
  the FULL form of hollow_detect4_body (clamped        quadrant width 943,  is_full
    loads without a condition, masked afterwards)        W = 1906
  sum_partial_kernel reads every step-th cell          H * W = 2^21         level_step
  the smallest quadrant the 55-cell window fits        130 x 130            quadrant

Terrain spectra are heavy-tailed and put peaks everywhere, so the rasters of the first three
rows are white Gaussian noise of sigma 1 m around a level with *pairs* of cosine waves on exact
bins (no leakage): a pair (i, j, amp) puts amplitude ``amp`` on the cells (i, j) and (i, j + 1)
of the first quadrant, in shifted coordinates.  Two adjacent cells survive IsolatedPoints, a lone
noise peak does not.  A strong pair A (amplitude 10) within 27 cells of a weak pair B (0.03)
lifts B's hollow mean above a quarter of B: the first pass finds A alone and zeroes it, the second
finds B.  The noise alone crosses 4 x its hollow mean in about 3.5e-6 of the cells.

Borderline cells.  The GPU's transform is rocFFT's in complex64, the oracle's is fftpack's in
complex128: magnitudes differ by up to FFT_RTOL * max|F|.  A cell decides differently only if
its margin q - 4 * mean is smaller than what q and the mean can be off by together:
BORDERLINE * FFT_RTOL * max|F|, 1 for q plus 4 for the mean, which errs at most as its cells do.
The seeds below are ones at which NO cell of either pass of either quadrant is that close
(tests/test_fourier_cases.py asserts it; about every second seed of the three noise rasters and
one in fifteen of the 2 M-cell ones is), so the GPU tests ask for the oracle's mask exactly.
"""
import functools

import numpy as np
from scipy import fftpack

from oracle import hdem_oracle_fourier as F

# ---------------------------------------------------------------------------
# the kernels' constants, each with the line it mirrors
# ---------------------------------------------------------------------------
WINDOW = 55                 # blanks_pass `int window = 55`
R = WINDOW // 2             # blanks_pass `const int R = window / 2` (hollow_detect4_kernel<27, 2>)
H4W = 512                   # `constexpr int H4T = 128, H4W = 4 * H4T`: columns a block loads
OUTW = H4W - 2 * R          # `per_block4 = H4W - 2 * R`: 458 columns a block writes
SEG_FIRST, SEG_LAST = 256, 32   # blanks_pass `int seg4 = 256; while (seg4 > 32 && ...) seg4 /= 2`
SEG_BLOCKS = 4096           # ... `(int64_t)bx4 * ((h + seg4 - 1) / seg4) < 4096`
OCC = 32                    # `y >> 5`, `(c0 + k) >> 5`: the occupancy cells are 32 x 32
MARGIN = 10                 # make_geom `g.qh = g.mid_y - 10`
SUM_STEP_SHIFT = 20         # hdem_fourier_destripe_f32_dev `step = n >> 20 ? n >> 20 : 1`
FFT_RTOL = 2e-6             # tests/test_gpu_fourier.py: complex64 transforms, relative to max|F|
BORDERLINE = 5              # 1 for the cell's own magnitude, 4 for the mean


def _ceil(a, b):
    return -(-int(a) // int(b))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------
# the geometry and the skip rule
# ---------------------------------------------------------------------------
def quadrant(shape):
    """make_geom: (qh, qw), a quarter less its 10-cell margin."""
    return shape[0] // 2 - MARGIN, shape[1] // 2 - MARGIN


def block_columns(qw):
    """blanks_pass `bx4 = (w + per_block4 - 1) / per_block4`."""
    return _ceil(qw, OUTW)


def segment_rows(q):
    """blanks_pass: the rows one block walks, halved from 256 while the grid has fewer than
    4 096 blocks, 32 at the least."""
    qh, qw = q
    seg = SEG_FIRST
    while seg > SEG_LAST and block_columns(qw) * _ceil(qh, seg) < SEG_BLOCKS:
        seg //= 2
    return seg


def grid(q):
    """(block columns, segments) of the detection launch."""
    return block_columns(q[1]), _ceil(q[0], segment_rows(q))


def first_column(bx):
    """hollow_detect4_body `c_first = (int)blockIdx.x * outw - R`."""
    return bx * OUTW - R


def is_full(bx, qw):
    """hollow_detect4_kernel `if (c_first >= 0 && c_first + H4W <= w)`: the FULL form."""
    return first_column(bx) >= 0 and first_column(bx) + H4W <= qw


def block_of(q, y, x):
    """(block column, segment) of the block that writes the quadrant cell (y, x)."""
    return x // OUTW, y // segment_rows(q)


def occupancy(hits):
    """`occ_mark[(y >> 5) * occ_w + ((c0 + k) >> 5)] = 1` for every hit of the first pass."""
    qh, qw = hits.shape
    occ = np.zeros((_ceil(qh, OCC), _ceil(qw, OCC)), bool)
    ys, xs = np.nonzero(hits)
    occ[ys // OCC, xs // OCC] = True
    return occ


def _any(occ, r_lo, r_hi, c_lo, c_hi):
    return bool(occ[r_lo:r_hi + 1, c_lo:c_hi + 1].any())


def _rows(q, by, reach):
    y0 = by * segment_rows(q)
    y1 = min(y0 + segment_rows(q), q[0])
    return max(y0 - reach, 0) // OCC, min(y1 - 1 + reach, q[0] - 1) // OCC


def visited(occ, q, bx, by):
    """The rule of hollow_detect4_body: `c_lo = max(c_first, 0) >> 5, c_hi = min(c_first + H4W
    - 1, w - 1) >> 5, r_lo = max(y0 - R, 0) >> 5, r_hi = min(y1 - 1 + R, h - 1) >> 5`; the block
    goes on when any occupancy cell of that range is set."""
    c = first_column(bx)
    return _any(occ, *_rows(q, by, R), max(c, 0) // OCC, min(c + H4W - 1, q[1] - 1) // OCC)


def visited_without_rows(occ, q, bx, by):
    """A rule that is too small: the block's own rows, without the R rows above and below."""
    c = first_column(bx)
    return _any(occ, *_rows(q, by, 0), max(c, 0) // OCC, min(c + H4W - 1, q[1] - 1) // OCC)


def visited_without_context(occ, q, bx, by):
    """Another: the block's output columns, without the R columns of context on either side."""
    c = bx * OUTW
    return _any(occ, *_rows(q, by, R), c // OCC, min(c + OUTW - 1, q[1] - 1) // OCC)


def visits(occ, q, rule=visited):
    """The (block columns x segments) boolean table of the blocks ``rule`` visits."""
    nbx, nby = grid(q)
    return np.array([[rule(occ, q, bx, by) for by in range(nby)] for bx in range(nbx)])


def level_step(shape):
    """hdem_fourier_destripe_f32_dev `step = n >> 20 ? n >> 20 : 1`: sum_partial_kernel reads
    every step-th cell and sum_final_kernel divides by their number."""
    n = shape[0] * shape[1]
    return max(n >> SUM_STEP_SHIFT, 1)


# ---------------------------------------------------------------------------
# the rasters
# ---------------------------------------------------------------------------
def wave_numbers(shape, i, j):
    """The wave numbers whose line falls on the shifted cell (i, j) of the upper left quadrant
    (and on its point mirror, which no quadrant holds)."""
    return shape[0] // 2 - i, shape[1] // 2 - j


def noise_with_pairs(shape, level, pairs, seed):
    """White noise of sigma 1 m around ``level`` plus, for every pair (i, j, amp), cosines of
    amplitude ``amp`` on the shifted cells (i, j) and (i, j + 1); float32."""
    h, w = shape
    z = level + np.random.default_rng(seed).standard_normal(shape)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    for i, j, amp in pairs:
        for jj in (j, j + 1):
            ky, kx = wave_numbers(shape, i, jj)
            # (the phase from integers modulo the size: exact bins at any raster size)
            z += amp * np.cos(2.0 * np.pi * ((ky * y % h) / h + (kx * x % w) / w))
    return z.astype(np.float32)


STRIPES = ((0.31, 0.07, 1.2), (0.12, -0.38, 0.8), (0.05, 0.45, 0.6))   # tests/test_gpu_fourier.py

A, B = 10.0, 0.03
# name -> (shape, level, pairs, seed); what each exists for is in the GPU file's docstring
NOISE_CASES = {
    "wide_300x1930": ((300, 1930), 100.0,
                      ((60, 300, A), (70, 305, B), (110, 440, A), (112, 462, B)), 2),
    "wide_130x4000": ((130, 4000), 100.0,
                      ((28, 300, A), (36, 305, B), (20, 1380, A), (22, 1395, B)), 5),
    "tall_4000x130": ((4000, 130), 100.0, ((1020, 20, A), (1030, 25, B)), 2),
}
# the rasters of the context-state test: the split inverse; the same cell count both ways round
STATE_SHAPES = ((256, 256), (256, 512), (512, 256))
STATE_PAIRS, STATE_SEED = ((40, 40, A), (48, 45, B)), 1
LEVEL_SHAPES = ((1024, 2048), (1031, 2039))       # step == 2; the split and the 2-D inverse
LEVELS = (8000.0, 100.0)
LEVEL_SEEDS = {(1024, 2048): 4, (1031, 2039): 11}      # the same noise at both levels


def level_pairs(shape):
    h, w = shape
    return ((h // 4, w // 8, 5.0), (h // 4 + 10, w // 8 + 5, B))


SMALL_CASES = {"small_130x130": ((130, 130), 1), "small_131x131": ((131, 131), 1),
               "small_130x131": ((130, 131), 1), "small_131x130": ((131, 130), 1)}


class Case:
    """A raster with the float64 oracle's answers, made once and left alone."""

    def __init__(self, dem, pairs=()):
        self.dem = _frozen(np.ascontiguousarray(dem, np.float32))
        self.shape = dem.shape
        self.q = quadrant(dem.shape)
        self.pairs = tuple(pairs)
        want, mask, stages = F.detect_apply_fourier(self.dem.astype(np.float64))
        self.want = _frozen(want)
        self.mask = _frozen(mask.astype(np.uint8))
        # per quadrant: the hits of the first and of the second pass, and their margins
        self.margins = stages["margins"]
        self.first = tuple(_frozen(g[0] > 0) for g in self.margins)
        self.second = tuple(_frozen(g[1] > 0) for g in self.margins)
        self.kept = tuple(_frozen(F.isolated_points(d) > 0) for d in stages["detected"])
        d64 = self.dem.astype(np.float64)
        self.scale = float(np.abs(fftpack.fft2(d64 - d64.mean())).max())

    def borderline(self):
        """The cells of both passes of both quadrants that rounding may decide."""
        width = BORDERLINE * FFT_RTOL * self.scale
        return sum(int((np.abs(m) <= width).sum()) for pair in self.margins for m in pair)

    def pair_cells(self, amp):
        """The boolean first-quadrant raster of the cells of the pairs of amplitude ``amp``."""
        cells = np.zeros(self.q, bool)
        for i, j, a in self.pairs:
            if a == amp:
                cells[i, j:j + 2] = True
        return cells


@functools.lru_cache(maxsize=None)
def noise_case(name):
    shape, level, pairs, seed = NOISE_CASES[name]
    return Case(noise_with_pairs(shape, level, pairs, seed), pairs)


@functools.lru_cache(maxsize=None)
def level_case(shape, level):
    pairs = level_pairs(shape)
    return Case(noise_with_pairs(shape, level, pairs, LEVEL_SEEDS[shape]), pairs)


@functools.lru_cache(maxsize=None)
def state_case(shape):
    if tuple(shape) == (300, 1930):
        return noise_case("wide_300x1930")
    return Case(noise_with_pairs(shape, 100.0, STATE_PAIRS, STATE_SEED), STATE_PAIRS)


@functools.lru_cache(maxsize=None)
def small_case(name):
    shape, seed = SMALL_CASES[name]
    return Case(F.synth_striped_dem(*shape, seed=seed, stripes=STRIPES))


def oracle_case(name):
    return noise_case(name) if name in NOISE_CASES else small_case(name)


ORACLE_CASES = tuple(NOISE_CASES) + tuple(SMALL_CASES)


@functools.lru_cache(maxsize=None)
def complex64_error(shape, level, fraction=1.0):
    """e32: the error, against the float64 oracle, of the CPU's own complex64 chain -- fftpack
    keeps float32 input in single precision -- run on dem - mean with the oracle's mask, the
    level added back before the |.|: the precision that the kernels claim.  ``fraction``: of
    the mean, the level that is subtracted (0.5: what a mean over twice the cells summed
    would be)."""
    case = level_case(shape, level)
    d64 = case.dem.astype(np.float64)
    mean = fraction * d64.mean()
    spec = fftpack.fft2((d64 - mean).astype(np.float32))
    assert spec.dtype == np.complex64
    keep = fftpack.ifftshift(1 - case.mask.astype(np.float32))
    back = fftpack.ifft2(spec * keep)
    assert back.dtype == np.complex64
    out = np.abs(back.astype(np.complex128) + mean)
    return float(np.abs(out - case.want).max())
