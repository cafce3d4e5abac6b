"""
Elevation regimes and D8 tie rasters: inputs for tests/test_elevation_regimes.py (the CPU
references among themselves) and tests/test_gpu_elevation_regimes.py (the HIP operators
against them).  A plain helper module: rasters and cached oracle results, nothing else.

Every other terrain raster of the suite lies at 50 ... 130 m, positive, with metres of relief.
``REGIMES`` moves the synthetic DEM to where the sign, the magnitude or the spacing of float32
matters to the fill, D8, ``ResolveFlats``, the flow trace and the depression inventory:

  below_sea   z - 600                 every value negative (keys, sentinels, a 0 fed into a lane)
  zero_cross  z - round(mean z)       both signs, +0 and -0 in one raster
  high_8000   z + 8000                one ulp (4.9e-4) is of the size of epsilon
  milli       (z - 100) * 1e-3        relief far below epsilon
  tiny        (z - 100) * 1e-30       normal floats near the bottom of the range
  huge_1e30   z * 1e30                epsilon vanishes in one ulp, depth quanta saturate
  near_max    z * 3.0e36              values on both sides of 3.0e38 (the hub raster's wall
                                      constant), all finite
  ulp_ladder  1000.0f + k ulps        neighbours a few ulps apart: ties and strict inequalities

``d8_tie_raster`` / ``d8_tie_strip`` hold the 48 patterns in which the float32 drop
``(zc - zk) * 0.70710678f`` towards a diagonal neighbour equals the drop towards a cardinal
one exactly, while exact arithmetic separates the two by about 1e-4 ulp: the first of the two
in window order must win, and a D8 that computes the drop in another precision, or divides by
sqrt 2 instead, picks the other one.
"""
import functools

import numpy as np

import hdem_synth
from oracle import c_oracle
from oracle.hdem_oracle_np import D8_CODES, D8_OFFSETS

HUB_BIG = np.float32(3.0e38)


# ---------------------------------------------------------------------------
# float32 a number of ulps away
# ---------------------------------------------------------------------------
def ulps_from(base, n):
    """The float32 ``n`` representable values above ``base`` (below for negative ``n``);
    ``base`` a non-zero finite scalar, ``n`` an integer or an integer array that does not
    carry the value across zero."""
    bits = np.array(base, np.float32).view(np.int32).astype(np.int64)
    n = np.asarray(n, np.int64)
    moved = bits + n if bits >= 0 else bits - n        # the magnitude of a negative float shrinks upwards
    return moved.astype(np.int32).view(np.float32)


# ---------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------
def _zero_cross(z):
    out = (z - np.float32(np.round(z.mean(dtype=np.float64)))).astype(np.float32)
    flat = out.ravel()
    zeros = np.flatnonzero(flat == 0)
    if zeros.size < 6:                                 # no exact zero among noisy metres: the six
        zeros = np.argsort(np.abs(flat), kind="stable")[:6]     # cells nearest to it become one
        flat[zeros] = 0.0
    flat[zeros[::3][:8]] = -0.0                        # a handful of them with a minus sign
    assert (np.signbit(flat) & (flat == 0)).any() and (~np.signbit(flat) & (flat == 0)).any()
    assert (flat < 0).any() and (flat > 0).any()
    return out


def _near_max(z):
    with np.errstate(over="ignore"):
        out = z * np.float32(3.0e36)
    assert np.isfinite(out).all(), "near_max left float32: the raster is too high for it"
    assert (out >= HUB_BIG).any() and (out < HUB_BIG).any()
    return out


def _ulp_ladder(z):
    steps = np.round((z.astype(np.float64) - np.float64(z.min())) * 40.0).astype(np.int64)
    return ulps_from(1000.0, steps)


REGIMES = {
    "below_sea": lambda z: z - np.float32(600.0),
    "zero_cross": _zero_cross,
    "high_8000": lambda z: z + np.float32(8000.0),
    "milli": lambda z: (z - np.float32(100.0)) * np.float32(1e-3),
    "tiny": lambda z: (z - np.float32(100.0)) * np.float32(1e-30),
    "huge_1e30": lambda z: z * np.float32(1e30),
    "near_max": _near_max,
    "ulp_ladder": _ulp_ladder,
}


def _near_max_basin(z):
    """``near_max`` with a basin of whole 16 x 16 blocks 20 m lower: block maxima between
    1.7e38 and 3.0e38, below the wall constant and above half of FLT_MAX -- twice the largest
    of them, the span the epsilon-coarse start sizes its rounding allowance by, overflows."""
    z = z.copy()
    z[48:80, 48:96] -= np.float32(20.0)
    out = _near_max(z)
    top = out[48:80, 48:96].reshape(2, 16, 3, 16).max(axis=(1, 3))
    assert (top < HUB_BIG).all() and (top > np.float32(1.7e38)).all()
    return out


# (not a regime of its own: one more raster for the epsilon-coarse start)
RASTERS = dict(REGIMES, near_max_basin=_near_max_basin)
VARIANTS = ("rough", "srtm")
TILE = 62                                              # interior tile edge of the fill


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def regime_raster(name, shape, variant="rough", nodata=False):
    """The regime's float32 raster (read-only, shared).  ``nodata``: one block and one cell on
    the corner of four tiles become NaN (asked for on rasters of 200 x 333 and above)."""
    z = RASTERS[name](hdem_synth.synth_dem(*shape, variant=variant))
    assert z.dtype == np.float32 and z.shape == tuple(shape) and np.isfinite(z).all(), name
    if nodata:
        z = z.copy()
        z[120:128, 200:215] = np.nan
        z[TILE + 1, TILE + 1] = np.nan                 # first cell of tile (1, 1)
    return _frozen(z)


@functools.lru_cache(maxsize=None)
def regime_fill(name, shape, variant="rough", nodata=False, eps=0.0):
    """(raster, its priority-flood fill, the D8 codes of the fill): computed once, read-only."""
    z = regime_raster(name, shape, variant, nodata)
    want = c_oracle.sinkfill_pflood(z, eps=eps)
    return _frozen(z, want, c_oracle.d8(want))


# ---------------------------------------------------------------------------
# D8 ties
# ---------------------------------------------------------------------------
TIE_BASES = (1000.0, -300.0, 8000.0)
# (a, b): a * 1.0f == fl(b * 0.70710678f) in float32 for a difference of a / b ulps inside one
# binade; b / sqrt 2 - a is about 1e-4
TIE_PAIRS = ((2378, 3363), (4756, 6726), (5741, 8119))
CARDINAL = tuple(k for k, (dy, dx) in enumerate(D8_OFFSETS) if dy == 0 or dx == 0)
DIAGONAL = tuple(k for k in range(8) if k not in CARDINAL)
HIGHER = 20000                                         # ulps: every other cell of a window
LOWER, LOWEST = -30000, -40000                         # ulps: outlets of the draining strip


def tie_patterns():
    """The 48 (a, b, window index of the cardinal, of the diagonal neighbour)."""
    return [(a, b, kc, kd) for a, b in TIE_PAIRS for kc in CARDINAL for kd in DIAGONAL]


def _place(steps, cy, cx, pattern):
    a, b, kc, kd = pattern
    steps[cy - 1:cy + 2, cx - 1:cx + 2] = HIGHER
    steps[cy, cx] = 0
    steps[cy + D8_OFFSETS[kc][0], cx + D8_OFFSETS[kc][1]] = -a
    steps[cy + D8_OFFSETS[kd][0], cx + D8_OFFSETS[kd][1]] = -b
    return D8_CODES[min(kc, kd)]                       # the earlier of the two in window order


def d8_tie_raster(base):
    """25 x 33 raster of the 48 patterns, centres 4 cells apart from (2, 2), everything outside
    a pattern's two low cells 20000 ulps above ``base``.  Returns (raster, centres, expected):
    ``centres`` the (rows, columns) index pair of the 48 centres, ``expected`` their codes."""
    patterns = tie_patterns()
    steps = np.full((25, 33), HIGHER, np.int64)
    rows, cols, expected = [], [], []
    for k, pattern in enumerate(patterns):
        cy, cx = 2 + 4 * (k // 8), 2 + 4 * (k % 8)
        expected.append(_place(steps, cy, cx, pattern))
        rows.append(cy)
        cols.append(cx)
    z = ulps_from(base, steps)
    return _frozen(z, np.array(rows), np.array(cols), np.array(expected, np.uint8))


def d8_tie_strip(base):
    """The draining form: the same 48 patterns side by side in a 3 x 193 strip that is its own
    fill, with and without a gradient.  The centres are the interior row; a window's north and
    south rows are raster ring; the column between two windows -- outside either -- is 30000
    ulps below ``base`` on the ring rows, so that a low west or east neighbour, and the high
    cell between two windows, have a lower outlet next to them.  Same return as
    ``d8_tie_raster``."""
    patterns = tie_patterns()
    steps = np.full((3, 4 * len(patterns) + 1), HIGHER, np.int64)
    steps[0, 0::4] = steps[2, 0::4] = LOWER
    steps[1, 0] = steps[1, -1] = LOWER
    cols, expected = [], []
    for k, pattern in enumerate(patterns):
        expected.append(_place(steps, 1, 2 + 4 * k, pattern))
        cols.append(2 + 4 * k)
    z = ulps_from(base, steps)
    return _frozen(z, np.ones(len(cols), np.int64), np.array(cols), np.array(expected, np.uint8))


def shifted_right(z, rows, cols, base):
    """``z`` behind one more column on the left (40000 ulps below ``base``: an outlet for what
    was the first column), so that every row starts one float off a 16-byte boundary."""
    first = np.full((z.shape[0], 1), ulps_from(base, LOWEST), np.float32)
    return _frozen(np.concatenate([first, z], axis=1)), rows, cols + 1


# ---------------------------------------------------------------------------
# two D8 restatements that break the arithmetic contract
# ---------------------------------------------------------------------------
def _d8_with(z, drop_of):
    z = np.ascontiguousarray(z, np.float32)
    h, w = z.shape
    out = np.zeros((h, w), np.uint8)
    zc = z[1:-1, 1:-1]
    best = np.zeros(zc.shape, np.float64)
    code = np.zeros(zc.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        for (dy, dx), c in zip(D8_OFFSETS, D8_CODES):
            drop = drop_of(zc, z[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx], dy != 0 and dx != 0)
            better = drop > best
            best = np.where(better, drop, best)
            code = np.where(better, np.uint8(c), code)
    out[1:-1, 1:-1] = code
    return out


def d8_drop_in_float64(z):
    """Wrong on purpose: the drop in float64 (the weight still the float32 constant)."""
    weight = np.float64(np.float32(0.70710678))
    return _d8_with(z, lambda zc, zk, diag: (zc.astype(np.float64) - zk.astype(np.float64))
                    * (weight if diag else 1.0))


def d8_divided_by_sqrt2(z):
    """Wrong on purpose: float32, but the diagonal drop divided by 1.4142135f."""
    return _d8_with(z, lambda zc, zk, diag: ((zc - zk) / np.float32(1.4142135) if diag
                                             else zc - zk).astype(np.float64))
