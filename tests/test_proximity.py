"""
Euclidean proximity (``hdem_proximity``, include/hydrodem_hip.h A15) without a device: the
references that tests/test_gpu_proximity.py holds the kernels to, checked against each other
and against SciPy, and the argument checks of ``hydrodem_amd.proximity.proximity_args``.

``brute``: every cell against every source, the sources in the order of their flat index, so
that ``argmin`` (the first minimum) applies the tie rule of the contract.  ``separable``: the
two passes the kernels make -- nearest source of the own row, ties to the left, then the
minimum over the rows of a column, ties upwards -- in NumPy integers.  The float formulas of
``distance``, ``rise`` and ``burned`` are written exactly as the header states them: float64
square root and product rounded once, float32 products and differences one at a time.
"""
import types

import numpy as np
import pytest
from scipy import ndimage

from hydrodem_amd import proximity as P

F32 = np.float32
UNREACHED = np.uint32(0xFFFFFFFF)


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
def brute(sources, block=1 << 22):
    """``(d2, nearest)`` of a bool raster, uint32, 0xFFFFFFFF everywhere without a source."""
    h, w = sources.shape
    flat = np.flatnonzero(sources)                       # ascending: the tie rule
    d2 = np.full(h * w, UNREACHED, np.uint32)
    nearest = np.full(h * w, UNREACHED, np.uint32)
    if flat.size:
        sr, sx = (flat // w).astype(np.int64), (flat % w).astype(np.int64)
        step = max(1, block // flat.size)
        for lo in range(0, h * w, step):
            cells = np.arange(lo, min(lo + step, h * w))
            r, x = cells // w, cells % w
            dist = (r[:, None] - sr[None, :]) ** 2 + (x[:, None] - sx[None, :]) ** 2
            k = dist.argmin(axis=1)
            d2[cells] = dist[np.arange(cells.size), k]
            nearest[cells] = flat[k]
    return d2.reshape(h, w), nearest.reshape(h, w)


def row_pass(sources):
    """The column of the nearest source of every cell's own row, ties to the left; -1: none."""
    h, w = sources.shape
    cols = np.broadcast_to(np.arange(w, dtype=np.int64), (h, w))
    far = np.int64(1) << 40
    left = np.maximum.accumulate(np.where(sources, cols, -far), axis=1)
    right = np.minimum.accumulate(np.where(sources, cols, far)[:, ::-1], axis=1)[:, ::-1]
    pick = np.where(cols - left <= right - cols, left, right)
    return np.where(np.abs(pick) >= far, -1, pick)


def separable(sources):
    """``(d2, nearest)`` by the two passes; the same results as :func:`brute`."""
    h, w = sources.shape
    xs = row_pass(sources)
    cols = np.arange(w, dtype=np.int64)
    far = np.int64(1) << 40
    g2 = np.where(xs < 0, far, (xs - cols[None, :]) ** 2)
    rows = np.arange(h, dtype=np.int64)
    d2 = np.empty((h, w), np.int64)
    arg = np.empty((h, w), np.int64)
    for r in range(h):
        cost = (rows - r)[:, None] ** 2 + g2
        arg[r] = cost.argmin(axis=0)                     # the first minimum: ties upwards
        d2[r] = cost[arg[r], cols]
    out = d2 >= far
    nearest = arg * w + xs[arg, cols[None, :]]
    return (np.where(out, UNREACHED, d2).astype(np.uint32),
            np.where(out, UNREACHED, nearest).astype(np.uint32))


def within(d2, nearest, max_distance):
    """The two rasters with the cells beyond ``max_distance`` (0 or None: none) out of reach."""
    if not max_distance:
        return d2, nearest
    out = d2.astype(np.uint64) > np.uint64(max_distance) ** 2
    return np.where(out, UNREACHED, d2), np.where(out, UNREACHED, nearest)


def label_of(labels, nearest):
    out = nearest == UNREACHED
    return np.where(out, 0, labels.ravel()[np.where(out, 0, nearest)]).astype(np.uint32)


def distance_of(d2, cellsize):
    out = d2 == UNREACHED
    value = (np.sqrt(d2.astype(np.float64)) * np.float64(cellsize)).astype(F32)
    return np.where(out, F32(np.nan), value).astype(F32)


def rise_of(dem, nearest):
    out = nearest == UNREACHED
    with np.errstate(invalid="ignore"):
        value = dem - dem.ravel()[np.where(out, 0, nearest)]
    return np.where(out, F32(np.nan), value).astype(F32)


def burned_of(dem, d2, buffer, smooth, sharp):
    out = d2 == UNREACHED
    d = np.sqrt(d2.astype(np.float64)).astype(F32)
    inv = F32(1.0 / float(buffer))
    with np.errstate(invalid="ignore"):
        t = F32(1) - d * inv
        lowered = (dem - F32(smooth) * t) - np.where(d2 == 0, F32(sharp), F32(0))
    assert t.dtype == lowered.dtype == np.dtype(F32)
    return np.where(~out & (d < F32(buffer)), lowered, dem).astype(F32)


def reference(sources, max_distance=None, dem=None, labels=None, cellsize=1.0, buffer=None,
              smooth=0.0, sharp=0.0, how=brute):
    """Every output of the call that the operands allow, as the header defines them."""
    d2, nearest = within(*how(sources), max_distance)
    ref = {"d2": d2, "nearest": nearest, "distance": distance_of(d2, cellsize)}
    if labels is not None:
        ref["label"] = label_of(labels, nearest)
    if dem is not None:
        ref["rise"] = rise_of(dem, nearest)
        if buffer is not None:
            ref["burned"] = burned_of(dem, d2, buffer, smooth, sharp)
    return ref


# ---------------------------------------------------------------------------
# source layouts
# ---------------------------------------------------------------------------
def checkerboard(shape):
    r, x = np.indices(shape)
    return (r + x) % 2 == 0


def mirrored_pair(shape):
    """Two sources mirrored about the centre: every cell of the axis between them is a tie."""
    h, w = shape
    s = np.zeros(shape, bool)
    s[h // 4, w // 4] = s[h - 1 - h // 4, w - 1 - w // 4] = True
    return s


def full_row(shape):
    s = np.zeros(shape, bool)
    s[shape[0] // 2, :] = True
    return s


def full_column(shape):
    s = np.zeros(shape, bool)
    s[:, shape[1] // 2] = True
    return s


def random_sources(shape, density, seed=3):
    return np.random.default_rng([seed, *shape]).random(shape) < density


TIES = {"checkerboard": checkerboard, "mirrored": mirrored_pair, "row": full_row,
        "column": full_column}
SMALL = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 7), (8, 13), (13, 8), (12, 12)]


# ---------------------------------------------------------------------------
# the references against each other and against SciPy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.1, 0.5])
def test_brute_force_and_the_two_passes_agree(density):
    for seed in range(12):
        rng = np.random.default_rng([seed, int(density * 100)])
        shape = tuple(rng.integers(1, 14, 2))
        s = rng.random(shape) < density
        for got, want in zip(separable(s), brute(s)):
            assert got.dtype == np.uint32 and np.array_equal(got, want), (shape, seed)


@pytest.mark.parametrize("density", [0.02, 0.1, 0.5])
def test_the_squared_distance_is_scipys(density):
    for seed in range(12):
        rng = np.random.default_rng([seed, 77, int(density * 100)])
        shape = tuple(rng.integers(1, 14, 2))
        s = rng.random(shape) < density
        s[rng.integers(shape[0]), rng.integers(shape[1])] = True         # SciPy needs one
        want = np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.uint32)
        assert np.array_equal(brute(s)[0], want) and np.array_equal(separable(s)[0], want)


@pytest.mark.parametrize("layout", list(TIES))
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_ties_go_to_the_smallest_flat_index(layout, shape):
    s = TIES[layout](shape)
    d2, nearest = brute(s)
    for got, want in zip(separable(s), (d2, nearest)):
        assert np.array_equal(got, want)
    # by the definition itself, cell by cell
    h, w = shape
    flat = np.flatnonzero(s)
    for c in range(h * w):
        dist = (c // w - flat // w) ** 2 + (c % w - flat % w) ** 2
        assert d2.ravel()[c] == dist.min()
        assert nearest.ravel()[c] == flat[dist == dist.min()].min()


def test_a_tie_is_there_to_break():
    d2, nearest = brute(mirrored_pair((8, 8)))
    first, second = 2 * 8 + 2, 5 * 8 + 5
    assert set(np.unique(nearest)) == {first, second}
    r, x = np.indices((8, 8))
    tied = (r - 2) ** 2 + (x - 2) ** 2 == (r - 5) ** 2 + (x - 5) ** 2
    assert tied.sum() == 8 and (nearest[tied] == first).all()


def test_without_a_source_and_beyond_max_distance_a_cell_is_out_of_reach():
    empty = np.zeros((5, 6), bool)
    for how in (brute, separable):
        d2, nearest = how(empty)
        assert (d2 == UNREACHED).all() and (nearest == UNREACHED).all()
    s = np.zeros((9, 9), bool)
    s[4, 4] = True
    dem = np.arange(81, dtype=F32).reshape(9, 9)
    dem[0, 0] = np.nan
    labels = s.astype(np.uint32) * 7
    ref = reference(s, 2, dem, labels, 30.0, 3.0, 5.0, 1.0)
    far = ref["d2"] == UNREACHED
    assert far.sum() == 81 - 13 and (ref["nearest"][far] == UNREACHED).all()
    assert (ref["label"][far] == 0).all() and (ref["label"][~far] == 7).all()
    assert np.isnan(ref["distance"][far]).all() and np.isnan(ref["rise"][far]).all()
    assert np.array_equal(ref["burned"][far], dem[far], equal_nan=True)
    assert ref["distance"][4, 6] == F32(60.0) and ref["rise"][4, 6] == F32(2.0)
    # on the source: smooth and sharp; one cell away: smooth * (1 - 1/3)
    assert ref["burned"][4, 4] == F32(40 - 5 - 1)
    assert ref["burned"][4, 5] == F32(41) - F32(5) * (F32(1) - F32(1) * F32(1 / 3))
    assert ref["burned"][4, 6] < dem[4, 6] and ref["burned"][3, 3] < dem[3, 3]


# ---------------------------------------------------------------------------
# proximity_args
# ---------------------------------------------------------------------------
def like(shape, dtype):
    return types.SimpleNamespace(shape=shape, dtype=np.dtype(dtype))


MASK, ACC, DEM = like((4, 5), np.uint8), like((4, 5), np.uint32), like((4, 5), np.float32)


def test_the_kinds_of_sources_and_the_order_of_the_outputs():
    assert P.proximity_args(MASK)[:4] == (P.SOURCES_MASK_U8, 0, 0, ("distance",))
    assert P.proximity_args(ACC, 10, "d2")[:4] == (P.SOURCES_ACC_U32, 10, 0, ("d2",))
    kind, threshold, reach, want, numbers = P.proximity_args(
        ACC, None, ("burned", "label", "rise", "d2"), DEM, 30, 7, 4, 2, 1)
    assert (kind, threshold, reach) == (P.SOURCES_LABELS_U32, 0, 7)
    assert want == ("d2", "label", "rise", "burned") and numbers == (30.0, 4.0, 2.0, 1.0)
    assert (P.SOURCES_MASK_U8, P.SOURCES_ACC_U32, P.SOURCES_LABELS_U32) == (1, 2, 3)
    assert [n for n, _ in P.PROXIMITY_OUTPUTS] == ["d2", "nearest", "label", "distance", "rise",
                                                   "burned"]


REFUSALS = [
    (lambda: P.proximity_args(None), "needs the source raster"),
    (lambda: P.proximity_args(like((4, 5), np.float32)), "sources are a uint8 mask"),
    (lambda: P.proximity_args(like((4, 5), np.int64)), "sources are a uint8 mask"),
    (lambda: P.proximity_args(like((4,), np.uint8)), "2-D raster"),
    (lambda: P.proximity_args(like((2, 4, 5), np.uint8)), "2-D raster"),
    (lambda: P.proximity_args(MASK, want=()), "no output wanted"),
    (lambda: P.proximity_args(MASK, want=("slope",)), "unknown proximity outputs"),
    (lambda: P.proximity_args(MASK, want="label"), "label needs a uint32 label raster"),
    (lambda: P.proximity_args(ACC, 10, "label"), "label needs a uint32 label raster"),
    (lambda: P.proximity_args(MASK, want="rise"), "rise needs the float32 dem"),
    (lambda: P.proximity_args(MASK, want="burned", buffer=3), "burned needs the float32 dem"),
    (lambda: P.proximity_args(MASK, 5), "takes no threshold"),
    (lambda: P.proximity_args(ACC, 0), "threshold is an integer in 1"),
    (lambda: P.proximity_args(ACC, 2.5), "threshold is an integer in 1"),
    (lambda: P.proximity_args(ACC, True), "threshold is an integer in 1"),
    (lambda: P.proximity_args(ACC, 1 << 32), "threshold is an integer in 1"),
    (lambda: P.proximity_args(MASK, dem=like((4, 5), np.float64)), "the dem is float32"),
    (lambda: P.proximity_args(MASK, dem=like((5, 4), np.float32)), "the dem is (5, 4)"),
    (lambda: P.proximity_args(MASK, cellsize=0), "cellsize must be finite and positive"),
    (lambda: P.proximity_args(MASK, cellsize=-30.0), "cellsize must be finite and positive"),
    (lambda: P.proximity_args(MASK, cellsize=float("nan")), "cellsize must be finite"),
    (lambda: P.proximity_args(MASK, max_distance=-1), "max_distance is a whole number"),
    (lambda: P.proximity_args(MASK, max_distance=1.5), "max_distance is a whole number"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM), "burned needs a buffer"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM, buffer=0), "buffer must be finite"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM, buffer=-2), "buffer must be finite"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM, buffer=float("inf")),
     "buffer must be finite"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM, buffer=2, smooth=-1),
     "smooth must be finite and not negative"),
    (lambda: P.proximity_args(MASK, want="burned", dem=DEM, buffer=2, sharp=float("nan")),
     "sharp must be finite and not negative"),
    (lambda: P.proximity_args(like((1, 65536), np.uint8)), "a side of more than 65535"),
    (lambda: P.proximity_args(like((65536, 1), np.uint8)), "a side of more than 65535"),
    (lambda: P.proximity_args(like((1, 65537), np.uint8)), "squared diagonal"),
    (lambda: P.proximity_args(like((65537, 1), np.uint8)), "squared diagonal"),
    (lambda: P.proximity_args(like((65535, 65535), np.uint8)), "squared diagonal"),
    (lambda: P.proximity_args(like((3, 1 << 31), np.uint8)), "more than 2^32 - 1 cells"),
    (lambda: P.proximity_args(like((0, 5), np.uint8)), "a raster with cells"),
]


@pytest.mark.parametrize("call,words", REFUSALS, ids=[words for _, words in REFUSALS])
def test_a_bad_call_is_refused_without_a_device(call, words):
    with pytest.raises(ValueError) as refusal:
        call()
    assert words in str(refusal.value)


def test_the_largest_rasters_pass():
    assert P.proximity_args(like((32768, 32768), np.uint8))[0] == P.SOURCES_MASK_U8
    assert P.proximity_args(like((1, 65535), np.uint8))[0] == P.SOURCES_MASK_U8
    assert P.proximity_args(like((65535, 1), np.uint32), 1)[0] == P.SOURCES_ACC_U32
    assert P.proximity_args(like((46341, 46341), np.uint8))[0] == P.SOURCES_MASK_U8
    with pytest.raises(ValueError):
        P.proximity_args(like((46342, 46342), np.uint8))     # 2 * 46341^2 > 2^32 - 2


def test_the_filters_check_their_operands_at_construction():
    import hydrodem_amd as hd
    mask = np.zeros((4, 5), bool)
    acc = np.ones((4, 5), np.uint32)
    assert hd.EuclideanDistance(mask).sources.dtype == np.uint8
    assert hd.EuclideanAllocation(acc, threshold=3).threshold == 3
    assert hd.BurnStreams(acc, threshold=2, buffer=3, smooth=5.0, sharp=1.0).buffer == 3
    for bad in (lambda: hd.EuclideanDistance(mask, threshold=3),
                lambda: hd.EuclideanDistance(acc, threshold=0),
                lambda: hd.EuclideanDistance(mask, cellsize=0),
                lambda: hd.EuclideanDistance(mask.astype(np.float32)),
                lambda: hd.BurnStreams(None, buffer=3),
                lambda: hd.BurnStreams(mask, buffer=0),
                lambda: hd.BurnStreams(mask, buffer=3, smooth=-1),
                lambda: hd.BurnStreams(mask, buffer=3).apply(np.zeros((4, 5), np.float64)),
                lambda: hd.BurnStreams(mask, buffer=3).apply(np.zeros((5, 4), np.float32)),
                lambda: hd.EuclideanDistance(mask).apply(np.zeros((5, 4), np.float32))):
        with pytest.raises(ValueError):
            bad()
