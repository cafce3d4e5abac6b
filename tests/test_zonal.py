"""
Zonal statistics without a device: ``zonal_np``, the NumPy restatement that the GPU tests hold
every column to (itself held to ``scipy.ndimage`` where that is unambiguous), the generators of
zone and value rasters that both files use, the derived ``mean`` and every refusal that is made
before the device is touched.
"""
import numpy as np
import pytest
from scipy import ndimage

import hydrodem_amd as hd
from hydrodem_amd import zonal

U32, U64 = np.uint32, np.uint64
NO_CELL = 0xFFFFFFFF
COUNTERS = ("zones", "unzoned", "clamped", "over_range")
SHAPES = [(1, 1), (1, 130), (130, 1), (64, 64), (65, 63), (129, 200), (257, 130)]


def key_of(v):
    """float32 -> uint32 whose unsigned order is the floats' order (-0.0 below +0.0)."""
    b = np.ascontiguousarray(v, np.float32).view(U32)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def float_of(k):
    k = np.asarray(k, U32)
    return np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32).view(np.float32)


def zonal_np(zones, values=None, frac_bits=16):
    """The table of ``zones`` (and ``values``) and the counters, with NumPy alone."""
    width = zones.shape[1]
    flat = zones.ravel()
    on = flat > 0
    at = np.flatnonzero(on).astype(U32)
    ids, inv = np.unique(flat[on], return_inverse=True)
    inv = inv.ravel()
    k = ids.size
    rows, cols = at // U32(width), at % U32(width)

    def gathered(start, how, what, where=slice(None)):
        out = np.full(k, start, what.dtype)
        how.at(out, inv[where], what[where])
        return out
    table = {"id": ids.astype(U32), "count": np.bincount(inv, minlength=k).astype(U32),
             "first": gathered(NO_CELL, np.minimum, at),
             "row_min": gathered(NO_CELL, np.minimum, rows),
             "row_max": gathered(0, np.maximum, rows),
             "col_min": gathered(NO_CELL, np.minimum, cols),
             "col_max": gathered(0, np.maximum, cols)}
    counters = {"zones": int(k), "unzoned": int((~on).sum()), "clamped": 0,
                "over_range": int((flat > flat.size).sum())}
    if values is None:
        return table, counters
    v = values.ravel()[on]
    if v.dtype == np.float32:
        ok = ~np.isnan(v)
        key = key_of(v)
        with np.errstate(invalid="ignore"):
            d = np.rint(v.astype(np.float64) * 2.0 ** frac_bits)
        bound = float(2 ** 31 - 1)
        counters["clamped"] = int((ok & (np.abs(d) > bound)).sum())
        q = np.where(ok, np.clip(d, -bound, bound), 0.0).astype(np.int64)
        total = np.zeros(k, np.int64)
    else:
        ok = np.ones(v.size, bool)
        key = v.astype(U32)
        q = v.astype(U64)
        total = np.zeros(k, U64)
    np.add.at(total, inv[ok], q[ok])
    packed_min = (key.astype(U64) << U64(32)) | at.astype(U64)
    packed_max = (key.astype(U64) << U64(32)) | (~at).astype(U64)
    low = gathered(U64(2 ** 64 - 1), np.minimum, packed_min, ok)
    high = gathered(U64(0), np.maximum, packed_max, ok)
    valid = np.bincount(inv[ok], minlength=k).astype(U32)
    table["valid"] = valid
    if v.dtype == np.float32:
        nan = np.float32(np.nan)
        table["min"] = np.where(valid > 0, float_of(low >> U64(32)), nan).astype(np.float32)
        table["max"] = np.where(valid > 0, float_of(high >> U64(32)), nan).astype(np.float32)
    else:
        table["min"] = np.where(valid > 0, low >> U64(32), 0).astype(v.dtype)
        table["max"] = np.where(valid > 0, high >> U64(32), 0).astype(v.dtype)
    table["at_min"] = (low & U64(NO_CELL)).astype(U32)
    table["at_max"] = ~(high & U64(NO_CELL)).astype(U32)
    table["sum"] = total
    return table, counters


def same_bits(a, b):
    """Equal dtype, shape and bytes: NaN equals NaN, -0.0 does not equal +0.0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_table(got, want):
    names = [n for n in got if n != "mean"]
    assert names == [n for n in zonal.ZONAL_COLUMNS if n in want], names
    for name in names:
        assert same_bits(got[name], want[name]), name
    return True


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def one_zone(shape):
    """One zone over everything: the hot row."""
    return np.full(shape, max(1, shape[0] * shape[1] // 2), U32)


def own_zones(shape, seed=0):
    """Every cell its own zone, the ids a random permutation of 1 ... H * W."""
    n = shape[0] * shape[1]
    return (np.random.default_rng(seed).permutation(n).astype(U32) + U32(1)).reshape(shape)


def salt_and_pepper(shape, seed=0):
    """Eight zones (fewer on a raster with fewer cells), a random one at every cell."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    ids = rng.choice(np.arange(1, n + 1), min(8, n), replace=False).astype(U32)
    return ids[rng.integers(0, ids.size, shape)]


def blobs(shape, seed=0):
    """Random rectangles of 7 x 9 cells, a third of the cells 0."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    coarse = rng.integers(1, n + 1, ((shape[0] + 6) // 7, (shape[1] + 8) // 9))
    zones = np.repeat(np.repeat(coarse, 7, 0), 9, 1)[:shape[0], :shape[1]].astype(U32)
    zones[rng.random(shape) < 1 / 3] = 0
    return np.ascontiguousarray(zones)


def multiples(shape, j, seed=0):
    """Ids that are multiples of 2^j (they collide under a masking hash); ``None`` when the
    raster has no such id."""
    n = shape[0] * shape[1]
    if not n >> j:
        return None
    rng = np.random.default_rng(seed + j)
    return (rng.integers(1, (n >> j) + 1, shape) << j).astype(U32)


def extremes(shape, seed=0):
    """Both the smallest and the largest legal id, and cells without a zone."""
    n = shape[0] * shape[1]
    zones = np.random.default_rng(seed).choice(np.array([0, 1, n], U32), shape)
    zones.flat[0], zones.flat[-1] = n, 1
    return np.ascontiguousarray(zones, U32)


ZONE_KINDS = {"one": one_zone, "own": own_zones, "salt": salt_and_pepper, "blobs": blobs,
              "extremes": extremes, "zeros": lambda shape: np.zeros(shape, U32)}


def float_values(shape, seed=0, scale=100.0):
    """float32 with 5 % NaN, negative numbers, both zeros and a few infinities."""
    rng = np.random.default_rng(seed + 17)
    v = (rng.standard_normal(shape) * scale).astype(np.float32)
    draw = rng.random(shape)
    v[draw < 0.05] = np.nan
    v[(draw >= 0.05) & (draw < 0.08)] = 0.0
    v[(draw >= 0.08) & (draw < 0.11)] = -0.0
    v[(draw >= 0.11) & (draw < 0.12)] = np.inf
    v[(draw >= 0.12) & (draw < 0.13)] = -np.inf
    return v


def distinct_values(shape, seed=0):
    """Distinct multiples of 0.25 without NaN and -0.0: what ``ndimage`` is unambiguous on."""
    n = shape[0] * shape[1]
    v = (np.random.default_rng(seed).permutation(n) - n // 2) * 0.25
    v[v == 0] = 0.0
    return v.astype(np.float32).reshape(shape)


# ---------------------------------------------------------------------------
# the restatement against scipy.ndimage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (65, 63), (129, 200)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["one", "own", "salt", "blobs", "extremes"])
def test_restatement_is_what_ndimage_computes(shape, kind):
    zones, values = ZONE_KINDS[kind](shape), distinct_values(shape, 3)
    table, counters = zonal_np(zones, values, 16)
    ids = table["id"]
    assert np.array_equal(ids, np.unique(zones[zones > 0]))
    assert counters == {"zones": ids.size, "unzoned": int((zones == 0).sum()), "clamped": 0,
                        "over_range": 0}
    width = shape[1]
    assert np.array_equal(table["count"], ndimage.sum(np.ones(shape), zones, ids))
    assert np.array_equal(table["valid"], table["count"])
    assert np.array_equal(table["min"], ndimage.minimum(values, zones, ids))
    assert np.array_equal(table["max"], ndimage.maximum(values, zones, ids))
    for name, where in (("at_min", ndimage.minimum_position), ("at_max", ndimage.maximum_position)):
        assert np.array_equal(table[name], [r * width + c for r, c in where(values, zones, ids)])
    exact = ndimage.sum(values.astype(np.float64), zones, ids)       # quarters: no rounding
    assert np.array_equal(table["sum"] / 2.0 ** 16, exact)
    cells = np.arange(zones.size).reshape(shape)
    assert np.array_equal(table["first"], ndimage.minimum(cells, zones, ids))
    boxes = ndimage.find_objects(zones.astype(np.int64))
    for r, zone in enumerate(ids):
        rows, cols = boxes[zone - 1]
        assert (table["row_min"][r], table["row_max"][r] + 1) == (rows.start, rows.stop)
        assert (table["col_min"][r], table["col_max"][r] + 1) == (cols.start, cols.stop)


def test_restatement_on_a_table_worked_by_hand():
    zones = np.array([[5, 5, 0, 2], [2, 5, 8, 8]], U32)
    nan = np.float32(np.nan)
    values = np.array([[1.5, -0.0, 7.0, nan], [nan, 0.0, 3e9, -3e9]], np.float32)
    table, counters = zonal_np(zones, values, 0)
    assert counters == {"zones": 3, "unzoned": 1, "clamped": 2, "over_range": 0}
    want = {"id": [2, 5, 8], "count": [2, 3, 2], "first": [3, 0, 6], "row_min": [0, 0, 1],
            "row_max": [1, 1, 1], "col_min": [0, 0, 2], "col_max": [3, 1, 3],
            "valid": [0, 3, 2], "at_min": [NO_CELL, 1, 7], "at_max": [NO_CELL, 0, 6],
            "sum": [0, 2, 0]}
    for name, column in want.items():
        assert table[name].tolist() == column, name
    assert same_bits(table["min"], np.array([nan, -0.0, -3e9], np.float32))
    assert same_bits(table["max"], np.array([nan, 1.5, 3e9], np.float32))
    # ties go to the smallest index, for the min and for the max
    tied, _ = zonal_np(np.ones((2, 3), U32), np.array([[4, 1, 9], [9, 1, 4]], np.uint8))
    assert (tied["at_min"][0], tied["at_max"][0], tied["sum"][0]) == (1, 2, 28)
    assert tied["sum"].dtype == U64 and tied["min"].dtype == np.uint8


def test_float_keys_order_as_the_floats_do():
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    keys = key_of(v)
    assert np.all(np.diff(keys.astype(np.int64)) > 0)
    assert same_bits(float_of(keys), v)


# ---------------------------------------------------------------------------
# the Python layer without a device
# ---------------------------------------------------------------------------
def test_mean_is_derived_in_float64_and_nan_without_a_valid_cell():
    table = {"valid": np.array([2, 0, 3], U32), "sum": np.array([3 << 16, 0, -(9 << 15)], np.int64)}
    mean = zonal.with_mean(dict(table), np.float32, 16)["mean"]
    assert mean.dtype == np.float64
    assert mean[0] == 1.5 and np.isnan(mean[1]) and mean[2] == -1.5
    whole = {"valid": np.array([4, 0], U32), "sum": np.array([2 ** 34 + 2, 0], U64)}
    mean = zonal.with_mean(whole, np.uint32, 16)["mean"]
    assert mean[0] == 2.0 ** 32 + 0.5 and np.isnan(mean[1])
    assert "mean" not in zonal.with_mean({"sum": whole["sum"]}, np.uint32, 16)
    assert "mean" not in zonal.with_mean({"valid": whole["valid"]}, np.uint32, 16)


def test_column_types_follow_the_values():
    assert zonal.column_dtype("sum", np.float32) == np.int64
    assert zonal.column_dtype("sum", np.uint8) == np.uint64
    assert zonal.column_dtype("min", np.uint8) == np.uint8
    assert zonal.column_dtype("at_max", np.float32) == np.uint32
    value_type, frac_bits, columns = zonal.zonal_args(np.zeros((2, 3), U32),
                                                      np.zeros((2, 3), np.uint8), ("sum", "id"), 3)
    assert (value_type, frac_bits, columns) == (3, 3, ("id", "sum"))
    assert zonal.zonal_args(np.zeros((2, 3), U32))[2] == zonal.ZONAL_COLUMNS[:7]


ZONES = np.ones((4, 5), U32)


@pytest.mark.parametrize("build, text", [
    (lambda: hd.ZonalStatistics().apply(np.ones((4, 5), np.int32)), "uint32 zone ids"),
    (lambda: hd.ZonalStatistics().apply(np.ones(20, U32)), "2-D raster"),
    (lambda: hd.ZonalStatistics(np.ones((4, 6), np.float32)).apply(ZONES), "the zones"),
    (lambda: hd.ZonalStatistics(np.ones((4, 5), np.float64)), "dtype"),
    (lambda: hd.ZonalStatistics(np.ones(20, np.float32)), "2-D"),
    (lambda: hd.ZonalStatistics([[1.0]]), "NumPy array or a DeviceRaster"),
    (lambda: hd.ZonalStatistics(columns=("count", "area")), "unknown zonal columns"),
    (lambda: hd.ZonalStatistics(columns=("count", "sum")), "needs the values"),
    (lambda: hd.ZonalStatistics(columns=()), "no column wanted"),
    (lambda: hd.ZonalStatistics(np.ones((4, 5), np.float32), frac_bits=31), "frac_bits"),
    (lambda: hd.ZonalStatistics(np.ones((4, 5), np.float32), frac_bits=-1), "frac_bits"),
    (lambda: hd.ZonalStatistics(np.ones((4, 5), np.float32), frac_bits=1.5), "frac_bits"),
    (lambda: hd.ZonalStatistics().broadcast("count"), "no table yet"),
    (lambda: hd.DemToBasins(flats="fill"), "flats"),
    (lambda: hd.DemToBasins(columns=("depth",)), "unknown zonal columns"),
    (lambda: hd.DemToBasins(frac_bits=40), "frac_bits"),
    (lambda: hd.DemToBasins().apply(np.ones((4, 5), np.float64)), "float32"),
])
def test_refusals_that_need_no_device(build, text):
    with pytest.raises(ValueError, match=text):
        build()


def test_a_list_is_no_raster():
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.ZonalStatistics().apply([[1, 2]])
