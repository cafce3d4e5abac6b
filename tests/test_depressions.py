"""
Depression labelling and inventory (``hd.Depressions``, ``hd.DepressionInventory``) without a
GPU: the references the GPU module compares with, checked against each other and against
grids whose answers are written out; the errors raised before the device is touched; the
layout of the C ABI's struct; and who frees which device raster, on the stand-in library of
tests/test_device_ownership.py.

References
    ``reference``       scipy.ndimage.label with the 3 x 3 structure (compact labels are
                        defined as its numbering) and NumPy reductions for the table; volumes
                        are summed as uint64 with ``np.add.at``.
    ``union_find``      an independent plain union-find in loops, for tiny grids.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import hydrodem_amd as hd
from hydrodem_amd import backend
from test_device_ownership import (Row, SHAPE, Tracker, operands, run_row,  # noqa: F401
                                   stand_in)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPERATORS = (hd.Depressions, hd.DepressionInventory)
COLUMNS = ("first", "area", "level", "max_depth", "volume_q20")


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def reference(dem, filled, cellsize=1.0):
    """Compact labels (uint32), K and the table of a dem / filled pair."""
    dem, filled = np.asarray(dem, np.float32), np.asarray(filled, np.float32)
    with np.errstate(invalid="ignore"):
        raised = filled > dem
    lab, count = ndimage.label(raised, structure=np.ones((3, 3)))
    lab = lab.astype(np.uint32)
    cells = np.flatnonzero(lab)
    row = lab.ravel()[cells].astype(np.int64) - 1
    z, w = dem.ravel()[cells], filled.ravel()[cells]
    with np.errstate(invalid="ignore", over="ignore"):
        depth = w - z                                            # one float32 subtraction
        quanta = np.minimum(np.rint(depth.astype(np.float64) * 2.0 ** 20), 2.0 ** 31 - 1)
    table = {"first": np.full(count, 2 ** 32 - 1, np.uint32),
             "area": np.bincount(row, minlength=count).astype(np.uint32),
             "level": np.full(count, np.inf, np.float32),
             "max_depth": np.zeros(count, np.float32),
             "volume_q20": np.zeros(count, np.uint64)}
    np.minimum.at(table["first"], row, cells.astype(np.uint32))
    np.minimum.at(table["level"], row, w)
    np.maximum.at(table["max_depth"], row, depth)
    np.add.at(table["volume_q20"], row, quanta.astype(np.uint64))
    table["volume"] = table["volume_q20"].astype(np.float64) / 2.0 ** 20 * float(cellsize) ** 2
    return lab, count, table


def first_labels(compact, first):
    """The ``labels="first"`` raster of compact labels and their ``first`` column."""
    lookup = np.concatenate([[0], first.astype(np.uint64) + 1]).astype(np.uint32)
    return lookup[compact]


def union_find(raised):
    """Compact labels and K of a bool grid by a plain union-find, cell by cell."""
    h, w = raised.shape
    parent = list(range(h * w))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for y in range(h):
        for x in range(w):
            if not raised[y, x]:
                continue
            for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
                ny, nx = y + dy, x + dx
                if 0 <= ny < h and 0 <= nx < w and raised[ny, nx]:
                    a, b = find(y * w + x), find(ny * w + nx)
                    parent[max(a, b)] = min(a, b)
    labels = np.zeros((h, w), np.uint32)
    number = {}
    for c in range(h * w):                       # scan order: a root is its set's first cell
        if raised.flat[c]:
            labels.flat[c] = number.setdefault(find(c), len(number) + 1)
    return labels, len(number)


def mask_pair(mask):
    """A mask as a dem / filled pair: dem = 0, filled = the mask."""
    mask = np.asarray(mask)
    return np.zeros(mask.shape, np.float32), mask.astype(np.float32)


# a 7 x 9 grid: depression 1 is two pieces that touch only diagonally ((1, 2) - (2, 3)), 2
# lies along the raster's edge, 3 is a single cell, the three cells of 4 touch only diagonally
HAND = np.array([[0, 1, 1, 0, 0, 0, 0, 2, 2],
                 [0, 1, 1, 0, 0, 0, 0, 0, 2],
                 [0, 0, 0, 1, 1, 0, 0, 0, 2],
                 [0, 0, 0, 1, 0, 0, 3, 0, 0],
                 [0, 0, 0, 0, 0, 0, 0, 0, 0],
                 [4, 0, 4, 0, 0, 0, 0, 0, 0],
                 [0, 4, 0, 0, 0, 0, 5, 5, 0]], np.uint32)
HAND_DEM = np.full(HAND.shape, 10.0, np.float32)
HAND_FILLED = HAND_DEM.copy()
HAND_FILLED[HAND == 1] = 12.0                    # 7 cells, 2 m deep
HAND_FILLED[HAND == 2] = 10.5                    # 4 cells, 0.5 m
HAND_FILLED[HAND == 3] = 11.0
HAND_FILLED[HAND == 4] = 10.25                   # 3 cells
HAND_FILLED[HAND == 5] = 13.0
HAND_DEM[0, 1] = 9.0                             # one cell of 1 is 3 m deep
HAND_TABLE = {"first": [1, 7, 33, 45, 60], "area": [7, 4, 1, 3, 2],
              "level": [12.0, 10.5, 11.0, 10.25, 13.0],
              "max_depth": [3.0, 0.5, 1.0, 0.25, 3.0],
              "volume_q20": [15 << 20, 2 << 20, 1 << 20, 3 << 18, 6 << 20]}


def test_the_references_agree_with_the_grid_written_out():
    lab, count, table = reference(HAND_DEM, HAND_FILLED, cellsize=30.0)
    assert count == 5 and np.array_equal(lab, HAND)
    for name in COLUMNS:
        assert np.array_equal(table[name], np.array(HAND_TABLE[name], table[name].dtype)), name
    assert np.array_equal(table["volume"], np.array([15, 2, 1, 0.75, 6]) * 900.0)
    got, k = union_find(HAND_FILLED > HAND_DEM)
    assert k == 5 and np.array_equal(got, HAND)
    want_first = np.where(HAND > 0, np.array([0, 2, 8, 34, 46, 61], np.uint32)[HAND], 0)
    assert np.array_equal(first_labels(lab, table["first"]), want_first)


@pytest.mark.parametrize("seed,density,shape", [(1, 0.41, (40, 50)), (2, 0.5, (33, 17)),
                                                (3, 0.2, (1, 70)), (4, 0.6, (70, 1)),
                                                (5, 0.9, (9, 9)), (6, 0.0, (5, 5))])
def test_the_two_references_agree_on_random_masks(seed, density, shape):
    mask = np.random.default_rng(seed).random(shape) < density
    lab, count, table = reference(*mask_pair(mask))
    got, k = union_find(mask)
    assert k == count and np.array_equal(got, lab)
    assert np.array_equal(lab != 0, mask)
    # ndimage numbers the components in scan order of their first cell
    assert np.all(np.diff(table["first"].astype(np.int64)) > 0)
    assert int(table["area"].sum()) == int(mask.sum())
    assert np.array_equal(table["volume_q20"], table["area"].astype(np.uint64) << np.uint64(20))


def test_nan_is_never_raised_and_depths_saturate_and_round_to_even():
    dem = np.zeros((3, 8), np.float32)
    filled = np.zeros((3, 8), np.float32)
    filled[0, 0], dem[0, 1] = np.nan, np.nan
    filled[0, 1] = 5.0                                           # NaN dem: not raised
    filled[1, 3] = 3000.0                                        # saturates
    filled[1, 5] = np.float32(7.6e-6)                            # 7.97 quanta -> 8
    filled[1, 7] = np.float32(2.5 / 2 ** 20)                     # a tie -> 2
    lab, count, table = reference(dem, filled)
    assert count == 3 and lab[0, 0] == 0 and lab[0, 1] == 0
    assert table["volume_q20"].tolist() == [2 ** 31 - 1, 8, 2]


# ---------------------------------------------------------------------------
# what needs no device
# ---------------------------------------------------------------------------
def test_constructor_and_argument_errors():
    z = np.zeros((4, 5), np.float32)
    for kwargs in (dict(dem=None), dict(dem=[[0.0]]), dict(dem=z.astype(np.float64)),
                   dict(dem=z[0]), dict(dem=z, labels="outlet"),
                   dict(dem=z, labels="first", table=True), dict(dem=z, cellsize=0),
                   dict(dem=z, cellsize="wide"), dict(dem=z, cellsize=np.inf)):
        with pytest.raises(ValueError):
            hd.Depressions(**kwargs)
    with pytest.raises(TypeError):
        hd.Depressions(z)                                        # dem is keyword-only
    for kwargs in (dict(cellsize=-1.0), dict(cellsize=None), dict(epsilon=-1e-3),
                   dict(epsilon=np.nan), dict(epsilon="small"), dict(epsilon=None)):
        with pytest.raises(ValueError):
            hd.DepressionInventory(**kwargs)
    f = hd.Depressions(dem=z, table=True)
    assert f.stats == {} and f.count is None and f.table is None
    # refused before the device is touched (no library call is made on the way)
    for wrong in (z.astype(np.float64), z[:, :4], z[0]):
        with pytest.raises(ValueError):
            f.apply(wrong)
        with pytest.raises(ValueError):
            hd.Depressions(dem=z, labels="first").apply(wrong)
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[0.0]])
    with pytest.raises(ValueError):
        hd.DepressionInventory().apply(z.astype(np.float64))
    labels = np.zeros((4, 5), np.uint32)
    for bad in (dict(labels=labels.astype(np.int32)), dict(labels=labels[:3]),
                dict(count=-1), dict(count=1.5), dict(count=True)):
        args = dict(dem=z, filled=z, labels=labels, count=0)
        args.update(bad)
        with pytest.raises(ValueError):
            backend.depression_table(**args)


def test_the_table_of_no_depression_is_empty_and_needs_no_library_call():
    z = np.zeros((4, 5), np.float32)
    table = backend.depression_table(z, z, np.zeros((4, 5), np.uint32), 0)
    assert sorted(table) == sorted(COLUMNS + ("volume",))
    for name, dtype in backend.DEPR_COLUMNS + (("volume", np.float64),):
        assert table[name].shape == (0,) and table[name].dtype == dtype


def test_the_binding_matches_the_header():
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    assert ctypes.sizeof(backend.DepressionsStats) == 56
    assert "} hdem_depressions_stats;   /* sizeof == 56 */" in header
    value = re.search(r"#define HDEM_DEPR_COMPACT (\d+)", header).group(1)
    assert int(value) == backend.DEPR_COMPACT
    st = backend.DepressionsStats()
    assert st.struct_size == 56
    assert sorted(st.as_dict()) == ["depressions", "ms_final", "ms_seam", "ms_tile",
                                    "raised_cells", "tile_components", "tile_h", "tile_w"]
    body = header[header.index("typedef struct hdem_depressions_stats"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("}")], flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [n for n, _ in backend.DepressionsStats._fields_]
    for name in ("hdem_depressions_f32", "hdem_depression_table_f32"):
        assert backend.SIGNATURES[name] == backend.SIGNATURES[name + "_dev"]


# ---------------------------------------------------------------------------
# who frees what (the stand-in leaves K at 0: that path allocates nothing)
# ---------------------------------------------------------------------------
B = backend


def _op(operator, method, *args):
    return getattr(operator, method)(*args), operator


def _table_dev(o, up, count):
    labels = up(np.zeros(SHAPE, np.uint32))
    return B.depression_table_dev(up(o.dem), up(o.hs), labels, count), None


ROWS = [
    Row("Depressions.apply", "hdem_depressions_f32",
        lambda o, up: _op(hd.Depressions(dem=o.dem, table=True), "apply", o.hs)),
    Row("Depressions.apply[device dem]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.Depressions(dem=up(o.dem), labels="first"), "apply", o.hs)),
    Row("Depressions.apply_device", "hdem_depressions_f32_dev",
        lambda o, up: _op(hd.Depressions(dem=o.dem, table=True), "apply_device", up(o.hs))),
    Row("Depressions.apply_device[device dem]", "hdem_depressions_f32_dev",
        lambda o, up: _op(hd.Depressions(dem=up(o.dem), labels="first"), "apply_device",
                          up(o.hs))),
    Row("DepressionInventory.apply", "hdem_depressions_f32_dev",
        lambda o, up: _op(hd.DepressionInventory(), "apply", o.dem)),
    Row("DepressionInventory.apply[download]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.DepressionInventory(), "apply", o.dem)),
    Row("DepressionInventory.apply_device", "hdem_depressions_f32_dev",
        lambda o, up: _op(hd.DepressionInventory(), "apply_device", up(o.dem))),
    Row("DepressionInventory.apply_device[fill]", "hdem_sinkfill_f32_dev",
        lambda o, up: _op(hd.DepressionInventory(epsilon=1e-3), "apply_device", up(o.dem))),
    Row("ComposedFilter.apply[SinkFill, Depressions]", "hdem_depressions_f32_dev",
        lambda o, up: _op(_chain(o), "apply", o.dem)),
    Row("depressions_dev", "hdem_depressions_f32_dev",
        lambda o, up: (B.depressions_dev(up(o.dem), up(o.hs)), None)),
    Row("depressions_dev[first, out]", "hdem_depressions_f32_dev",
        lambda o, up: (B.depressions_dev(up(o.dem), up(o.hs), compact=False,
                                         out=up.empty(SHAPE, np.uint32)), None)),
    Row("depression_table_dev", "hdem_depression_table_f32_dev",
        lambda o, up: _table_dev(o, up, 7)),
    Row("depression_table_dev[download]", "hdem_memcpy_d2h",
        lambda o, up: _table_dev(o, up, 7)),
]


def _chain(o):
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(), hd.Depressions(dem=o.dem)]
    return chain


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_a_call_frees_what_it_does_not_hand_over(row, stand_in):
    lib, tracker = stand_in
    run_row(row, tracker, False, lambda: lib.live)
    assert not lib.live


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_a_failing_call_frees_everything_it_made(row, stand_in):
    lib, tracker = stand_in
    lib.fail = row.fail
    run_row(row, tracker, True, lambda: lib.live)
    assert row.fail in lib.log and not lib.live


def test_no_depression_allocates_nothing_for_the_table(stand_in):
    lib, tracker = stand_in
    o = operands()
    dem, filled, labels = tracker(o.dem), tracker(o.hs), tracker(np.zeros(SHAPE, np.uint32))
    table = backend.depression_table_dev(dem, filled, labels, 0)
    assert not tracker.made and "hdem_depression_table_f32_dev" not in lib.log
    assert all(len(column) == 0 for column in table.values())
    operator = hd.Depressions(dem=o.dem, table=True)
    with operator.apply_device(filled):
        # (K = 0 on the stand-in) the labels and the uploaded dem, no block for the table
        assert len(tracker.made) == 2 and operator.count == 0
        assert operator.table is not None and len(operator.table["first"]) == 0
    for raster in (dem, filled, labels):
        raster.free()
    assert not lib.live
