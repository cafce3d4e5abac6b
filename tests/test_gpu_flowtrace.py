"""
D8 flow trace on the MI355X (``FlowDistance``, ``HeightAboveDrainage``, ``DemToHAND``,
``hdem_flowtrace_u8[_dev]``).  Every comparison is ``np.array_equal`` (``equal_nan`` for the
float rasters): exact answers on constructed paths, the hazards of the tiled scheme with
streams as hand-built cases with written-out answers, agreement with reference (b) of
tests/test_flowtrace.py on random acyclic codes (no streams, a mask, an accumulation with a
threshold), the ``DemToHAND`` chain against the host chain at 4096^2, the local proof at
16384^2, and the error cases.

Value-only mutants of the kernels that were run against this file (all but the two big
rasters), with the tests each fails:
  the crossing step not added to an exit's forest node -> 23 tests, the first
      test_a_row_and_a_column_count_their_steps; every test whose paths leave a tile
  11 doubling rounds in the tile pass -> test_a_spiral, both cases, and nothing else
  the forest schedule cut to two launches -> test_a_row_and_a_column_count_their_steps,
      test_a_snake_through_every_tile, test_a_diagonal_bouncing_between_the_walls and two more
  counts cut to 16 bits in the forest -> test_a_snake_through_every_tile and
      test_a_diagonal_bouncing_between_the_walls, and nothing else
  the final pass always reading the first of the two node arrays -> 17 tests, the first
      test_a_row_and_a_column_count_their_steps
B done in place (one node array for source and destination) was not run: a torn node can
hold a stop's index where a slot number is expected, which is an out-of-bounds read and not a
value-only mutant.  (No tile reads the streams of its halo, so "halo streams ignored" has no
counterpart here.)
"""
import ctypes
import itertools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from test_flowacc import (CODE_OFFSETS, acc_kahn, random_acyclic_codes, receivers,
                          terminal_mask)
from test_flowtrace import distance_of, hand_of, trace_doubling, trace_holds
from test_gpu_flowacc import path_codes, snake, spiral
from test_gpu_watersheds import RANDOM_SHAPES, rim_codes
from test_watersheds import random_seeds

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
ALL = ("stop", "ncard", "ndiag", "distance", "hand")
DTYPES = dict(backend.FT_OUTPUTS)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def trace(codes, streams=None, threshold=None, dem=None, cellsize=1.0, want=None):
    """The host entry point; all outputs that the operands allow unless ``want`` says."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    want = want or (ALL if dem is not None else ALL[:4])
    got, stats = backend.flowtrace(codes, streams, threshold, dem, cellsize, want)
    assert set(got) == set(want)
    for name, raster in got.items():
        assert raster.dtype == DTYPES[name] and raster.shape == codes.shape, name
    return got, stats


def reference(codes, mask=None, dem=None, cellsize=1.0):
    """Reference (b) and the two NumPy formulas."""
    stop, nc, nd = trace_doubling(codes, mask)
    want = {"stop": stop, "ncard": nc, "ndiag": nd,
            "distance": distance_of(stop, nc, nd, cellsize)}
    if dem is not None:
        want["hand"] = hand_of(stop, dem)
    return want


def assert_same(got, want, names=None):
    for name in names or got:
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name], want[name], equal_nan=got[name].dtype.kind == "f"), name


def index1(shape):
    return (np.arange(shape[0] * shape[1], dtype=np.int64) + 1).reshape(shape)


def path_answer(shape, cells, diagonal=False):
    """stop / ncard / ndiag for ``path_codes(shape, cells)`` without streams when all steps
    are of one kind: cell k of the path is len - 1 - k steps from the last, every other cell
    is its own stop."""
    stop = index1(shape)
    steps = np.zeros(shape, np.int64)
    last = stop[cells[-1]]
    ys, xs = np.array(cells).T
    stop[ys, xs] = last
    steps[ys, xs] = np.arange(len(cells) - 1, -1, -1)
    zero = np.zeros(shape, np.int64)
    return {"stop": stop, "ncard": zero if diagonal else steps,
            "ndiag": steps if diagonal else zero}


def assert_path(got, want):
    for name in ("stop", "ncard", "ndiag"):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["distance"],
                          distance_of(got["stop"], got["ncard"], got["ndiag"]))


# ---------------------------------------------------------------------------
# constructed paths: exact answers
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_count_their_steps():
    got, stats = trace(np.full((1, 10000), E, np.uint8), cellsize=30.0)    # 156 crossings
    assert np.array_equal(got["ncard"][0], np.arange(9999, -1, -1))
    assert not got["ndiag"].any() and np.array_equal(got["stop"][0], np.full(10000, 10000))
    assert np.array_equal(got["distance"][0],
                          (np.arange(9999, -1, -1) * 30.0).astype(np.float32))
    assert stats["stops"] == 1 and stats["unreached"] == 0 and stats["exits"] == 156
    got, _ = trace(np.full((10000, 1), S, np.uint8))
    assert np.array_equal(got["ncard"][:, 0], np.arange(9999, -1, -1))
    assert not got["ndiag"].any() and np.array_equal(got["stop"][:, 0], np.full(10000, 10000))


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    assert len(cells) == 4096                            # 4095 steps: the 12-bit field full
    got, _ = trace(path_codes(shape, cells))
    assert_path(got, path_answer(shape, cells))
    assert got["ncard"].max() == 4095


def test_a_snake_through_every_tile():
    cells = snake(512, 512)
    got, stats = trace(path_codes((512, 512), cells))
    assert_path(got, path_answer((512, 512), cells))
    assert got["ncard"][0, 0] == 262143
    assert stats["tile_h"] == 64 and stats["tile_w"] == 64
    assert stats["stops"] == 1 and stats["exits"] == 512 * 7 + 7
    assert stats["forest_rounds"] >= 2


def test_a_diagonal_bouncing_between_the_walls():
    h, w = 70000, 33
    k = np.arange(h)
    x = np.where(k % 64 <= 32, k % 64, 64 - k % 64)
    cells = list(zip(k.tolist(), x.tolist()))
    codes = path_codes((h, w), cells)
    assert set(np.unique(codes)) == {0, SE, SW}
    got, _ = trace(codes, cellsize=30.0)
    want = path_answer((h, w), cells, diagonal=True)
    for name in ("stop", "ncard", "ndiag"):
        assert np.array_equal(got[name], want[name]), name
    assert got["ndiag"][0, 0] == 69999 and not got["ncard"].any()      # more than 16 bits
    assert np.array_equal(got["distance"],
                          distance_of(got["stop"], got["ncard"], got["ndiag"], 30.0))


@pytest.mark.parametrize("anti", [False, True], ids=["SE", "SW"])
def test_a_diagonal_corner_crossing_between_four_tiles(anti):
    n = 128
    cells = [(k, n - 1 - k if anti else k) for k in range(n)]    # (63, 63) -> (64, 64)
    codes = path_codes((n, n), cells)
    codes[cells[-1]] = SW if anti else SE                # the last one points outside
    got, _ = trace(codes)
    assert_path(got, path_answer((n, n), cells, diagonal=True))
    z = np.random.default_rng(1).random((n, n), dtype=np.float32)
    for at in (64, 70):                                  # the corner cell itself; further in
        mask = np.zeros((n, n), np.uint8)
        mask[cells[at]] = 1
        got, stats = trace(codes, mask, dem=z)
        stop = np.zeros((n, n), np.int64)
        nd = np.zeros((n, n), np.int64)
        for j, (y, x) in enumerate(cells):
            stop[y, x] = cells[at][0] * n + cells[at][1] + 1 if j <= at else 0
            nd[y, x] = at - j if j <= at else n - 1 - j  # unreached: to the terminal cell
        assert np.array_equal(got["stop"], stop) and np.array_equal(got["ndiag"], nd)
        assert not got["ncard"].any()
        assert stats["unreached"] == n * n - at - 1
        assert stats["stops"] == n * n - (n - 1) + 1     # every terminal cell and the stream cell
        assert_same(got, reference(codes, mask, z))


def test_codes_pointing_outside_the_raster_are_terminal():
    h, w = 100, 130
    got, _ = trace(np.full((h, w), N, np.uint8))         # row 0 points off the top
    assert np.array_equal(got["stop"], np.repeat(index1((h, w))[:1], h, axis=0))
    assert np.array_equal(got["ncard"], np.repeat(np.arange(h)[:, None], w, axis=1))
    got, _ = trace(np.full((h, w), E, np.uint8))         # last column off the right
    assert np.array_equal(got["stop"], np.repeat(index1((h, w))[:, -1:], w, axis=1))
    assert np.array_equal(got["ncard"], np.repeat(np.arange(w - 1, -1, -1)[None, :], h, axis=0))
    got, _ = trace(np.full((h, w), NE, np.uint8))
    yy, xx = np.indices((h, w))
    assert np.array_equal(got["ndiag"], np.minimum(yy, w - 1 - xx)) and not got["ncard"].any()
    codes = np.zeros((h, w), np.uint8)
    codes[0, :], codes[-1, :], codes[:, 0], codes[:, -1] = N, S, W_, E
    codes[0, 0], codes[0, -1], codes[-1, 0], codes[-1, -1] = NW, NE, SW, SE
    got, stats = trace(codes)
    assert np.array_equal(got["stop"], index1((h, w)))
    assert not got["ncard"].any() and not got["ndiag"].any() and not got["distance"].any()
    assert stats["stops"] == h * w


def border_rotation_codes(h, w, k):
    """Every inner cell steps towards the centre cell (code 0 there), so the inner paths cross
    the tiles and never touch the border; border cell j, counted clockwise from the top left
    corner, holds entry (j + k) % 9 of (0, E, SE, ..., NE).  Over k = 0 ... 8 every border
    cell, the corners included, holds every code once: those that leave the raster, those
    that run along the border, those that point inwards, and 0.  Neighbours on the border
    hold directions 45 degrees apart, never opposite ones: no cycles."""
    yy, xx = np.indices((h, w))
    sy, sx = np.sign(h // 2 - yy), np.sign(w // 2 - xx)
    codes = np.zeros((h, w), np.uint8)
    for code, (dy, dx) in CODE_OFFSETS:
        codes[(sy == dy) & (sx == dx)] = code
    ring = ([(0, x) for x in range(w)] + [(y, w - 1) for y in range(1, h)]
            + [(h - 1, x) for x in range(w - 2, -1, -1)] + [(y, 0) for y in range(h - 2, 0, -1)])
    ys, xs = np.array(ring).T
    table = np.array((0, E, SE, S, SW, W_, NW, N, NE), np.uint8)
    codes[ys, xs] = table[(np.arange(len(ring)) + k) % 9]
    return codes


@pytest.mark.parametrize("k", range(9))
def test_the_three_operators_agree_on_which_cells_are_terminal(k):
    """Flow accumulation, watersheds and the flow trace share one decoder of a cell's code.
    The terminal cells that each of them implies are compared with each other and with
    ``terminal_mask`` on rasters with partial tiles in both axes."""
    h, w = 2 * 64 + 2, 3 * 64 + 5
    codes = border_rotation_codes(h, w, k)
    terminal = terminal_mask(codes)
    assert terminal[0, 0] == (k not in (1, 2, 3)) and terminal[h // 2, w // 2]   # E, SE, S stay
    # flow accumulation: acc = 1 + what the donors bring holds in every cell exactly when the
    # cells whose count enters no other cell's are those without a receiver
    acc = hd.FlowAccumulation().apply(codes)
    rec = receivers(codes)
    inflow = np.zeros(h * w, np.int64)
    np.add.at(inflow, rec[rec >= 0], acc.ravel()[rec >= 0].astype(np.int64))
    assert np.array_equal(acc.ravel(), 1 + inflow)
    assert int(acc[terminal].sum()) == h * w             # every cell ends in one of them
    assert np.array_equal(rec.reshape(h, w) < 0, terminal)
    # watersheds, outlet mode: a terminal cell, and no other, carries its own label
    label = hd.Watersheds().apply(codes)
    assert np.array_equal(label == index1((h, w)), terminal)
    # the flow trace without streams: a terminal cell, and no other, is its own stop
    got, stats = trace(codes)
    own = (got["stop"] == index1((h, w))) & (got["ncard"] + got["ndiag"] == 0)
    assert np.array_equal(own, terminal)
    assert stats["stops"] == int(terminal.sum())


# ---------------------------------------------------------------------------
# the hazards of the tiled scheme with streams, answers written out
# ---------------------------------------------------------------------------
def down(n):
    return list(range(n - 1, -1, -1))


def test_a_stream_on_a_frame_exit_cell_and_on_the_cell_it_drains_into():
    row = np.full((1, 130), E, np.uint8)                 # tiles end at x = 63 and 127
    z = np.arange(130, 0, -1, dtype=np.float32).reshape(1, 130) ** 2
    nan = np.float32(np.nan)
    mask = np.zeros((1, 130), np.uint8)
    mask[0, 63] = 1                                      # the exit cell of tile 0 itself
    got, stats = trace(row, mask, dem=z)
    assert np.array_equal(got["stop"][0], [64] * 64 + [0] * 66)
    assert np.array_equal(got["ncard"][0], down(64) + down(66))
    assert np.array_equal(got["distance"][0], np.array(down(64) + [nan] * 66, np.float32),
                          equal_nan=True)
    assert np.array_equal(got["hand"][0], np.array(list(z[0, :64] - z[0, 63]) + [nan] * 66,
                                                   np.float32), equal_nan=True)
    assert stats["unreached"] == 66 and stats["stops"] == 2
    mask[:] = 0
    mask[0, 64] = 1                                      # the halo cell that exit drains into
    got, _ = trace(row, mask, dem=z)
    assert np.array_equal(got["stop"][0], [65] * 65 + [0] * 65)
    assert np.array_equal(got["ncard"][0], down(65) + down(65))
    assert np.array_equal(got["hand"][0], np.array(list(z[0, :65] - z[0, 64]) + [nan] * 65,
                                                   np.float32), equal_nan=True)
    mask[0, 63] = 1                                      # both
    got, _ = trace(row, mask, dem=z)
    assert np.array_equal(got["stop"][0], [64] * 64 + [65] + [0] * 65)
    assert np.array_equal(got["ncard"][0], down(64) + [0] + down(65))
    col = np.full((130, 1), N, np.uint8)                 # upwards: exits at y = 64 and 128
    mask = np.zeros((130, 1), np.uint8)
    mask[64, 0], mask[127, 0] = 1, 255
    got, _ = trace(col, mask)
    assert np.array_equal(got["stop"][:, 0], [0] * 64 + [65] * 63 + [128] * 3)
    assert np.array_equal(got["ncard"][:, 0], list(range(64)) + list(range(63)) + [0, 1, 2])
    assert not got["ndiag"].any()


def test_two_nested_streams_on_one_path_crossing_four_tiles():
    cells = ([(30, x) for x in range(5, 121)] + [(y, 120) for y in range(31, 101)]
             + [(100, x) for x in range(119, 5, -1)])
    assert len(cells) == 300
    assert {(y // 64, x // 64) for y, x in cells} == {(0, 0), (0, 1), (1, 1), (1, 0)}
    codes = path_codes((128, 128), cells)
    mask = np.zeros((128, 128), bool)
    mask[cells[100]] = mask[cells[250]] = True
    stop = np.zeros((128, 128), np.int64)
    nc = np.zeros((128, 128), np.int64)
    for k, (y, x) in enumerate(cells):
        to = 100 if k <= 100 else 250 if k <= 250 else None
        stop[y, x] = cells[to][0] * 128 + cells[to][1] + 1 if to is not None else 0
        nc[y, x] = (to if to is not None else 299) - k
    got, stats = trace(codes, mask)
    assert np.array_equal(got["stop"], stop) and np.array_equal(got["ncard"], nc)
    assert not got["ndiag"].any()
    assert np.isnan(got["distance"]).sum() == 128 * 128 - 251 == stats["unreached"]
    got, _ = trace(codes)
    assert_path(got, path_answer((128, 128), cells))


def test_a_stream_on_a_terminal_cell_and_a_terminal_cell_that_is_no_stream():
    z = np.linspace(9, 0, 10, dtype=np.float32).reshape(1, 10)
    nan = np.float32(np.nan)
    for last in (E, 0):                                  # pointing outside; code 0
        row = np.full((1, 10), E, np.uint8)
        row[0, 9] = last
        mask = np.zeros((1, 10), np.uint8)
        mask[0, 9] = 1
        got, stats = trace(row, mask, dem=z)
        assert np.array_equal(got["stop"][0], [10] * 10)
        assert np.array_equal(got["ncard"][0], down(10)) and stats["unreached"] == 0
        assert np.array_equal(got["hand"][0], z[0])
        mask[:] = 0
        mask[0, 2] = 1                                   # the terminal cell stays dry
        got, stats = trace(row, mask, dem=z)
        assert np.array_equal(got["stop"][0], [3] * 3 + [0] * 7)
        assert np.array_equal(got["ncard"][0], down(3) + down(7))      # counts to the terminal
        assert not got["ndiag"].any()
        assert np.array_equal(got["distance"][0], np.array([2, 1, 0] + [nan] * 7, np.float32),
                              equal_nan=True)
        assert np.array_equal(got["hand"][0], np.array(list(z[0, :3] - z[0, 2]) + [nan] * 7,
                                                       np.float32), equal_nan=True)
        assert stats["unreached"] == 7 and stats["stops"] == 2


# ---------------------------------------------------------------------------
# random acyclic codes against reference (b)
# ---------------------------------------------------------------------------
def random_dem(shape, seed):
    rng = np.random.default_rng(seed)
    z = (rng.random(shape, dtype=np.float32) * np.float32(1000)).astype(np.float32)
    z[rng.random(shape) < 0.02] = np.nan
    return z


@pytest.mark.parametrize("shape", RANDOM_SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_match_the_doubling_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    z = random_dem(shape, seed=shape[0] + shape[1])
    acc = acc_kahn(codes).astype(np.uint32)
    big = ramp and codes.size >= 130 * 257
    for cellsize in (1.0, 30.0):
        got, stats = trace(codes, dem=z, cellsize=cellsize)            # no streams
        want = reference(codes, None, z, cellsize)
        assert_same(got, want)
        assert stats["unreached"] == 0 and stats["stops"] == int(terminal_mask(codes).sum())
        assert not np.isnan(got["distance"]).any()
        if big:
            assert want["ncard"].any() and want["ndiag"].any()
        mask = random_seeds(shape, seed=shape[0] * 3 + shape[1], every=50) != 0
        got, stats = trace(codes, mask, dem=z, cellsize=cellsize)      # a bool mask
        want = reference(codes, mask, z, cellsize)
        assert_same(got, want)
        assert stats["unreached"] == int((want["stop"] == 0).sum())
        assert stats["stops"] == int((mask | terminal_mask(codes)).sum())
        if big:
            assert (want["stop"] == 0).any() and (want["stop"] != 0).any()
            assert want["ncard"].any() and want["ndiag"].any()
    for threshold in (1, 10, int(acc.max()) + 1):        # every cell; some; no stream at all
        got, stats = trace(codes, acc, threshold, dem=z)
        want = reference(codes, acc >= threshold, z)
        print(f"{shape} ramp={ramp} T={threshold}: "
              f"{100.0 * np.count_nonzero(want['stop']) / want['stop'].size:.1f} % reached")
        assert_same(got, want)
        assert stats["unreached"] == int((want["stop"] == 0).sum())
        if threshold == 1:
            assert np.array_equal(got["stop"], index1(shape)) and not got["distance"].any()
        elif threshold > acc.max():
            assert not got["stop"].any() and np.isnan(got["hand"]).all()
            free = trace_doubling(codes)
            assert np.array_equal(got["ncard"], free[1]) and np.array_equal(got["ndiag"], free[2])
        elif big:
            assert (want["stop"] == 0).any() and (want["stop"] != 0).any()
            assert want["ncard"].any() and want["ndiag"].any()


def test_the_mask_form_and_the_threshold_form_give_identical_rasters():
    codes = random_acyclic_codes(300, 517, seed=9, ramp=True)
    z = random_dem(codes.shape, seed=4)
    acc = acc_kahn(codes).astype(np.uint32)
    for threshold in (2, 25):
        a, sa = trace(codes, acc, threshold, dem=z, cellsize=30.0)
        b, sb = trace(codes, (acc >= threshold).astype(np.uint8) * 255, dem=z, cellsize=30.0)
        c, _ = trace(codes, acc >= threshold, dem=z, cellsize=30.0)
        assert_same(a, b)
        assert_same(a, c)
        assert sa == sb
        assert_same(a, reference(codes, acc >= threshold, z, 30.0))


# ---------------------------------------------------------------------------
# host and device paths, subsets of the outputs, repeatability, profiling
# ---------------------------------------------------------------------------
def test_host_and_device_paths_are_bit_equal_and_repeatable():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    z = random_dem(codes.shape, seed=8)
    acc = acc_kahn(codes).astype(np.uint32)
    mask = (acc >= 10).astype(np.uint8)
    want = reference(codes, mask, z, 30.0)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(acc, dtype=np.uint32) as dacc, \
            backend.DeviceRaster.from_host(mask, dtype=np.uint8) as dmask, \
            backend.DeviceRaster.from_host(z, dtype=np.float32) as dz:
        for streams, dstreams, threshold in ((acc, dacc, 10), (mask, dmask, None)):
            a, sa = trace(codes, streams, threshold, dem=z, cellsize=30.0)
            b, sb = trace(codes, streams, threshold, dem=z, cellsize=30.0)
            outs, sc = backend.flowtrace_dev(dc, dstreams, threshold, dz, 30.0, ALL)
            c = {}
            for name, raster in outs.items():
                with raster:
                    assert raster.dtype == DTYPES[name]
                    c[name] = raster.to_host()
            assert_same(a, want)
            assert_same(b, a)
            assert_same(c, a)
            assert sa == sb == sc
        # the operators, operands on either side
        for streams, threshold in ((acc, 10), (dacc, 10), (mask, None), (dmask, None),
                                   (mask != 0, None)):
            f = hd.FlowDistance(streams, threshold=threshold, cellsize=30.0)
            assert np.array_equal(f.apply(codes), want["distance"], equal_nan=True)
            with f.apply_device(dc) as dev:
                assert np.array_equal(dev.to_host(), want["distance"], equal_nan=True)
            assert f.stats["unreached"] == int((want["stop"] == 0).sum())
            for dem in (z, dz):
                g = hd.HeightAboveDrainage(dem=dem, streams=streams, threshold=threshold)
                assert np.array_equal(g.apply(codes), want["hand"], equal_nan=True)
                assert g.distance is None and g.drainage is None
                with g.apply_device(dc) as dev:
                    assert np.array_equal(dev.to_host(), want["hand"], equal_nan=True)
        g = hd.HeightAboveDrainage(dem=z, streams=dacc, threshold=10, cellsize=30.0,
                                   keep_partial_results=True)
        assert np.array_equal(g.apply(codes), want["hand"], equal_nan=True)
        assert np.array_equal(g.distance, want["distance"], equal_nan=True)
        assert np.array_equal(g.drainage, want["stop"]) and g.drainage.dtype == np.uint32
        with g.apply_device(dc) as dev:
            assert np.array_equal(dev.to_host(), want["hand"], equal_nan=True)
        with g.distance as dd, g.drainage as ds:
            assert np.array_equal(dd.to_host(), want["distance"], equal_nan=True)
            assert np.array_equal(ds.to_host(), want["stop"])
        none = reference(codes, None, None, 1.0)
        assert np.array_equal(hd.FlowDistance().apply(codes), none["distance"])
        chain = hd.ComposedFilter()                      # both members run on the device
        chain.filters = [hd.FlowDistance()]
        with chain.apply_device(dc) as dev:
            assert np.array_equal(dev.to_host(), none["distance"])


def test_every_subset_of_the_outputs_gives_the_same_rasters():
    codes = random_acyclic_codes(257, 130, seed=2, ramp=True)
    z = random_dem(codes.shape, seed=6)
    acc = acc_kahn(codes).astype(np.uint32)
    full, stats = trace(codes, acc, 10, dem=z, cellsize=30.0)
    assert_same(full, reference(codes, acc >= 10, z, 30.0))
    for r in range(1, 5):
        for want in itertools.combinations(ALL, r):
            got, st = trace(codes, acc, 10, dem=z, cellsize=30.0, want=want)
            assert_same(got, full)
            assert st == stats
    got, _ = trace(codes, acc, 10, cellsize=30.0, want=("distance", "stop"))   # no dem at all
    assert_same(got, full)


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    codes = random_acyclic_codes(300, 300, seed=5, ramp=True)
    ctx = backend.context()
    f = hd.FlowDistance()
    f.apply(codes)
    assert f.stats["ms_tile"] == 0 and f.stats["ms_forest"] == 0 and f.stats["ms_final"] == 0
    ctx.profile(True)
    try:
        f.apply(codes)
    finally:
        ctx.profile(False)
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0
    assert "struct_size" not in f.stats


# ---------------------------------------------------------------------------
# the filled synthetic DEMs
# ---------------------------------------------------------------------------
def test_dem_to_hand_on_4096_equals_the_host_chain():
    import oracle  # noqa: F401
    from oracle import c_oracle
    z = hdem_synth.synth_dem(4096, 4096, variant="rough")
    chain = hd.DemToHAND(threshold=1000, epsilon=1e-3, cellsize=30.0,
                         keep_partial_results=True)
    hand = chain.apply(z)
    assert hand.dtype == np.float32
    filled = c_oracle.sinkfill_pflood(z, 1e-3)
    codes = c_oracle.d8(filled)
    acc = acc_kahn(codes).astype(np.uint32)
    stream = acc >= 1000
    want = reference(codes, stream, filled, 30.0)
    reached = want["stop"] != 0
    print(f"streams {100.0 * stream.mean():.2f} %, reached {100.0 * reached.mean():.2f} %, "
          f"longest path {int((want['ncard'] + want['ndiag'])[reached].max())} steps, "
          f"smallest HAND off the streams {want['hand'][reached & ~stream].min():.2e}")
    assert reached.any() and (~reached).any()
    assert np.array_equal(hand, want["hand"], equal_nan=True)
    assert np.array_equal(np.isnan(hand), ~reached)
    assert (hand[reached] >= 0).all() and (hand[reached & ~stream] > 0).all()
    # the kept partial results are the individual operators' outputs
    assert np.array_equal(chain.filled, filled) and np.array_equal(chain.codes, codes)
    assert np.array_equal(chain.accumulation, acc)
    assert np.array_equal(chain.distance, want["distance"], equal_nan=True)
    assert np.array_equal(chain.filled, hd.SinkFill(epsilon=1e-3).apply(z))
    assert np.array_equal(chain.accumulation, hd.FlowAccumulation().apply(chain.codes))
    assert np.array_equal(
        chain.distance,
        hd.FlowDistance(chain.accumulation, threshold=1000, cellsize=30.0).apply(chain.codes),
        equal_nan=True)
    assert np.array_equal(
        hand, hd.HeightAboveDrainage(dem=chain.filled, streams=chain.accumulation,
                                     threshold=1000).apply(chain.codes), equal_nan=True)
    assert set(chain.stats) == {"SinkFill", "FlowAccumulation", "HeightAboveDrainage"}
    assert chain.stats["HeightAboveDrainage"]["unreached"] == int((~reached).sum())
    plain = hd.DemToHAND(threshold=1000)
    assert np.array_equal(plain.apply(z), hand, equal_nan=True)
    assert plain.filled is None and plain.codes is None and plain.distance is None


def test_16384_holds_the_local_proof():
    threshold, cellsize = 10000, 30.0
    z = hdem_synth.synth_dem(16384, 16384)
    with backend.DeviceRaster.from_host(z) as dz:
        del z
        filled, dcodes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    with filled, dcodes:
        dacc, _ = backend.flowacc_dev(dcodes)
        with dacc:
            outs, stats = backend.flowtrace_dev(dcodes, dacc, threshold, filled, cellsize, ALL)
            acc = dacc.to_host()
        got = {}
        for name, raster in outs.items():
            with raster:
                got[name] = raster.to_host()
        codes, dem = dcodes.to_host(), filled.to_host()
    stream = acc >= threshold
    del acc
    assert trace_holds(codes, got["stop"], got["ncard"], got["ndiag"], streams=stream)
    h, w = codes.shape
    unreached = 0
    for r0 in range(0, h, 1024):                         # the float rasters, in row bands
        band = slice(r0, r0 + 1024)
        stop, nc, nd = got["stop"][band], got["ncard"][band], got["ndiag"][band]
        assert np.array_equal(got["distance"][band], distance_of(stop, nc, nd, cellsize),
                              equal_nan=True)
        at = np.maximum(stop.astype(np.int64) - 1, 0)
        hand = dem[band] - dem.ravel()[at]
        hand[stop == 0] = np.nan
        assert np.array_equal(got["hand"][band], hand, equal_nan=True)
        own = np.arange(r0 * w, (r0 + stop.shape[0]) * w, dtype=np.int64).reshape(stop.shape) + 1
        assert np.array_equal(stop == own, stream[band])
        unreached += int((stop == 0).sum())
    assert 0 < unreached < h * w and stats["unreached"] == unreached
    dry = terminal_mask_banded(codes) & ~stream
    assert stats["stops"] == int(stream.sum()) + int(dry.sum())
    assert stats["exits"] > 0 and stats["forest_rounds"] >= 2


def terminal_mask_banded(codes, band=1024):
    """``terminal_mask`` without the whole raster's int64 index arrays: each band is cut with
    a row of context on either side, so that its own rows see their true neighbours."""
    h = codes.shape[0]
    out = np.zeros(codes.shape, bool)
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        lo, hi = max(0, r0 - 1), min(h, r1 + 1)
        out[r0:r1] = terminal_mask(codes[lo:hi])[r0 - lo:r1 - lo]
    return out


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def good_call():
    got, _ = trace(np.full((3, 5), S, np.uint8))
    assert np.array_equal(got["ncard"][:, 0], [2, 1, 0]) and np.array_equal(got["stop"][:, 0],
                                                                           [11, 11, 11])


def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="cycle: 2 cells never resolve"):
        trace(np.array([[E, W_]], np.uint8))
    good_call()
    with pytest.raises(ValueError, match="cycle: 2 cells never resolve"):
        trace(np.array([[E, W_, 0]], np.uint8), np.array([[0, 0, 1]], np.uint8),
              dem=np.zeros((1, 3), np.float32))
    codes = rim_codes()
    codes[100, 21:100] = W_                              # 79 cells that drain into the loop
    with pytest.raises(ValueError, match="cycle: 875 cells never resolve"):
        trace(codes)
    mask = np.zeros((256, 256), np.uint8)
    mask[0, 0] = 1
    with pytest.raises(ValueError, match="cycle"):       # a stream cell elsewhere does not help
        trace(codes, mask, dem=np.zeros((256, 256), np.float32))
    good_call()
    # a loop that holds a stream cell ends there: legal, and reference (b) agrees
    mask[:] = 0
    mask[10, 150] = 1
    z = random_dem((256, 256), seed=3)
    got, stats = trace(codes, mask, dem=z)
    assert_same(got, reference(codes, mask, z))
    assert (got["stop"] != 0).sum() == 875 and got["ncard"].max() == 795
    assert stats["unreached"] == 256 * 256 - 875


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        trace(codes)
    with pytest.raises(ValueError, match="invalid D8 code"):
        trace(codes, np.ones((50, 70), np.uint8))
    good_call()


def _call(fn, ctx, d8, h, w, streams, kind, threshold, dem, cellsize, outs, flags, st):
    return fn(ctx.handle, d8, h, w, streams, kind, threshold, dem, cellsize, *outs, flags, st)


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_flowtrace_u8_dev, ctx.lib.hdem_flowtrace_u8):
        st = backend.FlowTraceStats()
        rc = _call(fn, ctx, fake, 65536, 65536, None, 0, 0, None, 1.0,
                   [fake, None, None, None, None], 0, ctypes.byref(st))
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
        rc = _call(fn, ctx, fake, 65536, 65536, fake, 2, 5, fake, 1.0, [fake] * 5, 0, None)
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    good_call()


def test_the_c_entry_points_check_their_arguments_and_struct_size():
    ctx = backend.context()
    with backend.DeviceRaster.from_host(np.full((4, 4), E, np.uint8), dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(np.ones((4, 4), np.uint32), dtype=np.uint32) as ds, \
            backend.DeviceRaster.empty((4, 4), np.uint32, ctx) as do, \
            backend.DeviceRaster.empty((4, 4), np.float32, ctx) as df:
        fn = ctx.lib.hdem_flowtrace_u8_dev
        none = [None] * 5

        def call(streams=None, kind=0, threshold=0, dem=None, cellsize=1.0,
                 outs=(do.ptr, None, None, None, None), flags=0, st=None):
            return _call(fn, ctx, dc.ptr, 4, 4, streams, kind, threshold, dem, cellsize, outs,
                         flags, st)
        cases = [
            (dict(outs=none), b"no output"),
            (dict(outs=[None, None, None, None, df.ptr]), b"hand needs the dem"),
            (dict(streams=ds.ptr, kind=2, threshold=0), b"threshold >= 1"),
            (dict(streams=ds.ptr, kind=1, threshold=3), b"no threshold"),
            (dict(streams=None, kind=2, threshold=3), b"null"),
            (dict(streams=None, kind=1), b"null"),
            (dict(streams=ds.ptr, kind=0), b"HDEM_FT_STREAMS_NONE"),
            (dict(kind=0, threshold=2), b"HDEM_FT_STREAMS_NONE"),
            (dict(kind=3), b"unknown stream kind"),
            (dict(cellsize=0.0), b"cellsize"),
            (dict(cellsize=-1.0), b"cellsize"),
            (dict(cellsize=float("nan")), b"cellsize"),
            (dict(cellsize=float("inf")), b"cellsize"),
            (dict(flags=1), b"flags"),
        ]
        for kwargs, text in cases:
            assert call(**kwargs) == backend.BAD_ARG, kwargs
            assert text in ctx.lib.hdem_last_error(), (kwargs, ctx.lib.hdem_last_error())
        st = backend.FlowTraceStats()
        st.struct_size = 0
        assert call(st=ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend.FlowTraceStats()
        st.struct_size = 16                              # an older, shorter struct
        st.unreached, st.exits, st.tile_h = -3, -5, -7
        assert call(st=ctypes.byref(st)) == backend.OK
        assert st.struct_size == 16 and st.stops == 4 and st.forest_rounds == 1
        assert st.unreached == -3 and st.exits == -5 and st.tile_h == -7   # nothing beyond it
        assert np.array_equal(do.to_host(), np.repeat([[4], [8], [12], [16]], 4, axis=1))
        assert call(streams=ds.ptr, kind=2, threshold=1, dem=df.ptr,
                    outs=[do.ptr, None, None, None, None]) == backend.OK
        assert np.array_equal(do.to_host(), np.arange(1, 17).reshape(4, 4))
    good_call()
