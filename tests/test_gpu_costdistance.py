"""
Cost distance, back link and allocation on the MI355X (``CostDistance``, ``CostAllocation``,
``CostPath``, ``hdem_costdistance_f32``).

The definition and the host reference are those of tests/test_costdistance.py.  Every comparison
is byte equality, of every output and of every count that no schedule changes: the operator works
in integers after one rounding per cell.

The operator is one C symbol that takes host or device pointers by a flag, so the table of
tests/device_cases.py does not list it; this file supplies that coverage itself: both forms,
poisoned scratch and output memory, and a caller's stream behind an unfinished producer, on a
second context (with the machinery of tests/test_gpu_scribble.py and tests/test_gpu_streams.py).

A float32 cost has 24 significant bits, so the largest quantised cost an input can reach is
2^28 - 16, not 2^28 - 1; the 64-bit tests use it, and 2^28 itself (4096.0 at frac_bits 16) for
the refusal above the bound.
"""
import ctypes

import numpy as np
import pytest

import hydrodem_amd as hd
import size_regimes as sr
from hydrodem_amd import backend, costdistance as cd
from hydrodem_amd.backend import DeviceRaster
from test_costdistance import (F32, NAN, NAN32, SCHEDULE_FREE, UNREACHED, cost_distance_ref,
                               follow, quantise, random_case, step_weight)
from test_gpu_flowacc import spiral
from test_gpu_scribble import Case, assert_same_bytes, execute
from test_gpu_streams import Delay, on_a_callers_stream

pytestmark = pytest.mark.gpu

SHAPES = [(130, 197), (1, 200), (65, 1), (64, 128), (200, 70)]
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731
ALL = ("units", "distance", "backlink", "nearest")
DIAGONAL = (2, 8, 32, 128)
CARDINAL = (1, 4, 16, 64)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def same_bytes(got, want, what=""):
    assert got.keys() == want.keys(), what
    for name, w in want.items():
        g = got[name]
        assert (g.dtype, g.shape) == (w.dtype, w.shape), f"{what} {name}"
        gb = g.view(np.uint32) if g.dtype == F32 else g
        wb = w.view(np.uint32) if w.dtype == F32 else w
        differ = np.argwhere(gb != wb)
        assert not len(differ), (what, name, len(differ),
                                 [(tuple(c), g[tuple(c)], w[tuple(c)]) for c in differ[:5]])


def source_tiles(cost, sources, threshold=None):
    """The 64 x 64 tiles that hold a source which is no barrier."""
    if sources.dtype == np.uint8 or threshold is None:
        src = sources != 0
    else:
        src = sources >= threshold
    ys, xs = np.nonzero(src & ~np.isnan(cost))
    return len(set(zip((ys // 64).tolist(), (xs // 64).tolist())))


def assert_matches(cost, sources, threshold=None, frac_bits=16, cellsize=1.0, max_units=None):
    """The host form with every output against the reference: the bytes and the counts that no
    schedule changes."""
    want, want_stats = cost_distance_ref(cost, sources, threshold, frac_bits, cellsize,
                                         max_units or 0)
    names = ALL + (("label",) if "label" in want else ())
    got, stats = cd.costdistance(cost, sources, threshold, names, cellsize, frac_bits,
                                 max_units=max_units)
    same_bytes(got, want)
    assert {k: stats[k] for k in SCHEDULE_FREE} == want_stats
    assert stats["tile_h"] == stats["tile_w"] == 64
    if want_stats["sources"]:
        assert stats["rounds"] >= 1
        assert stats["tile_visits"] >= source_tiles(cost, sources, threshold)
    return got, stats, want_stats


# ---------------------------------------------------------------------------
# random rasters of every tile geometry, the three kinds of sources
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", ["mask", "acc", "labels"])
def test_random_costs_with_barriers(shape, kind):
    # (a) float costs at frac_bits 16
    cost, sources, threshold, frac_bits = random_case(shape, kind, "float")
    assert_matches(cost, sources, threshold, frac_bits, cellsize=30.0)
    # (b) integer costs 1 ... 5 at frac_bits 0: ties, and both kinds of step
    cost, sources, threshold, frac_bits = random_case(shape, kind, "integer")
    got, _, counts = assert_matches(cost, sources, threshold, frac_bits)
    cells = cost.size
    diagonal = int(np.isin(got["backlink"], DIAGONAL).sum())
    cardinal = int(np.isin(got["backlink"], CARDINAL).sum())
    if min(shape) > 1:
        assert counts["tie_cells"] >= 0.05 * cells
        assert diagonal >= 0.2 * cells and cardinal >= 0.2 * cells
    else:
        # one cell wide: one neighbour on either side, so no diagonal link; a tie needs two
        # sources at equal distance, and barriers cut the line into pieces most of which hold no
        # source.  What is left to ask: cardinal links only, at least one, and cells out of reach
        assert diagonal == 0 and cardinal >= 1
        assert counts["unreached"] > 0 and counts["barriers"] > 0


# ---------------------------------------------------------------------------
# long paths across tile seams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles(upright):
    n = 4097
    cost = np.full((5, n), NAN, F32)
    cost[2] = 1
    src = np.zeros((5, n), np.uint8)
    src[2, 0] = 1
    if upright:
        cost, src = np.ascontiguousarray(cost.T), np.ascontiguousarray(src.T)
    got, stats, _ = assert_matches(cost, src)
    far = got["units"][n - 1, 2] if upright else got["units"][2, n - 1]
    assert far == 4096 * 131072 == stats["max_units"]      # 4 096 cardinal steps of 2 * 2^16
    assert stats["rounds"] >= 64 and stats["barriers"] == 4 * n
    assert (got["nearest"][~np.isnan(cost)] == (2 if upright else 2 * n)).all()


def test_a_diagonal_zigzag_along_a_seam():
    steps = 1000
    cost = np.full((steps + 1, 128), NAN, F32)
    rows = np.arange(steps + 1)
    cost[rows, 63 + rows % 2] = 1                           # columns 63 | 64: every step crosses
    src = np.zeros(cost.shape, np.uint8)
    src[0, 63] = 1
    got, stats, _ = assert_matches(cost, src, frac_bits=0)
    assert got["units"][steps, 63] == steps * step_weight(2, True) == 3000
    assert stats["rounds"] >= steps // 64                  # a tile row per round at the least
    assert set(np.unique(got["backlink"])) == {0, 32, 128}


def spiral_corridor(shape, offset):
    """A corridor of cost 1 between barriers: the cells of a 32 x 32 spiral at spacing 2 and
    those between them, 2 047 cells spanning 63 x 63; the source at its first cell."""
    coarse = spiral(0, 0, 32)
    cost = np.full(shape, NAN, F32)
    for (ay, ax), (by, bx) in zip(coarse[:-1], coarse[1:]):
        cost[offset + 2 * ay, offset + 2 * ax] = 1
        cost[offset + ay + by, offset + ax + bx] = 1
    cost[offset + 2 * coarse[-1][0], offset + 2 * coarse[-1][1]] = 1
    assert int((cost == 1).sum()) == 2047
    src = np.zeros(shape, np.uint8)
    src[offset, offset] = 1
    return cost, src


@pytest.mark.parametrize("shape,offset", [((66, 66), 1), ((130, 130), 33)])
def test_a_spiral_corridor_inside_one_tile_and_across_four(shape, offset):
    cost, src = spiral_corridor(shape, offset)
    _, stats, _ = assert_matches(cost, src, frac_bits=0)
    assert stats["max_units"] > 1800 * 2                   # 2 046 steps less one per corner cut
    assert stats["unreached"] == 0
    assert offset == 1 or stats["rounds"] > 1


def test_a_road_that_crosses_one_seam_several_times():
    # expensive ground, and a cheap road that weaves over the seam at column 64: the detour
    # along it is cheaper than the straight line, so the least path crosses the seam five times
    cost = np.full((70, 128), 50, F32)
    road = []
    for leg, y0 in enumerate(range(5, 65, 10)):
        xs = range(58, 71) if leg % 2 == 0 else range(70, 57, -1)
        road += [(y0, x) for x in xs]
        road += [(y, xs[-1]) for y in range(y0 + 1, y0 + 10)]
    road = road[:-9]
    for cell in road:
        cost[cell] = 1
    src = np.zeros(cost.shape, np.uint8)
    src[road[0]] = 1
    got, stats, _ = assert_matches(cost, src, frac_bits=0)
    path = follow(got["backlink"], road[-1])
    crossings = sum((a[1] < 64) != (b[1] < 64) for a, b in zip(path[:-1], path[1:]))
    assert crossings >= 5 and all(cost[c] == 1 for c in path)
    assert stats["rounds"] >= 5


# ---------------------------------------------------------------------------
# 64-bit arithmetic
# ---------------------------------------------------------------------------
def test_the_largest_costs_carry_the_distance_past_32_bits_in_a_few_steps():
    top = 2 ** 28 - 16                                     # the largest q a float32 cost reaches
    assert quantise(np.array([[top]], F32), 0)[0, 0] == top
    rng = np.random.default_rng(11)
    cost = np.where(rng.random((70, 140)) < 0.9, F32(top), rng.integers(1, 6, (70, 140)))
    cost = cost.astype(F32)
    cost[rng.random(cost.shape) < 0.03] = NAN
    src = np.zeros(cost.shape, np.uint8)
    src[3, 5] = src[66, 130] = 1
    got, stats, _ = assert_matches(cost, src, frac_bits=0)
    assert stats["max_units"] > 2 ** 34
    assert (got["units"] >= 2 ** 32).sum() > 0.5 * cost.size
    # frac_bits 12: 65535.996 * 2^12 = 2^28 - 16 too
    cost = np.full((3, 40), np.nextafter(F32(65536), F32(0)), F32)
    src = np.zeros(cost.shape, np.uint8)
    src[1, 0] = 1
    got, _, _ = assert_matches(cost, src, frac_bits=12, cellsize=10.0)
    assert got["units"][1, 39] == 39 * 2 * top > 2 ** 34


def ring(n, top_row, bottom_row):
    """Two ways round a wall from (1, 0) to (1, n - 1): along row 0 and along row 2."""
    cost = np.full((3, n), NAN, F32)
    cost[0], cost[2] = top_row, bottom_row
    cost[1, 0] = cost[1, n - 1] = 2 ** 26
    src = np.zeros((3, n), np.uint8)
    src[1, 0] = 1
    return cost, src


@pytest.mark.parametrize("differ", ["high word", "low word"])
@pytest.mark.parametrize("cheaper", ["top", "bottom"])
def test_competing_paths_whose_sums_differ_in_one_word_only(differ, cheaper):
    n = 140                                                # past one seam, sums past 2^33
    near = np.full(n, 2 ** 26, F32)
    far = near.copy()
    if differ == "high word":
        far[40:72] = 2 ** 27                               # 32 cells, 2 * 2^26 more each: 2^32
    else:
        near[70], far[70] = 2, 3                           # 2 more
    rows = (near, far) if cheaper == "top" else (far, near)
    cost, src = ring(n, *rows)
    arms = []
    for blocked in (2, 0):                                 # each way on its own
        one = cost.copy()
        one[blocked, 1:n - 1] = NAN
        arms.append(int(cost_distance_ref(one, src, frac_bits=0)[0]["units"][1, n - 1]))
    a, b = sorted(arms)
    assert a >= 2 ** 33 and (arms[0] < arms[1]) == (cheaper == "top")
    if differ == "high word":
        assert b - a == 2 ** 32 and a & 0xFFFFFFFF == b & 0xFFFFFFFF
    else:
        assert b - a == 2 and a >> 32 == b >> 32
    got, _, _ = assert_matches(cost, src, frac_bits=0)
    assert got["units"][1, n - 1] == a
    assert got["backlink"][1, n - 1] == (32 if cheaper == "top" else 8)


# ---------------------------------------------------------------------------
# more than 256 tiles: the schedule kernel spans two workgroups
# ---------------------------------------------------------------------------
def test_a_strip_of_more_than_256_tiles():
    shape = (70, 16450)
    assert sr.tiles_of(shape) == 516
    rng = np.random.default_rng(13)
    cost = np.full(shape, NAN, F32)
    cost[61:67] = rng.integers(1, 6, (6, shape[1]))        # a band over the seam at row 64
    cost[61:67][rng.random((6, shape[1])) < 0.03] = NAN
    src = np.zeros(shape, np.uint8)
    src[63, 100::2500] = 1                                 # a front of some twenty tiles each way
    src[65, 16400] = 1                                     # in tile 257 of the second tile row
    cost[src != 0] = 1
    got, stats, counts = assert_matches(cost, src, frac_bits=0)
    assert counts["sources"] >= 7 and stats["rounds"] >= 15
    assert (got["units"][61:67, 16000:] >= 0).any()        # tiles 250 ... 257 and 508 ... 515


# ---------------------------------------------------------------------------
# the operators, the limit, both forms, out=
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def labelled():
    """(cost, labels, frac_bits, reference outputs, reference stats) at 130 x 197, float costs."""
    cost, labels, _, frac_bits = random_case((130, 197), "labels", "float")
    want, stats = cost_distance_ref(cost, labels, None, frac_bits, 30.0)
    return cost, labels, frac_bits, want, stats


def test_the_operators_return_the_reference(labelled):
    cost, labels, _, want, stats = labelled
    for output in ("distance", "units", "backlink"):
        op = hd.CostDistance(labels, output=output, cellsize=30.0)
        same_bytes({output: op.apply(cost)}, {output: want[output]})
        assert {k: op.stats[k] for k in SCHEDULE_FREE} == stats
        with DeviceRaster.from_host(cost, dtype=F32) as dc, op.apply_device(dc) as out:
            same_bytes({output: out.to_host()}, {output: want[output]})
    same_bytes({"label": hd.CostAllocation(labels).apply(cost)}, {"label": want["label"]})
    same_bytes({"nearest": hd.CostAllocation(labels, output="nearest").apply(cost)},
               {"nearest": want["nearest"]})
    mask = (labels != 0)                                   # a bool mask, on the device
    with DeviceRaster.from_host(cost, dtype=F32) as dc, \
            DeviceRaster.from_host(mask.view(np.uint8), dtype=np.uint8) as dm, \
            hd.CostAllocation(dm).apply_device(dc) as out:
        same_bytes({"nearest": out.to_host()}, {"nearest": want["nearest"]})
    same_bytes({"nearest": hd.CostAllocation(mask).apply(cost)}, {"nearest": want["nearest"]})


def test_max_distance_changes_no_byte_of_the_cells_within_it(labelled):
    cost, labels, frac_bits, free, _ = labelled
    scale = cd.units_per_cost(30.0, frac_bits)
    limit = float(np.nanmedian(free["distance"]))
    units = cd.max_units_of(limit, 30.0, frac_bits)
    assert units == int(np.floor(limit / scale))
    cut, stats, counts = assert_matches(cost, labels, None, frac_bits, 30.0, max_units=units)
    inside = (free["units"] >= 0) & (free["units"] <= units)
    assert 0.3 * cost.size < inside.sum() < (free["units"] >= 0).sum()
    for name in free:
        a, b = cut[name][inside], free[name][inside]
        assert np.array_equal(a.view(np.uint32) if a.dtype == F32 else a,
                              b.view(np.uint32) if b.dtype == F32 else b), name
    assert (cut["units"][~inside] == -1).all() and (cut["backlink"][~inside] == 0).all()
    assert (cut["nearest"][~inside] == UNREACHED).all() and (cut["label"][~inside] == 0).all()
    assert (cut["distance"].view(np.uint32)[~inside] == NAN32).all()
    assert counts["max_units"] <= units and stats["unreached"] == counts["unreached"]
    op = hd.CostDistance(labels, cellsize=30.0, max_distance=limit)
    same_bytes({"distance": op.apply(cost)}, {"distance": cut["distance"]})


def test_both_forms_twice_each_give_the_same_bytes_and_a_subset_the_bytes_of_the_whole(labelled):
    cost, labels, frac_bits, want, _ = labelled
    names = ALL + ("label",)
    for _ in range(2):
        got, _ = cd.costdistance(cost, labels, None, names, 30.0, frac_bits)
        same_bytes(got, want, "host")
        with DeviceRaster.from_host(cost, dtype=F32) as dc, \
                DeviceRaster.from_host(labels, dtype=np.uint32) as dl:
            outs, _ = cd.costdistance_dev(dc, dl, None, names, 30.0, frac_bits)
            same_bytes({k: v.to_host() for k, v in outs.items()}, want, "device")
            for raster in outs.values():
                raster.free()
    for subset in (("units",), ("distance",), ("backlink",), ("nearest",), ("label",),
                   ("distance", "label"), ("units", "backlink"), ("backlink", "nearest")):
        got, stats = cd.costdistance(cost, labels, None, subset, 30.0, frac_bits)
        same_bytes(got, {k: want[k] for k in subset}, str(subset))


def test_out_is_the_callers_raster(labelled):
    cost, labels, frac_bits, want, _ = labelled
    ctx = backend.context()
    with DeviceRaster.from_host(cost, dtype=F32) as dc, \
            DeviceRaster.from_host(labels, dtype=np.uint32) as dl, \
            DeviceRaster.empty(cost.shape, np.int64, ctx) as units, \
            DeviceRaster.empty(cost.shape, np.uint32, ctx) as nearest, \
            DeviceRaster.empty(cost.shape, F32, ctx) as wrong:
        outs, _ = cd.costdistance_dev(dc, dl, None, ("units", "nearest", "backlink"), 30.0,
                                      frac_bits, out={"units": units, "nearest": nearest})
        assert outs["units"] is units and outs["nearest"] is nearest
        with outs["backlink"] as codes:
            same_bytes({"units": units.to_host(), "nearest": nearest.to_host(),
                        "backlink": codes.to_host()},
                       {k: want[k] for k in ("units", "nearest", "backlink")})
        with pytest.raises(ValueError, match=r"out\['units'\] is int64, got float32"):
            cd.costdistance_dev(dc, dl, want="units", out={"units": wrong})
        with pytest.raises(ValueError, match="out holds nearest, which is not wanted"):
            cd.costdistance_dev(dc, dl, want="units", out={"nearest": nearest})


# ---------------------------------------------------------------------------
# the back links are D8 codes: the D8 family on least-cost paths
# ---------------------------------------------------------------------------
def test_watersheds_on_the_back_links_is_the_allocation(labelled):
    cost, _, _, want, _ = labelled
    basins = hd.Watersheds().apply(want["backlink"])
    reached = want["units"] >= 0
    assert np.array_equal(basins[reached] - 1, want["nearest"][reached])
    got = hd.CostDistance(labelled[1], output="backlink", cellsize=30.0).apply(cost)
    assert np.array_equal(hd.Watersheds().apply(got)[reached] - 1, want["nearest"][reached])


def test_flow_distance_on_the_back_links_counts_the_steps_of_a_uniform_cost():
    rng = np.random.default_rng(17)
    cost = np.full((130, 197), 3, F32)
    cost[rng.random(cost.shape) < 0.1] = NAN
    src = (rng.random(cost.shape) < 0.001).astype(np.uint8)
    got, _, _ = assert_matches(cost, src, frac_bits=4)
    steps, _ = backend.flowtrace(got["backlink"], src, want=("ncard", "ndiag"))
    s = 2 * 3 * 16
    reached = got["units"] >= 0
    sums = steps["ncard"].astype(np.int64) * s + steps["ndiag"].astype(np.int64) * \
        step_weight(s, True)
    assert reached.sum() > 0.5 * cost.size and np.array_equal(sums[reached], got["units"][reached])


def test_cost_path_is_the_back_links_followed_on_the_host(labelled):
    cost, labels, _, want, _ = labelled
    reached = np.argwhere(want["units"] > 0)
    cells = [tuple(int(v) for v in reached[k]) for k in (0, len(reached) // 3, len(reached) // 2,
                                                         len(reached) - 1)]
    gone = tuple(int(v) for v in np.argwhere(want["units"] < 0)[0])        # marks only itself
    marked = np.zeros(cost.shape, np.uint8)
    for cell in cells + [gone]:
        for step in follow(want["backlink"], cell):
            marked[step] = 1
    assert marked[gone] == 1 and marked.sum() > len(cells) + 1
    assert any(labels[follow(want["backlink"], c)[-1]] != 0 for c in cells)
    got = hd.CostPath(cells + [gone]).apply(want["backlink"])
    assert got.dtype == np.uint8 and np.array_equal(got, marked)
    destinations = np.zeros(cost.shape, bool)
    for cell in cells + [gone]:
        destinations[cell] = True
    assert np.array_equal(hd.CostPath(destinations).apply(want["backlink"]), marked)
    with DeviceRaster.from_host(want["backlink"], dtype=np.uint8) as codes, \
            hd.CostPath(destinations.view(np.uint8)).apply_device(codes) as out:
        assert np.array_equal(out.to_host(), marked)


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off(labelled):
    cost, labels, frac_bits, _, _ = labelled
    ctx = backend.context()
    times = ("ms_classify", "ms_relax", "ms_final", "ms_trace")
    _, stats = cd.costdistance(cost, labels, None, ("distance", "label"), 30.0, frac_bits)
    assert all(stats[k] == 0 for k in times)
    ctx.profile(True)
    try:
        _, stats = cd.costdistance(cost, labels, None, ("distance", "label"), 30.0, frac_bits)
        _, plain = cd.costdistance(cost, labels, None, ("distance",), 30.0, frac_bits)
    finally:
        ctx.profile(False)
    assert all(stats[k] > 0 for k in times)
    assert all(plain[k] > 0 for k in times[:3]) and plain["ms_trace"] == 0      # no trace ran
    assert "struct_size" not in stats and "reserved" not in stats


# ---------------------------------------------------------------------------
# refusals: argument errors that the library returns; the context stays usable
# ---------------------------------------------------------------------------
def test_costs_out_of_range_are_refused_with_their_count(labelled):
    cost, labels, frac_bits, want, _ = labelled
    for n, bad in enumerate((-1.0, 0.0, float("inf"), float("-inf"), 2.0 ** -18, 4096.0), 1):
        broken = cost.copy()
        broken[5:5 + n, 66] = bad
        with pytest.raises(ValueError, match=f"cost out of range in {n} cells: a cost is NaN"):
            hd.CostDistance(labels).apply(broken)
        with DeviceRaster.from_host(broken, dtype=F32) as dc:
            with pytest.raises(ValueError, match=f"cost out of range in {n} cells"):
                hd.CostAllocation(labels).apply_device(dc)
        with pytest.raises(ValueError, match=f"cost out of range in {n} cells"):
            cost_distance_ref(broken, labels)
    got, _ = cd.costdistance(cost, labels, None, ALL, 30.0, frac_bits)      # usable afterwards
    same_bytes(got, {k: want[k] for k in ALL})


def test_the_c_entry_point_checks_its_arguments():
    h, w = 20, 30
    cost, labels, _, frac_bits = random_case((h, w), "labels", "float", seed=4)
    want, want_stats = cost_distance_ref(cost, labels, None, frac_bits)
    ctx = backend.context()
    dev = cd.ON_DEVICE
    n = h * w
    with DeviceRaster.from_host(cost, dtype=F32) as dc, \
            DeviceRaster.from_host(labels, dtype=np.uint32) as dl, \
            DeviceRaster.from_host((labels != 0).view(np.uint8), dtype=np.uint8) as dm, \
            DeviceRaster.empty((h, w), np.int64, ctx) as du, \
            DeviceRaster.empty((h, w), F32, ctx) as dd, \
            DeviceRaster.empty((h, w), np.uint8, ctx) as db, \
            DeviceRaster.empty((h, w), np.uint32, ctx) as dn, \
            DeviceRaster.empty((h, w), np.uint32, ctx) as dlab:
        fn = ctx.lib.hdem_costdistance_f32

        def call(cost=dc.ptr, sources=dl.ptr, kind=3, threshold=0, bits=frac_bits, cellsize=1.0,
                 limit=0, units=du.ptr, distance=dd.ptr, backlink=db.ptr, nearest=dn.ptr,
                 label=dlab.ptr, flags=dev, stats=None):
            return fn(ctx.handle, cost, h, w, sources, kind, threshold, bits, cellsize, limit,
                      units, distance, backlink, nearest, label, flags, stats)

        def refused(text, **kw):
            assert call(**kw) == backend.BAD_ARG
            assert text in ctx.lib.hdem_last_error(), ctx.lib.hdem_last_error()

        assert call() == backend.OK
        same_bytes({"units": du.to_host(), "label": dlab.to_host()},
                   {"units": want["units"], "label": want["label"]})
        refused(b"null raster pointer", cost=None)
        refused(b"null raster pointer", sources=None)
        refused(b"HDEM_FT_STREAMS_NONE is not a kind here", kind=0)
        refused(b"unknown stream kind 4", kind=4, label=None)
        refused(b"unknown stream kind -1", kind=-1, label=None)
        refused(b"a label raster takes no threshold (got 2)", threshold=2)
        refused(b"a uint8 stream mask takes no threshold (got 2)", sources=dm.ptr, kind=1,
                threshold=2, label=None)
        refused(b"needs a threshold >= 1", kind=2, label=None)
        assert call(kind=2, threshold=1, label=None) == backend.OK
        assert np.array_equal(du.to_host(), want["units"])
        assert call(sources=dm.ptr, kind=1, label=None) == backend.OK
        assert np.array_equal(dn.to_host(), want["nearest"])
        for bad in (-1, 17):
            refused(b"frac_bits is 0 ... 16", bits=bad)
        refused(b"max_units is >= 0", limit=-1)
        refused(b"no output wanted", units=None, distance=None, backlink=None, nearest=None,
                label=None)
        refused(b"label needs label sources", kind=2, threshold=1)
        refused(b"label needs label sources", sources=dm.ptr, kind=1)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(b"cellsize must be finite and positive", cellsize=bad)
            assert call(cellsize=bad, distance=None) == backend.OK      # only distance needs it
        for flags in (1, dev | 2, -1):
            refused(b"unknown flags", flags=flags)
        # an output that overlaps an input or another output, by one cell at either end
        refused(b"distance overlaps cost", distance=dc.ptr)
        refused(b"distance overlaps cost", distance=dc.ptr + 4 * (n - 1))
        refused(b"distance overlaps cost", cost=dd.ptr + 4 * (n - 1))
        refused(b"units overlaps sources", units=dl.ptr + 4 * (n - 1))
        refused(b"units overlaps sources", sources=du.ptr + 8 * n - 4)
        refused(b"backlink overlaps sources", sources=dm.ptr, kind=1, label=None,
                backlink=dm.ptr + n - 1)
        refused(b"backlink overlaps units", backlink=du.ptr + 8 * n - 1)
        refused(b"nearest overlaps distance", nearest=dd.ptr + 4 * (n - 1))
        refused(b"label overlaps ", label=dn.ptr - 4 * (n - 1))
        refused(b"label overlaps cost", label=dc.ptr)
        st = backend._CostDistanceStats()                  # pylint: disable=protected-access
        st.struct_size = 0
        refused(b"struct_size", stats=ctypes.byref(st))
        st = backend._CostDistanceStats()                  # pylint: disable=protected-access
        st.struct_size = 32                                # a shorter struct
        st.unreached, st.tile_h = -5, -7
        assert call(stats=ctypes.byref(st)) == backend.OK
        assert st.struct_size == 32
        assert st.sources == want_stats["sources"] and st.barriers == want_stats["barriers"]
        assert st.rounds >= 1 and st.tile_visits >= 1
        assert st.unreached == -5 and st.tile_h == -7      # nothing beyond it is written
        fake = ctypes.c_void_p(256)                        # never dereferenced
        for flags in (0, dev):
            assert fn(ctx.handle, fake, 65536, 65536, fake, 1, 0, 16, 1.0, 0, fake, None, None,
                      None, None, flags, None) == backend.BAD_ARG
            assert b"2^32" in ctx.lib.hdem_last_error()
        assert fn(None, dc.ptr, h, w, dl.ptr, 3, 0, 16, 1.0, 0, du.ptr, None, None, None, None,
                  dev, None) == backend.BAD_ARG
        assert ctx.lib.hdem_last_error() == b"ctx is null"
    # the context is as usable as before
    assert_matches(cost, labels, None, frac_bits)


# ---------------------------------------------------------------------------
# poisoned scratch and output memory, and a caller's stream
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=33):
    cost, labels, _, _ = random_case(shape, "labels", "float", seed=seed)
    return {"cost": cost, "labels": labels}


def poison_run(call, inp):
    """Every output (with the trace, its stop in the caller's nearest), the allocation alone
    (codes and stop in the arena) and the outputs that need no trace, under a limit."""
    dc, dl = call.up(inp["cost"]), call.up(inp["labels"])
    types = dict(cd.OUTPUTS)
    host, stats = {}, {}
    for tag, want, limit in (("all", ALL + ("label",), None), ("label", ("label",), None),
                             ("plain", ("units", "distance", "backlink"), 3000.0)):
        out = {name: call.out(dc.shape, types[name]) for name in want} if call.own else None
        got, st = cd.costdistance_dev(dc, dl, None, want, 30.0, 16, limit, out)
        assert not call.own or all(got[name] is out[name] for name in want)
        host.update({f"{tag}_{name}": call.host(raster) for name, raster in got.items()})
        stats.update({f"{tag}_{k}": st[k] for k in SCHEDULE_FREE})
    return host, stats


def poison_check(inp, got):
    cost, labels = inp["cost"], inp["labels"]
    want, _ = cost_distance_ref(cost, labels, None, 16, 30.0)
    same_bytes({k[4:]: v for k, v in got.items() if k.startswith("all_")}, want)
    same_bytes({"label": got["label_label"]}, {"label": want["label"]})
    units = cd.max_units_of(3000.0, 30.0, 16)
    cut, counts = cost_distance_ref(cost, labels, None, 16, 30.0, units)
    assert 0 < counts["unreached"] < cost.size // 2
    same_bytes({k[6:]: v for k, v in got.items() if k.startswith("plain_")},
               {k: cut[k] for k in ("units", "distance", "backlink")})


POISON_CASE = Case("costdistance", ((130, 197),), poison_inputs, poison_run, poison_check, True,
                   frozenset())


@pytest.fixture(scope="module")
def clean_runs():
    """Inputs and the run on a fresh context's own stream, once per ``own``."""
    runs = {}

    def run(own):
        if own not in runs:
            inputs = POISON_CASE.build((130, 197))
            got, stats = execute(POISON_CASE, inputs, None, own)
            POISON_CASE.check(inputs, got)
            runs[own] = (inputs, got, stats)
        return runs[own]
    return run


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
def test_poisoned_memory_changes_no_byte(clean_runs, own):
    inputs, clean, clean_stats = clean_runs(own)
    for byte in (0x00, 0xA5, 0xFF):
        got, stats = execute(POISON_CASE, inputs, byte, own)
        assert stats == clean_stats
        assert_same_bytes(got, clean, f"costdistance under {byte:#04x}")


@pytest.fixture(scope="module")
def delay():
    return Delay()


def test_a_callers_stream_behind_an_unfinished_producer_changes_no_byte(clean_runs, delay):
    inputs, want, want_stats = clean_runs(False)
    got, stats = on_a_callers_stream(POISON_CASE, inputs, want, False)
    assert_same_bytes(got, want, "costdistance on an idle stream of the caller's")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"costdistance behind the delay, out= {whose}"
        got, stats = on_a_callers_stream(POISON_CASE, inputs, want, own, delay)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
