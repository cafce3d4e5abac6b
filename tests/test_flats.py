"""
D8 flat resolution (``ResolveFlats``, ``hdem_resolve_flats_u8``): the CPU half.

Definition.  ``dem`` float32 with NaN as nodata, ``codes`` uint8 ESRI D8, "equal" float ``==``.
Drains S: non-NaN cells with ``codes != 0``, on the raster ring, or with a NaN 8-neighbour.
Flat cells F: the other non-NaN cells.  ``dist[c]``, c in F: the length k >= 1 of the shortest
8-connected path c = p0 ... pk with every ``dem[pi] == dem[c]``, p0 ... p(k-1) in F, pk in S;
infinite (0xFFFFFFFF) without one.  ``out[c]``: for c in F with finite dist the code of the
first neighbour in D8 window order with c's elevation and ``dist == dist[c] - 1`` (S counts as
0); ``codes[c]`` for every other cell.  The ``dist`` raster holds 0 outside F.

The host references live here and are used by tests/test_gpu_flats.py:
  (a) ``resolve_flats_bfs``      a frontier breadth-first search from S, level by level;
  (b) ``flat_resolution_holds``  the local property, vectorised, any size: outside F ``dist`` is
                                 0 and ``out`` is ``codes``; in F ``dist`` is 1 + the least
                                 ``dist`` among the equal neighbours (infinite when none is
                                 finite) and ``out`` is the first equal neighbour one step
                                 nearer, 0 where ``dist`` is infinite.  A finite solution of
                                 these equations on a flat is the path length (its least cell
                                 would need a smaller neighbour otherwise), so (b) is a proof.
  (c) ``resolve_flats_walk``     plain loops, cell by cell with a queue -- tiny grids.
No GPU here: the references agree with each other and with hand-written grids, (b) rejects
value mutants, and the operator is importable and rejects what it must without a device.
"""
import collections
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle.hdem_oracle_np import D8_CODES, D8_OFFSETS, d8_flow_direction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFF
E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def shifted(a, dy, dx, fill):
    """``a[y + dy, x + dx]`` at (y, x), ``fill`` where that lies outside."""
    h, w = a.shape
    out = np.full((h, w), fill, dtype=a.dtype)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def drains_and_flats(dem, codes):
    nan = np.isnan(dem)
    ring = np.ones(dem.shape, bool)
    ring[1:-1, 1:-1] = False
    near_nan = np.zeros(dem.shape, bool)
    for dy, dx in D8_OFFSETS:
        near_nan |= shifted(nan, dy, dx, False)
    drains = ~nan & ((codes != 0) | ring | near_nan)
    return drains, ~nan & ~drains


def resolve_flats_bfs(dem, codes):
    """(out, dist) of the definition: level k of the search is the set of flat cells with an
    equal neighbour in level k - 1, level 0 being the drains."""
    dem = np.asarray(dem, np.float32)
    codes = np.asarray(codes, np.uint8)
    drains, flat = drains_and_flats(dem, codes)
    dist = np.where(flat, INF, 0).astype(np.int64)
    frontier, k = drains, 0
    with np.errstate(invalid="ignore"):
        while frontier.any():
            k += 1
            reach = np.zeros(dem.shape, bool)
            for dy, dx in D8_OFFSETS:
                reach |= shifted(frontier, dy, dx, False) & (shifted(dem, dy, dx, np.nan) == dem)
            frontier = reach & flat & (dist == INF)
            dist[frontier] = k
        out = codes.copy()
        todo = flat & (dist != INF)
        for (dy, dx), c in zip(D8_OFFSETS, D8_CODES):
            pick = todo & (shifted(dem, dy, dx, np.nan) == dem) & \
                (shifted(dist, dy, dx, INF) == dist - 1)
            out[pick] = c
            todo &= ~pick
    return out, dist.astype(np.uint32)


def resolve_flats_walk(dem, codes):
    """The same by plain loops and one queue (tiny grids)."""
    dem = np.asarray(dem, np.float32)
    h, w = dem.shape
    drains, flat = drains_and_flats(dem, np.asarray(codes))
    dist = np.where(flat, INF, 0).astype(np.int64)
    queue = collections.deque((y, x) for y in range(h) for x in range(w) if drains[y, x])
    while queue:
        y, x = queue.popleft()
        for dy, dx in D8_OFFSETS:
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and flat[ny, nx] and dist[ny, nx] == INF and \
                    dem[ny, nx] == dem[y, x]:
                dist[ny, nx] = dist[y, x] + 1
                queue.append((ny, nx))
    out = np.array(codes, np.uint8)
    for y in range(h):
        for x in range(w):
            if not flat[y, x] or dist[y, x] == INF:
                continue
            for (dy, dx), c in zip(D8_OFFSETS, D8_CODES):
                n = (y + dy, x + dx)            # a flat cell is interior
                if dem[n] == dem[y, x] and dist[n] == dist[y, x] - 1:
                    out[y, x] = c
                    break
    return out, dist.astype(np.uint32)


def flat_resolution_holds(dem, codes, out, dist):
    """The local property (b) of the module docstring."""
    dem = np.asarray(dem, np.float32)
    codes, out = np.asarray(codes, np.uint8), np.asarray(out, np.uint8)
    dist = np.asarray(dist).astype(np.int64)
    _, flat = drains_and_flats(dem, codes)
    if np.any(dist[~flat] != 0) or np.any(out[~flat] != codes[~flat]):
        return False
    nearest = np.full(dem.shape, INF, np.int64)
    want = np.zeros(dem.shape, np.uint8)
    todo = flat & (dist != INF)
    with np.errstate(invalid="ignore"):
        for (dy, dx), c in zip(D8_OFFSETS, D8_CODES):
            equal = shifted(dem, dy, dx, np.nan) == dem
            nd = shifted(dist, dy, dx, INF)
            nearest = np.where(equal, np.minimum(nearest, nd), nearest)
            pick = todo & equal & (nd == dist - 1)
            want[pick] = c
            todo &= ~pick
    expect = np.where(nearest == INF, INF, nearest + 1)
    return bool(np.all(dist[flat] == expect[flat]) and np.all(out[flat] == want[flat]))


def random_flats(shape, seed):
    """Integer elevations 0 ... 3 with 2 % nodata, not filled, and their D8 codes."""
    rng = np.random.default_rng(seed)
    dem = rng.integers(0, 4, shape).astype(np.float32)
    dem[rng.random(shape) < 0.02] = np.nan
    return dem, d8_flow_direction(dem)


# ---------------------------------------------------------------------------
# the references against hand-written grids and each other
# ---------------------------------------------------------------------------
def walled(rows):
    """``rows`` inside a wall of 9."""
    body = np.asarray(rows, np.float32)
    dem = np.full((body.shape[0] + 2, body.shape[1] + 2), 9, np.float32)
    dem[1:-1, 1:-1] = body
    return dem


def test_a_corridor_counts_up_from_its_drain():
    dem = walled([[9] * 6, [4, 5, 5, 5, 5, 5], [9] * 6])
    codes = d8_flow_direction(dem)
    assert codes[2].tolist() == [0, 0, W_, 0, 0, 0, 0, 0]
    for ref in (resolve_flats_bfs, resolve_flats_walk):
        out, dist = ref(dem, codes)
        assert out[2].tolist() == [0, 0, W_, W_, W_, W_, W_, 0]
        assert dist[2].tolist() == [0, INF, 0, 1, 2, 3, 4, 0]        # the 4 is a pit of one cell
        rest = [0, 1, 3, 4]                              # the walls drain into the corridor
        assert np.array_equal(out[rest], codes[rest]) and not dist[rest].any()
        assert flat_resolution_holds(dem, codes, out, dist)


def test_two_terraces_drain_over_their_own_edges():
    dem = walled([[9] * 8, [6, 6, 6, 6, 5, 5, 5, 4], [9] * 8])
    codes = d8_flow_direction(dem)
    for ref in (resolve_flats_bfs, resolve_flats_walk):
        out, dist = ref(dem, codes)
        assert out[2].tolist() == [0, E, E, E, E, E, E, E, 0, 0]
        assert dist[2].tolist() == [0, 3, 2, 1, 0, 2, 1, 0, INF, 0]


def test_ties_go_to_the_first_neighbour_in_window_order():
    # two drains at distance 1: W comes before E
    dem = walled([[9] * 5, [4, 5, 5, 5, 4], [9] * 5])
    out, dist = resolve_flats_bfs(dem, d8_flow_direction(dem))
    assert out[2].tolist() == [0, 0, W_, W_, E, 0, 0] and dist[2, 3] == 1
    # a diagonal (NE) and a cardinal (E) one step nearer: NE comes first
    dem = walled([[9, 9, 5, 4], [9, 5, 5, 4]])
    codes = d8_flow_direction(dem)
    assert codes[1, 3] == E and codes[2, 3] == E and codes[2, 2] == 0
    out, dist = resolve_flats_bfs(dem, codes)
    assert out[2, 2] == NE and dist[2, 2] == 1
    assert np.array_equal(out, resolve_flats_walk(dem, codes)[0])


def test_the_ring_nodata_and_signed_zero_are_drains_and_equal():
    # a flat raster drains over its ring
    dem = np.full((5, 5), 5, np.float32)
    out, dist = resolve_flats_bfs(dem, np.zeros((5, 5), np.uint8))
    assert dist[1:-1, 1:-1].tolist() == [[1, 1, 1], [1, 2, 1], [1, 1, 1]]
    assert out[1:-1, 1:-1].tolist() == [[NW, NW, NW], [NW, NW, NE], [NW, SW, NE]]
    assert not out[0].any() and not out[:, 0].any()
    # next to nodata: the neighbours of the NaN cell stay 0, theirs point at them
    dem = walled(np.full((5, 5), 5.0))
    dem[3, 3] = np.nan
    out, dist = resolve_flats_bfs(dem, d8_flow_direction(dem))
    assert not out[2:5, 2:5].any() and not dist[2:5, 2:5].any()
    assert dist[1, 1:6].tolist() == [1] * 5 and dist[5, 5] == 1
    assert out[1, 1:6].tolist() == [SE, S, SW, SW, SW] and out[5, 5] == NW
    # -0.0 == 0.0
    dem = walled([[9] * 5, [-1, 0.0, -0.0, 0.0, -0.0], [9] * 5])
    out, dist = resolve_flats_bfs(dem, d8_flow_direction(dem))
    assert dist[2].tolist() == [0, INF, 0, 1, 2, 3, 0] and out[2, 3:6].tolist() == [W_] * 3


def test_a_closed_flat_stays_unresolved():
    dem = walled([[3, 3], [3, 3]])
    codes = d8_flow_direction(dem)
    out, dist = resolve_flats_bfs(dem, codes)
    assert not out.any() and (dist[1:3, 1:3] == INF).all()
    assert flat_resolution_holds(dem, codes, out, dist)


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 7), (3, 3), (17, 23), (40, 9), (64, 65)])
def test_the_references_agree_on_random_rasters(shape):
    dem, codes = random_flats(shape, seed=shape[0] * 1000 + shape[1])
    out, dist = resolve_flats_bfs(dem, codes)
    walk_out, walk_dist = resolve_flats_walk(dem, codes)
    assert np.array_equal(out, walk_out) and np.array_equal(dist, walk_dist)
    assert flat_resolution_holds(dem, codes, out, dist)
    assert np.array_equal(out[codes != 0], codes[codes != 0])


def test_the_local_check_rejects_value_mutants():
    dem, codes = random_flats((40, 50), seed=5)
    out, dist = resolve_flats_bfs(dem, codes)
    assert flat_resolution_holds(dem, codes, out, dist)
    _, flat = drains_and_flats(dem, codes)
    resolved = np.argwhere(flat & (dist != INF))
    assert len(resolved) > 100
    for y, x in resolved[::17]:
        for delta in (-1, 1):                           # one distance off by one
            bad = dist.copy()
            bad[y, x] = int(dist[y, x]) + delta
            assert not flat_resolution_holds(dem, codes, out, bad)
        bad = out.copy()                                 # one code zeroed
        bad[y, x] = 0
        assert not flat_resolution_holds(dem, codes, bad, dist)
    # a later neighbour chosen in a tie
    later = 0
    for y, x in resolved:
        ties = [c for (dy, dx), c in zip(D8_OFFSETS, D8_CODES)
                if dem[y + dy, x + dx] == dem[y, x] and dist[y + dy, x + dx] == dist[y, x] - 1]
        assert ties[0] == out[y, x]
        if len(ties) > 1 and later < 20:
            bad = out.copy()
            bad[y, x] = ties[1]
            assert not flat_resolution_holds(dem, codes, bad, dist)
            later += 1
    assert later == 20
    # a drain given a distance, a drain's code changed, an unresolved cell given a code
    y, x = np.argwhere(codes != 0)[0]
    bad = dist.copy()
    bad[y, x] = 1
    assert not flat_resolution_holds(dem, codes, out, bad)
    bad = out.copy()
    bad[y, x] = 0
    assert not flat_resolution_holds(dem, codes, bad, dist)
    y, x = np.argwhere(flat & (dist == INF))[0]
    bad = out.copy()
    bad[y, x] = E
    assert not flat_resolution_holds(dem, codes, bad, dist)


# ---------------------------------------------------------------------------
# the operator without a device
# ---------------------------------------------------------------------------
def test_the_operator_is_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd.filters import custom_filters
    assert hd.ResolveFlats is custom_filters.ResolveFlats
    assert issubclass(hd.ResolveFlats, hd.Filter) and hd.ResolveFlats.auto_device is True
    f = hd.ResolveFlats(dem=np.zeros((2, 2), np.float32))
    assert f.stats == {} and f.distance is None and f.keep_partial_results is False
    assert hd.HydroConditioning().flats == "keep" and hd.DemToHAND(threshold=5).flats == "keep"
    assert hd.HydroConditioning(flats="resolve").flats == "resolve"
    assert hd.DemToHAND(threshold=5, epsilon=0.0, flats="resolve").flats == "resolve"


def test_the_operator_resolves_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import ResolveFlats
        import hydrodem_amd
        assert ResolveFlats is hydrodem_amd.ResolveFlats
        print("ok")
    """)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr


def test_the_operator_rejects_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    dem = np.zeros((4, 4), np.float32)
    # the dem
    with pytest.raises(TypeError):
        hd.ResolveFlats()                                # pylint: disable=missing-kwoa
    with pytest.raises(ValueError, match="needs the dem"):
        hd.ResolveFlats(dem=None)
    with pytest.raises(ValueError, match="NumPy array or a DeviceRaster"):
        hd.ResolveFlats(dem=[[0.0, 1.0], [1.0, 0.0]])
    with pytest.raises(ValueError, match="float32"):
        hd.ResolveFlats(dem=np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError, match="2-D"):
        hd.ResolveFlats(dem=np.zeros(4, np.float32))
    # the codes
    f = hd.ResolveFlats(dem=dem)
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    with pytest.raises(ValueError, match="uint8"):
        f.apply(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        f.apply(np.zeros((2, 4, 4), np.uint8))
    with pytest.raises(ValueError, match=r"the dem is \(4, 4\), the codes \(3, 4\)"):
        f.apply(np.zeros((3, 4), np.uint8))
    # the backend's own checker
    with pytest.raises(ValueError, match="needs the dem"):
        backend.resolve_flats(np.zeros((4, 4), np.uint8), None)
    with pytest.raises(ValueError, match="NumPy array"):
        backend.resolve_flats([[0]], dem)
    # the chains
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve'"):
        hd.HydroConditioning(flats="bogus")
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve'"):
        hd.DemToHAND(threshold=5, flats="bogus")
    with pytest.raises(ValueError, match="apply_batch does not resolve flats"):
        hd.HydroConditioning(flats="resolve").apply_batch([dem])


def test_the_library_exports_the_entry_points():
    from hydrodem_amd import backend
    for name in ("hdem_resolve_flats_u8", "hdem_resolve_flats_u8_dev"):
        assert name in backend.SIGNATURES
    assert ctypes_size(backend.ResolveFlatsStats) == 64
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "int hdem_resolve_flats_u8(" in header and "int hdem_resolve_flats_u8_dev(" in header
    assert "hdem_flats.hip" in open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile"),
                                    encoding="utf-8").read()


def ctypes_size(struct):
    import ctypes
    return ctypes.sizeof(struct)
