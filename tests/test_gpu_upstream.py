"""
Longest upstream D8 flow length on the MI355X (``UpstreamFlowLength``,
``hdem_upstream_u8[_dev]``): exact answers on constructed paths (lines through a thousand
tiles, a snake, spirals, the pair of tributaries whose float32 lengths tie, a comb of
confluences), agreement with the host references of tests/test_upstream.py on random acyclic
codes and on the conditioned synthetic DEMs, the cross-check against ``FlowDistance`` and
``Watersheds``, the device forms, and the refusals (invalid bytes, cycles, cellsize, size).
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, upstream
from test_flowacc import random_acyclic_codes
from test_upstream import length_of, upstream_holds, upstream_kahn

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
ALL = ("ncard", "ndiag", "length")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def up(codes, want=("ncard", "ndiag"), cellsize=1.0):
    outs, _ = upstream.upstream(np.ascontiguousarray(codes, dtype=np.uint8), cellsize, want)
    assert set(outs) == set(want)
    for name in want:
        assert outs[name].dtype == (np.float32 if name == "length" else np.uint32)
    return outs


def same(outs, nc, nd):
    return np.array_equal(outs["ncard"], nc) and np.array_equal(outs["ndiag"], nd)


# the builders of tests/test_gpu_flowacc.py
def path_codes(shape, cells):
    """Codes that send each cell of ``cells`` (a list of (y, x), neighbours in order) to
    the next one; the last is terminal, every other cell is 0."""
    codes = np.zeros(shape, np.uint8)
    by_step = {(0, 1): E, (1, 1): SE, (1, 0): S, (1, -1): SW, (0, -1): W_, (-1, -1): NW,
               (-1, 0): N, (-1, 1): NE}
    for (y, x), (ny, nx) in zip(cells[:-1], cells[1:]):
        codes[y, x] = by_step[(ny - y, nx - x)]
    return codes


def path_answer(shape, cells):
    nc = np.zeros(shape, np.int64)
    for k, (y, x) in enumerate(cells):
        nc[y, x] = k
    return nc


def snake(h, w):
    return [(y, x if y % 2 == 0 else w - 1 - x) for y in range(h) for x in range(w)]


def spiral(y0, x0, n):
    cells, top, left, bottom, right = [], y0, x0, y0 + n - 1, x0 + n - 1
    while top <= bottom and left <= right:
        cells += [(top, x) for x in range(left, right + 1)]
        cells += [(y, right) for y in range(top + 1, bottom + 1)]
        if top < bottom:
            cells += [(bottom, x) for x in range(right - 1, left - 1, -1)]
        if left < right:
            cells += [(y, left) for y in range(bottom - 1, top, -1)]
        top, left, bottom, right = top + 1, left + 1, bottom - 1, right - 1
    return cells


# ---------------------------------------------------------------------------
# 1, 2: lines and constructed paths, exact answers
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_count_their_position_past_65535():
    got = up(np.full((1, 70000), E, np.uint8))              # 1093 tile crossings
    assert np.array_equal(got["ncard"][0], np.arange(70000)) and not got["ndiag"].any()
    got = up(np.full((70000, 1), S, np.uint8))
    assert np.array_equal(got["ncard"][:, 0], np.arange(70000)) and not got["ndiag"].any()


def test_all_east_and_all_south_east():
    got = up(np.full((100, 130), E, np.uint8))
    assert same(got, np.repeat(np.arange(130)[None, :], 100, axis=0), np.zeros((100, 130)))
    got = up(np.full((2500, 2500), SE, np.uint8))
    yy, xx = np.indices((2500, 2500))
    assert same(got, np.zeros((2500, 2500)), np.minimum(yy, xx))


def test_a_snake_through_every_tile():
    cells = snake(512, 512)
    f = hd.UpstreamFlowLength(keep_partial_results=True)
    got = f.apply(path_codes((512, 512), cells))
    want = path_answer((512, 512), cells)
    assert np.array_equal(f.ncard, want) and not f.ndiag.any()
    assert np.array_equal(got, want.astype(np.float32))
    assert f.stats["tile_h"] == 64 and f.stats["tile_w"] == 64
    assert f.stats["max_hops"] >= 63                      # the path crosses every tile
    assert f.stats["heads"] == 512 * 512 - (len(cells) - 1)


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    assert len(cells) == 4096
    got = up(path_codes(shape, cells))
    assert same(got, path_answer(shape, cells), np.zeros(shape))


# ---------------------------------------------------------------------------
# 3: two tributaries whose float32 lengths are equal
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("width,winner", [(8121, (0, 5741)), (8122, (8120, 0))],
                         ids=["diagonal_wins", "trunk_one_longer"])
def test_the_float32_trap(width, winner):
    """8119 cardinal steps against 5741 diagonal ones: 5741 sqrt(2) = 8119.00006, the same
    float32.  The trunk runs E along row 5741 and the diagonal comes down SE; they meet at
    the cell in front of the last two, which flow E."""
    h, meet = 5742, width - 2
    codes = np.zeros((h, width), np.uint8)
    codes[5741, :meet] = E
    dy = np.arange(5741)
    dx = meet - 5741 + dy                          # from (0, meet - 5741) to (5740, meet - 1)
    codes[dy, dx] = SE
    codes[5741, meet] = E
    if width == 8121:
        assert (dx[0], dx[-1]) == (2378, 8118)
        assert np.float32(8119.0) == np.float32(5741 * np.sqrt(2.0))
    got = up(codes)
    nc, nd = got["ncard"], got["ndiag"]
    assert (nc[5741, meet], nd[5741, meet]) == winner
    assert (nc[5741, meet + 1], nd[5741, meet + 1]) == (winner[0] + 1, winner[1])
    xs = np.arange(meet)
    assert np.array_equal(nc[5741, :meet], xs) and not nd[5741, :meet].any()
    assert np.array_equal(nd[dy, dx], dy) and not nc[dy, dx].any()
    assert int(nc.sum(dtype=np.int64)) == int(xs.sum()) + 2 * winner[0] + 1
    assert int(nd.sum(dtype=np.int64)) == int(dy.sum()) + 2 * winner[1]


# ---------------------------------------------------------------------------
# 4: a comb
# ---------------------------------------------------------------------------
def comb_codes():
    """200 x 300: a trunk along the bottom row flowing E over 5 tiles and N -> S tributary
    columns of assorted heights.  Rows 192-199 are the trunk's tile row, so the columns taller
    than 7 start in a tile row above and cross a horizontal seam (the one at x = 150 starts
    at the top of the raster and crosses three).  At x = 100 the trunk meets a column of 110
    cardinal steps and, from the NW, a diagonal of 90 steps: 127.3 long, fewer steps and
    worth more."""
    h, w = 200, 300
    codes = np.zeros((h, w), np.uint8)
    codes[h - 1, :w - 1] = E
    heights = {5: 3, 20: 25, 40: 10, 64: 30, 70: 1, 100: 110, 150: 199, 200: 7, 256: 190,
               290: 60}
    for x, height in heights.items():
        codes[h - 1 - height:h - 1, x] = S
    k = np.arange(1, 91)
    codes[h - 1 - k, 100 - k] = SE                         # 90 diagonal steps into (199, 100)
    return codes


def test_a_comb_of_confluences():
    codes = comb_codes()
    nc, nd = upstream_kahn(codes)
    trunk = list(zip(nc[199].tolist(), nd[199].tolist()))
    assert trunk[5] == (5, 0)                              # the trunk beats 3 steps
    assert trunk[20] == (25, 0) and trunk[40] == (45, 0)   # the tributary wins, then the trunk
    assert trunk[99] == (104, 0)
    assert trunk[100] == (0, 90)                           # 127.3 beats 105 and 110
    assert trunk[149] == (49, 90) and trunk[150] == (199, 0)   # 199 beats 50 + 127.3
    assert trunk[256] == (305, 0) and trunk[299] == (348, 0)
    got = up(codes)
    assert same(got, nc, nd)


# ---------------------------------------------------------------------------
# 5: random acyclic codes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (63, 63), (64, 64), (65, 65),
                                   (127, 129), (7, 1000), (1000, 7), (4097, 300)])
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_match_the_kahn_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    nc, nd = upstream_kahn(codes)
    got = up(codes, ALL, cellsize=30.0)
    assert same(got, nc, nd)
    assert np.array_equal(got["length"], length_of(nc, nd, 30.0))
    for name in ALL:                                       # one output, the others NULL
        alone = up(codes, (name,), cellsize=30.0)
        assert np.array_equal(alone[name], got[name])


# ---------------------------------------------------------------------------
# 6: real codes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conditioned_1024():
    """{variant: (codes, (ncard, ndiag) of upstream_kahn)} of the 1024^2 synthetic DEM."""
    z = hdem_synth.synth_dem(1024, 1024)
    made = {}
    for name, kwargs in (("epsilon", {"epsilon": 1e-3}),
                         ("resolve", {"epsilon": 0.0, "flats": "resolve"})):
        codes = hd.HydroConditioning(**kwargs).apply(z)
        made[name] = (codes, upstream_kahn(codes))
    return made


@pytest.mark.parametrize("variant", ["epsilon", "resolve"])
def test_conditioned_1024_matches_the_kahn_reference(conditioned_1024, variant):
    codes, (nc, nd) = conditioned_1024[variant]
    got = up(codes)
    assert same(got, nc, nd)
    assert upstream_holds(codes, got["ncard"], got["ndiag"])


def test_conditioned_2048_satisfies_the_local_equation():
    codes = hd.HydroConditioning(epsilon=1e-3).apply(hdem_synth.synth_dem(2048, 2048))
    got = up(codes)
    assert upstream_holds(codes, got["ncard"], got["ndiag"])
    assert got["ncard"].max() > 64                         # paths that leave their tile


def test_the_longest_path_of_a_basin_ends_at_its_outlet(conditioned_1024):
    """Over every basin of ``Watersheds``, the greatest ``FlowDistance`` to the outlet is
    ``up(outlet)``: the same path seen from its two ends.  At this size near-ties of the
    float64 key differ by >= 3e-7 against an ulp of 1e-10, so its argmax is safe."""
    codes, (nc, nd) = conditioned_1024["epsilon"]
    labels = hd.Watersheds().apply(codes)                  # 1 + flat index of the outlet
    down, _ = backend.flowtrace(codes, want=("ncard", "ndiag"))
    dc, dd = down["ncard"].ravel().astype(np.int64), down["ndiag"].ravel().astype(np.int64)
    key = dc + dd * np.sqrt(2.0)
    basin = labels.ravel().astype(np.int64) - 1
    order = np.lexsort((key, basin))                       # by basin, then by key
    last = np.r_[np.flatnonzero(np.diff(basin[order])), order.size - 1]
    outlet, farthest = basin[order][last], order[last]
    assert outlet.size == np.unique(basin).size > 10
    uc, ud = nc.ravel()[outlet], nd.ravel()[outlet]
    assert np.array_equal(uc + ud * np.sqrt(2.0), key[farthest])
    assert np.array_equal(uc, dc[farthest]) and np.array_equal(ud, dd[farthest])
    got = up(codes)
    assert np.array_equal(got["ncard"].ravel()[outlet], dc[farthest])
    assert np.array_equal(got["ndiag"].ravel()[outlet], dd[farthest])


# ---------------------------------------------------------------------------
# 7: device forms
# ---------------------------------------------------------------------------
def test_host_and_device_forms_are_bit_equal_and_repeatable():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    f = hd.UpstreamFlowLength(cellsize=30.0, keep_partial_results=True)
    a = f.apply(codes)
    assert isinstance(f.ncard, np.ndarray) and isinstance(f.ndiag, np.ndarray)
    a_c, a_d = f.ncard, f.ndiag
    b = f.apply(codes)
    assert np.array_equal(a, b) and np.array_equal(a_c, f.ncard) and np.array_equal(a_d, f.ndiag)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        dev = f.apply_device(dc)
        with dev, f.ncard, f.ndiag:
            assert all(backend.is_device_raster(r) for r in (dev, f.ncard, f.ndiag))
            assert dev.dtype == np.float32 and f.ncard.dtype == f.ndiag.dtype == np.uint32
            c, c_c, c_d = dev.to_host(), f.ncard.to_host(), f.ndiag.to_host()
        g = hd.UpstreamFlowLength(cellsize=30.0)
        with g.apply_device(dc) as dev:
            assert g.ncard is None and g.ndiag is None
            assert np.array_equal(dev.to_host(), a)
    assert a.dtype == c.dtype == np.float32
    assert np.array_equal(a, c) and np.array_equal(a_c, c_c) and np.array_equal(a_d, c_d)
    assert np.array_equal(a, length_of(a_c, a_d, 30.0))
    assert f.stats["heads"] == int(((a_c == 0) & (a_d == 0)).sum())


def test_the_chain_from_a_dem_stays_on_the_device():
    z = hdem_synth.synth_dem(300, 400)
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(epsilon=1e-3), hd.D8FlowDirection(), hd.UpstreamFlowLength()]
    with backend.DeviceRaster.from_host(z) as dz:
        with chain.apply_device(dz) as out:
            assert backend.is_device_raster(out) and out.dtype == np.float32
            got = out.to_host()
    codes = hd.D8FlowDirection().apply(hd.SinkFill(epsilon=1e-3).apply(z))
    want = hd.UpstreamFlowLength().apply(codes)
    assert np.array_equal(got, want)
    assert np.array_equal(chain.apply(z), want)
    assert np.array_equal(want, length_of(*upstream_kahn(codes)))


def test_profiling_times_the_phases():
    ctx = backend.context()
    ctx.profile(True)
    try:
        f = hd.UpstreamFlowLength()
        f.apply(random_acyclic_codes(300, 300, seed=5, ramp=True))
    finally:
        ctx.profile(False)
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0
    f.apply(np.full((3, 5), S, np.uint8))
    assert f.stats["ms_tile"] == 0 and f.stats["exits"] == 0


# ---------------------------------------------------------------------------
# 8: refusals: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def still_works():
    got = up(np.full((3, 5), S, np.uint8))
    assert np.array_equal(got["ncard"][:, 0], [0, 1, 2]) and not got["ndiag"].any()


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        up(codes)
    still_works()


def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="flow directions form a cycle: 2 cells never drain"):
        up(np.array([[E, W_]], np.uint8))
    codes = np.zeros((200, 200), np.uint8)               # clockwise round a 50 x 50 rim
    y0, x0, n = 40, 40, 50                               # that lies in four tiles
    codes[y0, x0:x0 + n - 1] = E
    codes[y0:y0 + n - 1, x0 + n - 1] = S
    codes[y0 + n - 1, x0 + 1:x0 + n] = W_
    codes[y0 + 1:y0 + n, x0] = N
    assert int((codes != 0).sum()) == 196
    codes[y0 + 20, :x0] = E                              # tributaries that drain into it,
    codes[:y0, x0 + 30] = S
    codes[y0 + 35, x0 + n:] = W_                         # across a vertical seam
    codes[y0 + n:, x0 + 10] = N                          # and across a horizontal one
    # a stretch of the ring completes inside its tile, from the cell whose donor lies in the
    # tile before: what never drains is counted where it is stuck, at the four tile crossings
    with pytest.raises(ValueError, match="flow directions form a cycle: 4 cells never drain"):
        up(codes)
    still_works()


def test_a_bad_cellsize_and_a_short_struct_are_refused_by_the_library():
    ctx = backend.context()
    lib = ctx.lib
    codes = np.full((4, 6), E, np.uint8)
    out = np.zeros((4, 6), np.uint32)
    st = backend._UpstreamStats()                   # pylint: disable=protected-access
    args = (ctx.handle, codes.ctypes.data, 4, 6)
    for cellsize in (0.0, -1.0, float("nan"), float("inf")):
        rc = lib.hdem_upstream_u8(*args, cellsize, out.ctypes.data, None, None, 0,
                                  ctypes.byref(st))
        assert rc == backend.BAD_ARG and b"cellsize" in lib.hdem_last_error()
    assert lib.hdem_upstream_u8(*args, 1.0, None, None, None, 0, None) == backend.BAD_ARG
    assert b"no output wanted" in lib.hdem_last_error()
    assert lib.hdem_upstream_u8(*args, 1.0, out.ctypes.data, None, None, 1, None) == \
        backend.BAD_ARG
    assert b"flags" in lib.hdem_last_error()
    st.struct_size = 3
    assert lib.hdem_upstream_u8(*args, 1.0, out.ctypes.data, None, None, 0,
                                ctypes.byref(st)) == backend.BAD_ARG
    assert b"hdem_upstream_stats.struct_size is 3" in lib.hdem_last_error()
    # a shorter struct of an earlier version is filled as far as it goes
    st = backend._UpstreamStats()                   # pylint: disable=protected-access
    st.struct_size, st.tile_h = 24, -7
    assert lib.hdem_upstream_u8(*args, 1.0, out.ctypes.data, None, None, 0,
                                ctypes.byref(st)) == backend.OK
    assert st.struct_size == 24 and st.heads == 4 and st.tile_h == -7
    assert np.array_equal(out, np.repeat(np.arange(6)[None, :], 4, axis=0))
    with pytest.raises(ValueError, match="cellsize must be finite and positive"):
        upstream.upstream(codes, 0)
    still_works()


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_upstream_u8_dev, ctx.lib.hdem_upstream_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, 1.0, fake, fake, fake, 0, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    still_works()
