"""
D8 flat resolution on the GPU (``ResolveFlats``, ``hdem_resolve_flats_u8[_dev]``, the
``flats="resolve"`` keyword of ``HydroConditioning`` and ``DemToHAND``).

The definition and the host references are those of tests/test_flats.py.  Every comparison
is ``np.array_equal``.  The input codes are ``oracle.hdem_oracle_np.d8_flow_direction`` of the
raster.  Constructed rasters with their answers written out (corridors over 64 tiles, ties,
terraces, each kind of drain, pits), a spiral corridor of 2 000 steps inside one tile and
across a four-tile corner and a lake round an island against the breadth-first reference,
random rasters of every tile geometry, then the chains on filled 2048^2 DEMs against the
local proof, and the errors.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from oracle.hdem_oracle_np import d8_flow_direction
from test_flats import (INF, drains_and_flats, flat_resolution_holds, random_flats,
                        resolve_flats_bfs, walled)
from test_flowacc import terminal_mask
from test_gpu_flowacc import spiral

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def resolve(dem, codes=None):
    """(out, dist, stats) of the host form."""
    dem = np.ascontiguousarray(dem, dtype=np.float32)
    codes = d8_flow_direction(dem) if codes is None else codes
    op = hd.ResolveFlats(dem=dem, keep_partial_results=True)
    out = op.apply(codes)
    assert out.dtype == np.uint8 and op.distance.dtype == np.uint32
    return out, op.distance, op.stats


def assert_matches_reference(dem, codes=None):
    dem = np.ascontiguousarray(dem, dtype=np.float32)
    codes = d8_flow_direction(dem) if codes is None else codes
    want_out, want_dist = resolve_flats_bfs(dem, codes)
    out, dist, stats = resolve(dem, codes)
    assert np.array_equal(out, want_out)
    assert np.array_equal(dist, want_dist)
    _, flat = drains_and_flats(dem, codes)
    finite = want_dist[want_dist != INF]
    assert stats["flat_cells"] == int(flat.sum())
    assert stats["unresolved"] == int((want_dist == INF).sum())
    assert stats["max_distance"] == (int(finite.max()) if finite.size else 0)
    assert stats["tile_h"] == stats["tile_w"] == 64
    return out, dist, stats


def schedule_free(stats):
    """The stats that do not depend on which tile ran when."""
    return {k: stats[k] for k in ("flat_cells", "unresolved", "max_distance", "active_tiles",
                                  "tile_h", "tile_w")}


# ---------------------------------------------------------------------------
# constructed rasters: answers written out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("upright", [False, True])
@pytest.mark.parametrize("low_first", [True, False])
def test_a_corridor_across_64_tiles(upright, low_first):
    n = 4097
    dem = np.full((5, n), 9, np.float32)
    dem[2, 1:n - 1] = 5
    dem[2, 1 if low_first else n - 2] = 4                # one lower cell behind the end
    want_dist = np.zeros((5, n), np.uint32)
    if low_first:                                        # cell 2 drains into cell 1
        along, want_dist[2, 3:n - 1] = slice(3, n - 1), np.arange(1, n - 3)
        want_dist[2, 1] = INF                            # the lower cell is a pit of its own
    else:
        along, want_dist[2, 1:n - 3] = slice(1, n - 3), np.arange(n - 4, 0, -1)
        want_dist[2, n - 2] = INF
    towards = {(False, True): W_, (False, False): E, (True, True): N, (True, False): S}
    if upright:
        dem, want_dist = np.ascontiguousarray(dem.T), np.ascontiguousarray(want_dist.T)
    codes = d8_flow_direction(dem)
    want_out = codes.copy()
    (want_out.T if upright else want_out)[2, along] = towards[upright, low_first]
    out, dist, stats = resolve(dem, codes)
    assert np.array_equal(out, want_out)
    assert np.array_equal(dist, want_dist)
    assert stats["flat_cells"] == n - 3 and stats["unresolved"] == 1
    assert stats["max_distance"] == n - 4
    assert stats["rounds"] > 1                           # a tile per round at the least
    assert stats["active_tiles"] == 64 and stats["tile_visits"] >= 64


def spiral_corridor(shape, offset):
    """A corridor at 5 with one-cell walls of 9: the cells of a 32 x 32 spiral at spacing 2
    and those between them, 2 047 cells; its first cell at 4."""
    coarse = spiral(0, 0, 32)
    dem = np.full(shape, 9, np.float32)
    for (ay, ax), (by, bx) in zip(coarse[:-1], coarse[1:]):
        dem[offset + 2 * ay, offset + 2 * ax] = 5
        dem[offset + ay + by, offset + ax + bx] = 5
    dem[offset + 2 * coarse[-1][0], offset + 2 * coarse[-1][1]] = 5
    assert int((dem == 5).sum()) == 2047
    dem[offset, offset] = 4
    return dem


@pytest.mark.parametrize("shape,offset", [((66, 66), 1), ((130, 130), 33)])
def test_a_spiral_corridor_inside_one_tile_and_across_four(shape, offset):
    _, _, stats = assert_matches_reference(spiral_corridor(shape, offset))
    assert stats["max_distance"] > 1800                  # 2 045 less a step per corner cut
    assert stats["unresolved"] == 1
    assert offset == 1 or stats["rounds"] > 1


def test_a_lake_round_an_island_that_spans_a_tile_seam():
    dem = np.full((40, 130), 9, np.float32)
    dem[1:39, 1:129] = 5
    dem[1:31, 60:69] = 9                                 # from the top wall down, over column 64
    dem[20, 1] = 4                                       # the outlet, left of the island
    _, dist, stats = assert_matches_reference(dem)
    # behind the island: 26 steps down to (31, 68), 66 under it and up to (21, 2), which
    # drains into the outlet -- the straight line would be 73
    assert dist[5, 75] == 92
    assert stats["unresolved"] == 1


def test_ties_go_to_the_first_neighbour_in_window_order():
    dem = walled([[9] * 5, [4, 5, 5, 5, 4], [9] * 5])
    out, dist, _ = resolve(dem)
    assert out[2].tolist() == [0, 0, W_, W_, E, 0, 0] and dist[2].tolist() == [0, INF, 0, 1, 0, INF, 0]
    dem = walled([[9, 9, 5, 4], [9, 5, 5, 4]])           # NE and E one step nearer: NE first
    out, dist, _ = assert_matches_reference(dem)
    assert out[2, 2] == NE and dist[2, 2] == 1


def test_two_terraces_drain_over_their_own_edges():
    dem = walled([[9] * 8, [6, 6, 6, 6, 5, 5, 5, 4], [9] * 8])
    out, dist, stats = resolve(dem)
    assert out[2].tolist() == [0, E, E, E, E, E, E, E, 0, 0]
    assert dist[2].tolist() == [0, 3, 2, 1, 0, 2, 1, 0, INF, 0]
    assert stats["flat_cells"] == 6 and stats["unresolved"] == 1
    # two lakes side by side across a tile seam, the upper one spilling into the lower
    dem = np.full((30, 140), 9, np.float32)
    dem[1:29, 1:70] = 6
    dem[1:29, 70:139] = 5
    dem[15, 138] = 4
    out, dist, _ = assert_matches_reference(dem)
    assert dist[10, 1] == 68 and dist[10, 69] == 0 and dist[10, 70] == 67


def test_the_ring_nodata_and_signed_zero():
    # a flat raster drains over its ring
    dem = np.full((5, 5), 5, np.float32)
    out, dist, _ = resolve(dem)
    assert dist[1:-1, 1:-1].tolist() == [[1, 1, 1], [1, 2, 1], [1, 1, 1]]
    assert out[1:-1, 1:-1].tolist() == [[NW, NW, NW], [NW, NW, NE], [NW, SW, NE]]
    assert not out[0].any() and not out[-1].any() and not out[:, 0].any() and not out[:, -1].any()
    assert_matches_reference(np.full((70, 131), 5, np.float32))
    # next to a nodata block: its neighbours stay 0, theirs point at them
    dem = walled(np.full((5, 5), 5.0))
    dem[3, 3] = np.nan
    out, dist, stats = resolve(dem)
    assert not out[2:5, 2:5].any() and not dist[2:5, 2:5].any()
    assert dist[1, 1:6].tolist() == [1] * 5 and out[1, 1:6].tolist() == [SE, S, SW, SW, SW]
    assert out[5, 5] == NW and stats["flat_cells"] == 16 and stats["unresolved"] == 0
    dem = np.full((80, 150), 9, np.float32)
    dem[1:79, 1:149] = 5
    dem[60:66, 62:70] = np.nan                           # across the seam at column 64
    out, _, stats = assert_matches_reference(dem)
    assert stats["unresolved"] == 0 and not out[59:67, 61:71].any()
    # -0.0 == 0.0
    dem = walled([[9] * 5, [-1, 0.0, -0.0, 0.0, -0.0], [9] * 5])
    out, dist, _ = resolve(dem)
    assert dist[2].tolist() == [0, INF, 0, 1, 2, 3, 0] and out[2, 3:6].tolist() == [W_] * 3


def test_closed_flats_of_an_unfilled_dem_keep_0():
    dem = walled([[3, 3], [3, 3]])
    out, dist, stats = resolve(dem)
    assert not out.any() and (dist[1:3, 1:3] == INF).all()
    assert stats["unresolved"] == stats["flat_cells"] == 4 and stats["max_distance"] == 0
    dem = np.full((100, 100), 9, np.float32)
    dem[10:90, 10:90] = 2                                # a closed lake over four tiles
    dem[30:40, 30:40] = 7                                # with an island that drains into it
    _, dist, stats = assert_matches_reference(dem)
    assert stats["unresolved"] == 80 * 80 - 100 and (dist[10:90, 10:30] == INF).all()


# ---------------------------------------------------------------------------
# random rasters; host and device forms
# ---------------------------------------------------------------------------
RANDOM_SHAPES = [(1, 1), (1, 2), (3, 3), (63, 63), (64, 64), (65, 65), (130, 257), (257, 130),
                 (3, 4097), (4097, 3)]


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_rasters_match_the_breadth_first_reference(shape):
    dem, codes = random_flats(shape, seed=shape[0] * 5000 + shape[1])
    out, dist, stats = assert_matches_reference(dem, codes)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(dem, dtype=np.float32) as dz:
        # the dem as a host array and as a device raster, with and without the distances
        for operand, keep in ((dz, True), (dem, False)):
            op = hd.ResolveFlats(dem=operand, keep_partial_results=keep)
            with op.apply_device(dc) as dev:
                assert dev.dtype == np.uint8 and np.array_equal(dev.to_host(), out)
            if keep:
                with op.distance as dd:
                    assert dd.dtype == np.uint32 and np.array_equal(dd.to_host(), dist)
            else:
                assert op.distance is None
            assert schedule_free(op.stats) == schedule_free(stats)
        assert np.array_equal(hd.ResolveFlats(dem=dz).apply(codes), out)
        # in place
        same, none, _ = backend.resolve_flats_dev(dc, dz, out=dc)
        assert same is dc and none is None and np.array_equal(dc.to_host(), out)


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    dem, codes = random_flats((300, 300), seed=9)
    ctx = backend.context()
    op = hd.ResolveFlats(dem=dem)
    op.apply(codes)
    assert op.stats["ms_classify"] == 0 and op.stats["ms_relax"] == 0 and op.stats["ms_final"] == 0
    ctx.profile(True)
    try:
        op.apply(codes)
    finally:
        ctx.profile(False)
    assert op.stats["ms_classify"] > 0 and op.stats["ms_relax"] > 0 and op.stats["ms_final"] > 0
    assert "struct_size" not in op.stats


# ---------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,nodata", [("rough", True), ("srtm", False)])
def test_the_exact_fill_with_resolved_flats_on_2048(variant, nodata):
    z = hdem_synth.synth_dem(2048, 2048, variant=variant)
    if nodata:
        z[700:760, 1000:1090] = np.nan
    keep = hd.HydroConditioning(epsilon=0.0)
    codes = keep.apply(z)
    chain = hd.HydroConditioning(epsilon=0.0, flats="resolve")
    out = chain.apply(z)
    filled = chain.filled
    assert np.array_equal(filled, keep.filled, equal_nan=True)
    assert chain.resolve_stats["unresolved"] == 0
    assert chain.resolve_stats["flat_cells"] > 0.3 * z.size
    assert chain.resolve_stats["rounds"] > 1
    # the distances of the same call on the same rasters, and the local proof
    op = hd.ResolveFlats(dem=filled, keep_partial_results=True)
    assert np.array_equal(op.apply(codes), out)
    assert op.stats["max_distance"] == chain.resolve_stats["max_distance"] > 64
    assert flat_resolution_holds(filled, codes, out, op.distance)
    # no cycle, and every cell drains to a ring cell, a nodata cell or a neighbour of one
    acc = hd.FlowAccumulation().apply(out)
    terminal = terminal_mask(out)
    assert int(acc[terminal].sum(dtype=np.int64)) == z.size
    drains, _ = drains_and_flats(filled, np.zeros_like(codes))   # ring and next to nodata
    assert not (terminal & ~(drains | np.isnan(filled))).any()
    assert int(terminal_mask(codes).sum()) > 10 * int(terminal.sum())
    # twice the same bytes
    assert np.array_equal(chain.apply(z), out)


def test_dem_to_hand_with_resolved_flats_equals_the_stages_one_by_one():
    z = hdem_synth.synth_dem(700, 900, variant="srtm")
    chain = hd.DemToHAND(threshold=200, epsilon=0.0, flats="resolve", keep_partial_results=True)
    hand = chain.apply(z)
    filled = hd.SinkFill(epsilon=0.0).apply(z)
    codes = hd.ResolveFlats(dem=filled).apply(hd.D8FlowDirection().apply(filled))
    acc = hd.FlowAccumulation().apply(codes)
    trace = hd.HeightAboveDrainage(dem=filled, streams=acc, threshold=200,
                                   keep_partial_results=True)
    assert np.array_equal(chain.filled, filled)
    assert np.array_equal(chain.codes, codes)
    assert np.array_equal(chain.accumulation, acc)
    assert np.array_equal(hand, trace.apply(codes), equal_nan=True)
    assert np.array_equal(chain.distance, trace.distance, equal_nan=True)
    assert chain.stats["ResolveFlats"]["unresolved"] == 0
    assert set(chain.stats) == {"SinkFill", "ResolveFlats", "FlowAccumulation",
                                "HeightAboveDrainage"}
    # the rivers cross the lakes: far fewer cells end short of a stream than on the kept flats
    plain = hd.DemToHAND(threshold=200, epsilon=0.0).apply(z)
    assert int(np.isnan(hand).sum()) < int(np.isnan(plain).sum()) // 2


def test_the_defaults_are_unchanged():
    z = hdem_synth.synth_dem(300, 500)
    with backend.DeviceRaster.from_host(z, dtype=np.float32) as dz:
        filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=0.0)
        with filled, codes:
            want_filled, want_codes = filled.to_host(), codes.to_host()
        for chain in (hd.HydroConditioning(), hd.HydroConditioning(flats="keep")):
            assert np.array_equal(chain.apply(z), want_codes)
            assert np.array_equal(chain.filled, want_filled) and chain.resolve_stats == {}
        filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
        with filled, codes:
            acc, _ = backend.flowacc_dev(codes)
            with acc:
                outs, _ = backend.flowtrace_dev(codes, acc, 150, filled, 1.0, ("hand",))
                with outs["hand"] as dh:
                    want = dh.to_host()
    for chain in (hd.DemToHAND(threshold=150), hd.DemToHAND(threshold=150, flats="keep")):
        assert np.array_equal(chain.apply(z), want, equal_nan=True)
        assert set(chain.stats) == {"SinkFill", "FlowAccumulation", "HeightAboveDrainage"}
    (a, ca), (b, cb) = hd.HydroConditioning().apply_batch([z, z[:100]])
    assert np.array_equal(ca, want_codes) and np.array_equal(a, want_filled)


# ---------------------------------------------------------------------------
# errors: the context stays usable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    dem = np.full((50, 70), 5, np.float32)
    codes = np.zeros((50, 70), np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        hd.ResolveFlats(dem=dem).apply(codes)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        with pytest.raises(ValueError, match="invalid D8 code in 1 cells: a code is 0 or one of"):
            hd.ResolveFlats(dem=dem).apply_device(dc)
    assert_matches_reference(dem)


def test_an_unknown_flats_keyword_raises():
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve', got 'bogus'"):
        hd.HydroConditioning(flats="bogus")
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve', got 'bogus'"):
        hd.DemToHAND(threshold=10, flats="bogus")
    with pytest.raises(ValueError, match="apply_batch does not resolve flats"):
        hd.HydroConditioning(flats="resolve").apply_batch([np.zeros((4, 4), np.float32)])


def test_the_c_entry_points_check_their_arguments_and_struct_size():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_resolve_flats_u8_dev, ctx.lib.hdem_resolve_flats_u8):
        st = backend.ResolveFlatsStats()
        rc = fn(ctx.handle, fake, fake, 65536, 65536, fake, None, 0, ctypes.byref(st))
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    dem = walled([[9] * 5, [4, 5, 5, 5, 4], [9] * 5])
    codes = d8_flow_direction(dem)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(dem, dtype=np.float32) as dz, \
            backend.DeviceRaster.empty(dem.shape, np.uint8, ctx) as do:
        fn = ctx.lib.hdem_resolve_flats_u8_dev
        call = lambda z, flags, st: fn(                   # noqa: E731
            ctx.handle, dc.ptr, z, 5, 7, do.ptr, None, flags, st)
        assert call(None, 0, None) == backend.BAD_ARG
        assert b"needs the dem" in ctx.lib.hdem_last_error()
        assert call(dz.ptr, 1, None) == backend.BAD_ARG
        assert b"flags" in ctx.lib.hdem_last_error()
        st = backend.ResolveFlatsStats()
        st.struct_size = 0
        assert call(dz.ptr, 0, ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend.ResolveFlatsStats()
        st.struct_size = 16                              # an older, shorter struct
        st.unresolved, st.tile_h = -5, -7
        assert call(dz.ptr, 0, ctypes.byref(st)) == backend.OK
        assert st.struct_size == 16 and st.flat_cells == 3 and st.rounds == 1
        assert st.unresolved == -5 and st.tile_h == -7   # nothing beyond it is written
        assert call(dz.ptr, 0, None) == backend.OK       # no stats wanted
        assert do.to_host()[2].tolist() == [0, 0, W_, W_, E, 0, 0]
