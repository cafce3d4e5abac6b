"""
D-infinity flow direction and accumulation on the MI355X (``DInfFlowDirection``,
``DInfFlowAccumulation``, ``DemToDInfArea``, ``hdem_dinf_f32[_dev]``, ``hdem_dinfacc_u32[_dev]``).

The definition and the host references are those of tests/test_dinf.py.  Every comparison is
``np.array_equal`` but one: the float32 ``angle`` is held to 1 float32 ulp of the float64
reference rounded to float32 (both sides round a float64 value good to a few float64 ulp, so
they can differ only by the side of a float32 rounding boundary they land on).  Words are held
to equality: the only library function in ``q`` is one float64 ``atan2`` whose quotient is then
rounded to 15 bits, so two implementations a few ulp apart disagree only within ~1e-16 of a
rounding boundary; a cell that differs is reported with both words.  The accumulation takes
its words from the *reference* direction, so that question cannot reach it.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, dinf
from hydrodem_amd.backend import DeviceRaster
from hydrodem_amd.dinf import Q_ONE
from elevation_regimes import REGIMES, regime_raster
from test_dinf import (accumulate_ref, counts_of, direction_ref, plane, random_dem, value_of)
from test_flowacc import random_acyclic_codes, terminal_mask
from test_gpu_flowacc import path_codes, spiral
from test_gpu_scribble import Case, execute

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (2, 9), (3, 3), (64, 64), (65, 63), (130, 197)]
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


# ---------------------------------------------------------------------------
# direction
# ---------------------------------------------------------------------------
def ulps_apart(a, b):
    """Distance in float32 values between two float32 arrays of one sign pattern."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def assert_direction(z, cellsize=1.0, fallback=None):
    z = np.ascontiguousarray(z, dtype=F32)
    dx, dy = dinf.cellsizes(cellsize)
    want_words, want_angle, want_slope, taken = direction_ref(z, dx, dy, fallback)
    words, extras, stats = dinf.dinf(z, cellsize, fallback, dinf.EXTRAS)
    assert words.dtype == np.uint32 and extras["angle"].dtype == F32 and extras["slope"].dtype == F32
    differ = np.argwhere(words != want_words)
    assert not len(differ), [(tuple(c), hex(words[tuple(c)]), hex(want_words[tuple(c)]))
                             for c in differ[:5]]
    assert np.array_equal(extras["slope"].view(np.uint32), want_slope.view(np.uint32))
    want32 = want_angle.astype(F32)
    assert np.array_equal(extras["angle"] < 0, want32 < 0)
    assert int(ulps_apart(extras["angle"], want32).max()) <= 1
    assert stats["no_flow"] == int((want_words == 0).sum()) and stats["fallback_cells"] == taken
    # the words alone are the same words; so are those of the device form
    alone, none, _ = dinf.dinf(z, cellsize, fallback)
    assert none == {} and np.array_equal(alone, words)
    with DeviceRaster.from_host(z, dtype=F32) as dz, \
            backend.on_device(fallback, dtype=np.uint8) as dfb:
        dev, dev_extras, dev_stats = dinf.dinf_dev(dz, cellsize, dfb, ("slope",))
        with dev, dev_extras["slope"] as ds:
            assert np.array_equal(dev.to_host(), words)
            assert np.array_equal(ds.to_host().view(np.uint32), want_slope.view(np.uint32))
        assert {k: v for k, v in dev_stats.items() if k != "ms_total"} == \
            {k: v for k, v in stats.items() if k != "ms_total"}
    return words, stats


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_direction_matches_the_reference(shape):
    words, _ = assert_direction(random_dem(shape, seed=shape[0] * 7 + shape[1]))
    assert min(shape) < 64 or counts_of(words)["split_cells"] > 0.1 * words.size


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_direction_in_every_elevation_regime(regime):
    assert_direction(regime_raster(regime, (130, 197)))


def test_direction_with_nodata_and_with_cells_that_are_not_square():
    _, stats = assert_direction(random_dem((130, 197), seed=11, nan=0.01))
    assert stats["no_flow"] > 130 * 2 + 197 * 2 - 4
    assert_direction(random_dem((130, 197), seed=12), cellsize=(30.0, 10.0))
    assert_direction(plane((70, 300), 3.0, 1.0, 30.0, 10.0), cellsize=(30.0, 10.0))
    assert_direction(plane((40, 50), 1.0, 0.0))


@pytest.fixture(scope="module")
def integer_fill():
    """Integer metres, their exact fill and its D8 codes routed across the flats, 256^2."""
    z = np.round(hdem_synth.synth_dem(256, 256, variant="rough")).astype(F32)
    chain = hd.HydroConditioning(epsilon=0.0, flats="resolve")
    codes = chain.apply(z)
    filled = chain.filled
    filled.setflags(write=False)
    codes.setflags(write=False)
    return filled, codes


def test_direction_on_integer_metres_with_the_resolved_codes_as_fallback(integer_fill):
    filled, codes = integer_fill
    words, stats = assert_direction(filled, fallback=codes)
    assert stats["fallback_cells"] > 0.05 * filled.size
    # the flats keep draining: every unit arrives on the ring
    acc = hd.DInfFlowAccumulation(output="sum").apply(words)
    assert np.array_equal(acc, accumulate_ref(words))
    assert int(acc[words >> 16 == 0].sum()) == filled.size << 16
    assert not (words[1:-1, 1:-1] == 0).any()


def test_direction_keeps_its_partial_results():
    z = random_dem((65, 63), seed=3)
    want_words, want_angle, want_slope, _ = direction_ref(z)
    op = hd.DInfFlowDirection(keep_partial_results=True)
    assert np.array_equal(op.apply(z), want_words)
    assert np.array_equal(op.slope, want_slope) and op.angle.dtype == F32
    plain = hd.DInfFlowDirection()
    with DeviceRaster.from_host(z, dtype=F32) as dz, plain.apply_device(dz) as dev:
        assert dev.dtype == np.uint32 and np.array_equal(dev.to_host(), want_words)
    assert plain.angle is None and plain.slope is None
    fallback = np.zeros(z.shape, np.uint8)
    fallback[0, :2] = 3
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        hd.DInfFlowDirection(fallback=fallback).apply(z)


# ---------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------
def schedule_free(stats):
    return {k: stats[k] for k in ("split_cells", "terminal_cells", "invalid", "outside",
                                  "unresolved", "tile_h", "tile_w")}


def assert_accumulation(words, frac_bits=16, want=None):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    want = accumulate_ref(words, frac_bits) if want is None else want
    outs, stats = dinf.dinfacc(words, frac_bits, ("sum", "value"))
    assert outs["sum"].dtype == np.int64 and outs["value"].dtype == F32
    assert np.array_equal(outs["sum"], want)
    assert np.array_equal(outs["value"], value_of(want, frac_bits))
    assert schedule_free(stats) == counts_of(words)
    assert stats["rounds"] >= 1 and stats["tile_visits"] >= -(-words.shape[0] // 64) * \
        -(-words.shape[1] // 64)
    return outs, stats


def random_acyclic_words(shape, seed):
    """Words over a random potential: every receiver lies strictly lower, so no cycle; a third
    of the cells split, and cells without a lower neighbour in their facet stay 0."""
    rng = np.random.default_rng(seed)
    h, w = shape
    p = np.full((h + 2, w + 2), -1, np.int64)              # outside: never a receiver
    p[1:-1, 1:-1] = rng.permutation(h * w).reshape(h, w)
    here = p[1:-1, 1:-1]
    facet = rng.integers(1, 9, shape)
    kind = rng.integers(0, 3, shape)
    q = np.where(kind == 0, 0, np.where(kind == 1, Q_ONE, rng.integers(1, Q_ONE, shape)))
    for k, ((y1, x1), (y2, x2), _, _) in dinf.FACETS.items():
        card = p[1 + y1:h + 1 + y1, 1 + x1:w + 1 + x1]
        diag = p[1 + y2:h + 1 + y2, 1 + x2:w + 1 + x2]
        card_ok, diag_ok = (card >= 0) & (card < here), (diag >= 0) & (diag < here)
        m = facet == k
        q = np.where(m & ~card_ok, Q_ONE, q)                # the diagonal alone ...
        q = np.where(m & ~diag_ok, 0, q)                    # ... or the cardinal alone ...
        facet = np.where(m & ~card_ok & ~diag_ok, 0, facet)     # ... or nothing
    q = np.where(facet == 0, 0, q)
    return dinf.pack(facet, q)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_accumulation_on_the_reference_direction(shape, frac_bits):
    words, _, _, _ = direction_ref(random_dem(shape, seed=shape[0] * 7 + shape[1], nan=0.01))
    outs, _ = assert_accumulation(words, frac_bits)
    assert int(outs["sum"][words >> 16 == 0].sum()) == words.size << frac_bits


@pytest.mark.parametrize("shape", [(130, 197), (1, 200), (65, 1), (64, 128), (200, 70)], ids=IDS)
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_accumulation_on_random_acyclic_words(shape, frac_bits):
    words = random_acyclic_words(shape, seed=shape[0] * 3 + shape[1])
    assert min(shape) == 1 or counts_of(words)["split_cells"] > 0.05 * words.size
    assert_accumulation(words, frac_bits)


@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles(upright):
    n = 4097
    codes = np.zeros((5, n), np.uint8)
    codes[2, :n - 1] = 1                                  # eastwards
    want = np.full((5, n), 1 << 16, np.int64)
    want[2] = np.arange(1, n + 1, dtype=np.int64) << 16
    if upright:
        codes, want = np.where(codes.T, 4, 0).astype(np.uint8), np.ascontiguousarray(want.T)
    _, stats = assert_accumulation(dinf.words_from_d8(np.ascontiguousarray(codes)), want=want)
    # (a tile per round, unless a tile happens to see its neighbour's cells of the same round)
    assert stats["rounds"] > 1 and stats["terminal_cells"] == 4 * n + 1


def test_a_zigzag_of_1000_diagonal_steps_along_a_tile_seam():
    cells = [(k, 63 + k % 2) for k in range(1001)]         # crosses column 63 | 64 every step
    words = dinf.words_from_d8(path_codes((1001, 128), cells))
    want = np.full((1001, 128), 1 << 16, np.int64)
    for k, (y, x) in enumerate(cells):
        want[y, x] = (k + 1) << 16
    _, stats = assert_accumulation(words, want=want)
    assert stats["rounds"] > 1                             # the worst case: about one per step


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    want = np.full(shape, 1, np.int64)
    for k, (y, x) in enumerate(cells):
        want[y, x] = k + 1
    assert_accumulation(dinf.words_from_d8(path_codes(shape, cells)), 0, want)
    assert_accumulation(dinf.words_from_d8(path_codes(shape, cells)), 16, want << 16)


def test_a_cone_where_nearly_every_cell_splits():
    rows, cols = np.mgrid[0:200, 0:200]
    words, _, _, _ = direction_ref((-np.hypot(rows - 99.5, cols - 99.5)).astype(F32))
    assert counts_of(words)["split_cells"] > 0.9 * 198 * 198
    outs, _ = assert_accumulation(words)
    assert int(outs["sum"][words == 0].sum()) == 200 * 200 << 16


@pytest.mark.parametrize("frac_bits", [0, 7, 16])
def test_canonical_words_give_the_d8_accumulation(frac_bits):
    codes = random_acyclic_codes(150, 210, seed=5, ramp=True)
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    acc = hd.FlowAccumulation().apply(codes)
    got = hd.DInfFlowAccumulation(frac_bits=frac_bits, output="sum").apply(dinf.words_from_d8(codes))
    assert np.array_equal(got, acc.astype(np.int64) << frac_bits)


def test_two_runs_and_both_forms_give_identical_bytes():
    words = random_acyclic_words((257, 130), seed=21)
    a, stats_a = dinf.dinfacc(words, 16, ("sum", "value"))
    b, _ = dinf.dinfacc(words, 16, ("sum", "value"))
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw:
        dev, stats_c = dinf.dinfacc_dev(dw, 16, ("sum", "value"))
        with dev["sum"] as ds, dev["value"] as dv:
            c = {"sum": ds.to_host(), "value": dv.to_host()}
        # one output at a time: the working raster is then the arena's, or the caller's sum
        for name in ("value", "sum"):
            op = hd.DInfFlowAccumulation(output=name)
            with op.apply_device(dw) as one:
                assert one.dtype == a[name].dtype and one.to_host().tobytes() == a[name].tobytes()
            assert op.apply(words).tobytes() == a[name].tobytes()
    for name in ("sum", "value"):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes()
    assert schedule_free(stats_a) == schedule_free(stats_c)


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    words = random_acyclic_words((300, 300), seed=9)
    z = random_dem((300, 300), seed=9)
    ctx = backend.context()
    acc, direct = hd.DInfFlowAccumulation(), hd.DInfFlowDirection()
    acc.apply(words)
    direct.apply(z)
    assert acc.stats["ms_classify"] == 0 and acc.stats["ms_relax"] == 0
    assert acc.stats["ms_final"] == 0 and direct.stats["ms_total"] == 0
    ctx.profile(True)
    try:
        acc.apply(words)
        direct.apply(z)
    finally:
        ctx.profile(False)
    assert acc.stats["ms_classify"] > 0 and acc.stats["ms_relax"] > 0 and acc.stats["ms_final"] > 0
    assert direct.stats["ms_total"] > 0 and "struct_size" not in acc.stats


# ---------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rough_1024():
    z = hdem_synth.synth_dem(1024, 1024, variant="rough")
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("flats,epsilon", [("keep", 1e-3), ("resolve", 0.0)])
def test_the_chain_on_1024_against_the_reference_on_its_own_stages(rough_1024, flats, epsilon):
    chain = hd.DemToDInfArea(epsilon=epsilon, flats=flats, output="sum", keep_partial_results=True)
    got = chain.apply(rough_1024)
    assert chain.filled.dtype == F32 and chain.codes.dtype == np.uint8
    want_words, _, _, taken = direction_ref(chain.filled, fallback=chain.codes)
    assert np.array_equal(chain.words, want_words)
    want = accumulate_ref(want_words)
    assert np.array_equal(got, want)
    assert int(got[want_words >> 16 == 0].sum()) == rough_1024.size << 16
    assert chain.stats["DInfFlowDirection"]["fallback_cells"] == taken
    assert schedule_free(chain.stats["DInfFlowAccumulation"]) == counts_of(want_words)
    # (about a fifth of the cells split on the gradient fill; the flats of the exact fill take
    # their one receiver from the fallback)
    assert 0.05 < chain.stats["DInfFlowAccumulation"]["split_cells"] / rough_1024.size < 0.4
    assert ("ResolveFlats" in chain.stats) == (flats == "resolve")
    assert set(chain.stats) - {"ResolveFlats"} == {"SinkFill", "DInfFlowDirection",
                                                  "DInfFlowAccumulation"}
    # the default output, without the stages kept, on the device
    plain = hd.DemToDInfArea(epsilon=epsilon, flats=flats)
    with DeviceRaster.from_host(rough_1024, dtype=F32) as dz, plain.apply_device(dz) as area:
        assert area.dtype == F32 and np.array_equal(area.to_host(), value_of(want))
    assert plain.filled is None and plain.codes is None and plain.words is None


# ---------------------------------------------------------------------------
# refusals: the context stays usable
# ---------------------------------------------------------------------------
def loop_cells(y0, x0, n):
    """The perimeter of an n x n square, clockwise from its first cell: 4 n - 4 cells."""
    top = [(y0, x0 + k) for k in range(n - 1)]
    right = [(y0 + k, x0 + n - 1) for k in range(n - 1)]
    bottom = [(y0 + n - 1, x0 + n - 1 - k) for k in range(n - 1)]
    left = [(y0 + n - 1 - k, x0) for k in range(n - 1)]
    return top + right + bottom + left


def test_invalid_words_are_refused_with_their_count():
    words = random_acyclic_words((70, 90), seed=2)
    kinds = {"facet > 8": 9 << 16, "q > 32768": (3 << 16) | (Q_ONE + 1), "facet 0 with q": 7,
             "stray bit 20": (2 << 16) | (1 << 20), "stray bit 31": 1 << 31}
    for n, (kind, word) in enumerate(kinds.items(), 1):
        bad = words.copy()
        bad[5:5 + n, 66] = word
        with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells: the facet"):
            hd.DInfFlowAccumulation().apply(bad)
        with DeviceRaster.from_host(bad, dtype=np.uint32) as dw:
            with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells"):
                hd.DInfFlowAccumulation(output="sum").apply_device(dw)
        assert kind
    assert_accumulation(words)


def test_a_receiver_outside_the_raster_is_refused():
    words = np.zeros((66, 70), np.uint32)
    words[0, 3] = dinf.pack(2, 0)                         # north of the first row
    words[65, 69] = dinf.pack(8, 100)                     # east is outside, south-east too
    words[30, 69] = dinf.pack(1, Q_ONE)                   # north-east only, outside
    words[30, 0] = dinf.pack(1, Q_ONE)                    # north-east only, inside
    with pytest.raises(ValueError, match="send flow outside the raster in 3 cells"):
        hd.DInfFlowAccumulation().apply(words)
    with pytest.raises(ValueError, match="outside the raster in 3 cells"):
        accumulate_ref(words)


def test_cycles_are_refused_in_bounded_time():
    words = np.zeros((40, 130), np.uint32)
    words[7, 7:9] = dinf.pack(np.array([1, 4]), np.array([0, 0]))     # E then W: a 2-cycle
    with pytest.raises(ValueError, match="form a cycle: 2 cells never resolve"):
        hd.DInfFlowAccumulation().apply(words)
    cells = loop_cells(10, 59, 11)                        # across the seam at column 64
    assert len(cells) == 40
    words = dinf.words_from_d8(path_codes((40, 130), cells + cells[:1]))
    words[3, 3] = dinf.pack(7, 1000)                      # and a cell that does resolve
    op = hd.DInfFlowAccumulation(output="sum")
    with pytest.raises(ValueError, match="form a cycle: 40 cells never resolve"):
        op.apply(words)
    with pytest.raises(ValueError, match="40 cells never resolve"):
        accumulate_ref(words)
    # a cell that the loop drains into never resolves either: (10, 60) also sends north-east
    words[10, 60] = dinf.pack(1, 5)
    with pytest.raises(ValueError, match="form a cycle: 41 cells never resolve"):
        op.apply(words)
    assert_accumulation(random_acyclic_words((40, 130), seed=1))


def test_an_output_of_the_wrong_dtype_is_refused_and_the_c_entry_points_check_their_arguments():
    words = random_acyclic_words((20, 30), seed=4)
    ctx = backend.context()
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.empty(words.shape, np.uint32, ctx) as wrong, \
            DeviceRaster.empty((20, 31), np.int64, ctx) as wide, \
            DeviceRaster.empty(words.shape, np.int64, ctx) as right:
        with pytest.raises(ValueError, match=r"out\['sum'\] is int64, got uint32"):
            dinf.dinfacc_dev(dw, want="sum", out={"sum": wrong})
        with pytest.raises(ValueError, match=r"out\['sum'\] is \(20, 31\), the words \(20, 30\)"):
            dinf.dinfacc_dev(dw, want="sum", out={"sum": wide})
        with pytest.raises(ValueError, match="out has value, which is not wanted"):
            dinf.dinfacc_dev(dw, want="sum", out={"value": right})
        outs, _ = dinf.dinfacc_dev(dw, want="sum", out={"sum": right})
        assert outs["sum"] is right and np.array_equal(right.to_host(), accumulate_ref(words))
        fn = ctx.lib.hdem_dinfacc_u32_dev
        call = lambda frac, s, v, flags, st: fn(           # noqa: E731
            ctx.handle, dw.ptr, 20, 30, frac, s, v, flags, st)
        assert call(16, None, None, 0, None) == backend.BAD_ARG
        assert b"no output wanted" in ctx.lib.hdem_last_error()
        assert call(17, right.ptr, None, 0, None) == backend.BAD_ARG
        assert b"frac_bits is 0 ... 16, got 17" in ctx.lib.hdem_last_error()
        assert call(16, right.ptr, None, 1, None) == backend.BAD_ARG
        assert b"flags" in ctx.lib.hdem_last_error()
        st = backend._DInfAccStats()                       # pylint: disable=protected-access
        st.struct_size = 0
        assert call(16, right.ptr, None, 0, ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend._DInfAccStats()                       # pylint: disable=protected-access
        st.struct_size = 24                                # an older, shorter struct
        st.terminal_cells, st.tile_h = -5, -7
        assert call(16, right.ptr, None, 0, ctypes.byref(st)) == backend.OK
        assert st.struct_size == 24 and st.split_cells == counts_of(words)["split_cells"]
        assert st.terminal_cells == -5 and st.tile_h == -7   # nothing beyond it is written
        fake = ctypes.c_void_p(256)                        # never dereferenced
        for f in (ctx.lib.hdem_dinfacc_u32_dev, ctx.lib.hdem_dinfacc_u32):
            assert f(ctx.handle, fake, 65536, 65536, 16, fake, None, 0, None) == backend.BAD_ARG
            assert b"2^32" in ctx.lib.hdem_last_error()
        for f in (ctx.lib.hdem_dinf_f32_dev, ctx.lib.hdem_dinf_f32):
            assert f(ctx.handle, fake, 4, 4, None, 0.0, 1.0, fake, None, None, 0,
                     None) == backend.BAD_ARG
            assert b"dx and dy must be finite and positive" in ctx.lib.hdem_last_error()
            assert f(ctx.handle, fake, 4, 4, None, 1.0, 1.0, None, None, None, 0,
                     None) == backend.BAD_ARG


# ---------------------------------------------------------------------------
# poisoned scratch and output memory
# ---------------------------------------------------------------------------
def poison_words(shape, seed=33):
    return {"words": random_acyclic_words(shape, seed=seed)}


def poison_dem(shape, seed=33):
    return {"z": random_dem(shape, seed=seed, nan=0.01)}


def poison_run_acc(call, inp):
    """The accumulation for ``value`` alone (the arena's working raster), then for both outputs
    (the caller's or the library's sum as working raster)."""
    words = inp["words"]
    dw = call.up(words)
    out = {name: call.out(words.shape, dtype) for name, dtype in dinf.OUTPUTS}
    alone, _ = dinf.dinfacc_dev(dw, 16, "value", {"value": out["value"]} if call.own else None)
    host = {"alone": alone["value"].to_host()}
    if not call.own:
        call.stack.enter_context(alone["value"])
    dev, stats = dinf.dinfacc_dev(dw, 16, ("sum", "value"), out if call.own else None)
    for name, raster in dev.items():
        assert not call.own or raster is out[name]
        host[name] = call.host(raster)
    return host, schedule_free(stats)


def poison_check_acc(inp, got):
    assert np.array_equal(got["sum"], accumulate_ref(inp["words"]))
    assert np.array_equal(got["alone"], got["value"])


def poison_run_direction(call, inp):
    """The direction for the words and both extras."""
    dz = call.up(inp["z"])
    made, extras, stats = dinf.dinf_dev(dz, 1.0, None, dinf.EXTRAS, call.out(dz.shape, np.uint32))
    host = {name: call.host(raster) for name, raster in {"words": made, **extras}.items()}
    return host, {k: v for k, v in stats.items() if not k.startswith("ms_")}


def poison_check_direction(inp, got):
    want_words, want_angle, want_slope, _ = direction_ref(inp["z"], 1.0, 1.0, None)
    assert got["words"].dtype == np.uint32 and np.array_equal(got["words"], want_words)
    assert np.array_equal(got["slope"].view(np.uint32), want_slope.view(np.uint32))
    want32 = want_angle.astype(F32)
    assert np.array_equal(got["angle"] < 0, want32 < 0)
    assert int(ulps_apart(got["angle"], want32).max()) <= 1


# (33, 257): a second 256-column tile of the direction kernel, one cell wide
POISON_CASES = [Case("dinfacc", ((130, 197),), poison_words, poison_run_acc, poison_check_acc,
                     True, frozenset()),
                Case("dinf-direction", ((130, 197), (33, 257)), poison_dem, poison_run_direction,
                     poison_check_direction, True, frozenset())]


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
def test_poisoned_memory_changes_no_byte(own):
    for entry in POISON_CASES:
        inp = entry.build((130, 197))
        clean, clean_stats = execute(entry, inp, None, own)
        entry.check(inp, clean)
        for byte in (0x00, 0xFF, 0x7F, 0x01):
            got, stats = execute(entry, inp, byte, own)
            assert stats == clean_stats
            assert got.keys() == clean.keys()
            for name, raster in clean.items():
                assert got[name].tobytes() == raster.tobytes(), (entry.name, name, hex(byte))
