"""
Multiple-flow-direction flow direction and accumulation on the MI355X (``MFDFlowDirection``,
``MFDFlowAccumulation``, ``DemToMFDArea``, ``hdem_mfd_f32``, ``hdem_mfdacc_u64``).

The definition and the host references are those of tests/test_mfd.py.  Every comparison is
byte equality: the direction has no library function in it (the power is the contract's own
sequence of float64 operations, transcribed in the reference), and the accumulation is integer
adds.  The accumulation takes its words from the *reference* direction or from
``random_acyclic_words``, so the direction cannot reach it.

The two operators are one C symbol each, taking host or device pointers by a flag, so the table
of tests/device_cases.py does not list them; this file supplies that coverage itself: both
forms on every input, poisoned scratch and output memory, and a caller's stream behind an
unfinished producer (``POISON_CASES`` with the machinery of tests/test_gpu_scribble.py and
tests/test_gpu_streams.py).
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
import size_regimes as sr
from hydrodem_amd import backend, dinf, mfd
from hydrodem_amd.backend import DeviceRaster
from elevation_regimes import REGIMES, regime_raster
from test_dinf import random_dem, value_of
from test_flowacc import random_acyclic_codes, terminal_mask
from test_gpu_flowacc import path_codes, spiral
from test_gpu_scribble import Case, assert_same_bytes, execute
from test_gpu_streams import Delay, on_a_callers_stream
from test_mfd import (accumulate_ref, counts_of, direction_ref, random_acyclic_words)

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (2, 9), (3, 3), (64, 64), (65, 63), (130, 197)]
WIDE = (33, 257)                # a second 256-column tile of the direction kernel, one cell wide
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731
METHODS = {"exponent-1": ((1.0, 1.0, 1.0), None), "freeman-1.1": ("freeman", None),
           "holmgren-4": ("holmgren", 4.0), "quinn": ("quinn", None)}


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def without_times(stats):
    return {k: v for k, v in stats.items() if not k.startswith("ms_")}


# ---------------------------------------------------------------------------
# direction
# ---------------------------------------------------------------------------
def assert_direction(z, method="freeman", exponent=None, cellsize=1.0, fallback=None):
    z = np.ascontiguousarray(z, dtype=F32)
    dx, dy = mfd.cellsizes(cellsize)
    want_words, want_slope, want_stats = direction_ref(z, method, exponent, dx, dy, fallback)
    words, extras, stats = mfd.mfd(z, method, exponent, cellsize, fallback, mfd.EXTRAS)
    assert words.dtype == np.uint64 and extras["slope"].dtype == F32
    differ = np.argwhere(words != want_words)
    assert not len(differ), [(tuple(c), hex(words[tuple(c)]), hex(want_words[tuple(c)]))
                             for c in differ[:5]]
    assert np.array_equal(extras["slope"].view(np.uint32), want_slope.view(np.uint32))
    assert without_times(stats) == want_stats
    # the words alone are the same words; so are those of the device form, and its stats
    alone, none, _ = mfd.mfd(z, method, exponent, cellsize, fallback)
    assert none == {} and alone.tobytes() == words.tobytes()
    with DeviceRaster.from_host(z, dtype=F32) as dz, \
            backend.on_device(fallback, dtype=np.uint8) as dfb:
        dev, dev_extras, dev_stats = mfd.mfd_dev(dz, method, exponent, cellsize, dfb, ("slope",))
        with dev, dev_extras["slope"] as ds:
            assert dev.dtype == np.uint64 and dev.to_host().tobytes() == words.tobytes()
            assert ds.to_host().tobytes() == want_slope.tobytes()
        assert without_times(dev_stats) == want_stats
    return words, stats


@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=IDS)
@pytest.mark.parametrize("method", sorted(METHODS))
def test_direction_matches_the_reference(shape, method):
    words, stats = assert_direction(random_dem(shape, seed=shape[0] * 7 + shape[1]),
                                    *METHODS[method])
    assert min(shape) < 33 or stats["split_cells"] > 0.5 * words.size


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_direction_in_every_elevation_regime(regime):
    assert_direction(regime_raster(regime, (130, 197)))
    assert_direction(regime_raster(regime, (130, 197)), "holmgren", 4.0)


def test_direction_with_nodata_and_with_cells_that_are_not_square():
    z = random_dem((130, 197), seed=11, nan=0.01)
    _, stats = assert_direction(z)
    assert stats["no_flow"] >= int(np.isnan(z).sum()) > 100
    assert_direction(z, "quinn", None, (30.0, 20.0))
    assert_direction(random_dem((130, 197), seed=12), "holmgren", 4.0, (30.0, 20.0))
    rows, cols = np.mgrid[0:70, 0:300]
    assert_direction((-(3.0 * cols * 30.0 - rows * 20.0)).astype(F32), cellsize=(30.0, 20.0))
    # a plane tilted east: whole families of cells with the same three weights
    words, _ = assert_direction((-cols[:40, :50]).astype(F32), (1.0, 1.0, 1.0))
    assert (mfd.shares_of(words)[1:-1, :-1] == [106, 75, 0, 0, 0, 0, 0, 75]).all()
    # infinite elevations go through the definition as they are
    z = random_dem((65, 63), seed=13)
    z[10, 10], z[20, 20] = -np.inf, np.inf
    assert_direction(z)


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
    # the flats keep draining: every unit arrives at a cell without outflow, on the ring
    acc = hd.MFDFlowAccumulation(output="sum").apply(words)
    assert np.array_equal(acc, accumulate_ref(words))
    assert int(acc[words == 0].sum()) == filled.size << 16
    assert not (words[1:-1, 1:-1] == 0).any()


def test_direction_keeps_its_partial_results():
    z = random_dem((65, 63), seed=3)
    want_words, want_slope, _ = direction_ref(z)
    op = hd.MFDFlowDirection(keep_partial_results=True)
    assert np.array_equal(op.apply(z), want_words)
    assert np.array_equal(op.slope, want_slope) and op.slope.dtype == F32
    plain = hd.MFDFlowDirection()
    with DeviceRaster.from_host(z, dtype=F32) as dz, plain.apply_device(dz) as dev:
        assert dev.dtype == np.uint64 and np.array_equal(dev.to_host(), want_words)
    assert plain.slope is None
    fallback = np.zeros(z.shape, np.uint8)
    flat = np.zeros(z.shape, F32)
    fallback[0, :2] = 3
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        hd.MFDFlowDirection(fallback=fallback).apply(flat)
    # the slope feeds the area wetness index as its given slope
    area = hd.MFDFlowAccumulation().apply(want_words)
    twi = hd.AreaWetnessIndex(area, given_slope=op.slope).apply(z)
    assert twi.shape == z.shape and twi.dtype == F32 and np.isfinite(twi[1:-1, 1:-1]).all()


# ---------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------
def schedule_free(stats):
    return {k: stats[k] for k in ("split_cells", "terminal_cells", "invalid", "outside",
                                  "unresolved", "tile_h", "tile_w")}


def assert_accumulation(words, frac_bits=16, want=None, weights=None):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    want = accumulate_ref(words, weights, frac_bits) if want is None else want
    outs, stats = mfd.mfdacc(words, weights, frac_bits, ("sum", "value"))
    assert outs["sum"].dtype == np.int64 and outs["value"].dtype == F32
    assert np.array_equal(outs["sum"], want)
    assert np.array_equal(outs["value"], value_of(want, frac_bits))
    assert schedule_free(stats) == counts_of(words)
    assert stats["rounds"] >= 1 and stats["tile_visits"] >= sr.tiles_of(words.shape)
    return outs, stats


@pytest.mark.parametrize("shape", SHAPES + [(1, 200), (65, 1)], ids=IDS)
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_accumulation_on_random_acyclic_words(shape, frac_bits):
    words = random_acyclic_words(shape, seed=shape[0] * 3 + shape[1])
    assert min(shape) < 64 or counts_of(words)["split_cells"] > 0.3 * words.size
    outs, _ = assert_accumulation(words, frac_bits)
    assert int(outs["sum"][words == 0].sum()) == words.size << frac_bits


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accumulation_on_the_reference_direction(shape):
    words, _, _ = direction_ref(random_dem(shape, seed=shape[0] * 7 + shape[1], nan=0.01))
    outs, _ = assert_accumulation(words)
    assert int(outs["sum"][words == 0].sum()) == words.size << 16


@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles(upright):
    n = 4097
    cells = [(2, x) for x in range(n)]
    want = np.full((5, n), 1 << 16, np.int64)
    want[2] = np.arange(1, n + 1, dtype=np.int64) << 16
    codes = path_codes((5, n), cells)
    if upright:
        codes, want = path_codes((n, 5), [(x, y) for y, x in cells]), np.ascontiguousarray(want.T)
    _, stats = assert_accumulation(mfd.words_from_d8(codes), want=want)
    assert stats["rounds"] > 1 and stats["terminal_cells"] == 4 * n + 1


def test_a_zigzag_of_1000_diagonal_steps_along_a_tile_seam():
    cells = [(k, 63 + k % 2) for k in range(1001)]         # crosses column 63 | 64 every step
    words = mfd.words_from_d8(path_codes((1001, 128), cells))
    want = np.full((1001, 128), 1 << 16, np.int64)
    for k, (y, x) in enumerate(cells):
        want[y, x] = (k + 1) << 16
    _, stats = assert_accumulation(words, want=want)
    assert stats["rounds"] > 1


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    want = np.full(shape, 1, np.int64)
    for k, (y, x) in enumerate(cells):
        want[y, x] = k + 1
    assert_accumulation(mfd.words_from_d8(path_codes(shape, cells)), 0, want)
    assert_accumulation(mfd.words_from_d8(path_codes(shape, cells)), 16, want << 16)


def test_a_cone_where_nearly_every_cell_has_three_receivers_or_more():
    rows, cols = np.mgrid[0:200, 0:200]
    words, _, _ = direction_ref((-np.hypot(rows - 99.5, cols - 99.5)).astype(F32),
                                (1.0, 1.0, 1.0))
    receivers = (mfd.shares_of(words) > 0).sum(axis=-1)
    assert (receivers >= 3).sum() > 0.9 * 198 * 198
    outs, _ = assert_accumulation(words)
    assert int(outs["sum"][words == 0].sum()) == 200 * 200 << 16


@pytest.mark.parametrize("frac_bits", [0, 7, 16])
def test_canonical_words_give_the_d8_and_the_d_infinity_accumulation(frac_bits):
    codes = random_acyclic_codes(150, 210, seed=5, ramp=True)
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    acc = hd.FlowAccumulation().apply(codes)
    got = hd.MFDFlowAccumulation(frac_bits=frac_bits, output="sum").apply(mfd.words_from_d8(codes))
    assert np.array_equal(got, acc.astype(np.int64) << frac_bits)
    outs, _ = dinf.dinfacc(dinf.words_from_d8(codes), frac_bits, ("sum", "value"))
    mine, _ = mfd.mfdacc(mfd.words_from_d8(codes), None, frac_bits, ("sum", "value"))
    assert mine["sum"].tobytes() == outs["sum"].tobytes()
    assert mine["value"].tobytes() == outs["value"].tobytes()


def test_a_strip_whose_schedule_kernel_spans_two_workgroups():
    shape = sr.DINF_SHAPES[1]
    assert sr.schedule_blocks(shape) >= 2 and sr.tiles_of(shape) > 256
    words = random_acyclic_words(shape, seed=sr.DINF_SEED)
    assert counts_of(words)["split_cells"] >= 0.05 * words.size
    _, stats = assert_accumulation(words)
    assert stats["rounds"] >= 2


def test_weighted_accumulation_against_the_reference():
    rng = np.random.default_rng(17)
    shape = (130, 197)
    words = random_acyclic_words(shape, seed=23)
    cases = ((rng.random(shape).astype(F32) * 9, 20), (rng.random(shape).astype(F32), 30),
             (rng.integers(0, 2 ** 14, shape).astype(np.uint32), 16),
             (rng.integers(0, 256, shape).astype(np.uint8), 3))
    for weights, frac_bits in cases:
        weights = np.ascontiguousarray(weights)
        if weights.dtype == F32:
            weights[rng.random(shape) < 0.01] = np.nan
            weights[5, 5] = -0.0
        outs, stats = assert_accumulation(words, frac_bits, weights=weights)
        total = int(dinf.quantise(weights, frac_bits).sum())
        assert stats["total"] == total and int(outs["sum"][words == 0].sum()) == total
        assert stats["nan_weights"] == int(np.isnan(weights.astype(np.float64)).sum())
        assert stats["bad_weights"] == 0
    ones = np.ones(shape, np.uint8)
    plain, _ = mfd.mfdacc(words, None, 16, ("sum", "value"))
    for weights in (ones, ones.astype(np.uint32), ones.astype(F32)):
        weighted, _ = mfd.mfdacc(words, weights, 16, ("sum", "value"))
        assert weighted["sum"].tobytes() == plain["sum"].tobytes()
        assert weighted["value"].tobytes() == plain["value"].tobytes()
    op = hd.MFDFlowAccumulation(weights=cases[2][0], output="sum")
    want = accumulate_ref(words, cases[2][0], 16)
    assert np.array_equal(op.apply(words), want) and op.stats["total"] == int(want[words == 0].sum())
    with DeviceRaster.from_host(words, dtype=np.uint64) as dw, op.apply_device(dw) as dev:
        assert np.array_equal(dev.to_host(), want)


def test_two_runs_and_both_forms_give_identical_bytes():
    words = random_acyclic_words((257, 130), seed=21)
    a, stats_a = mfd.mfdacc(words, None, 16, ("sum", "value"))
    b, _ = mfd.mfdacc(words, None, 16, ("sum", "value"))
    with DeviceRaster.from_host(words, dtype=np.uint64) as dw:
        dev, stats_c = mfd.mfdacc_dev(dw, None, 16, ("sum", "value"))
        with dev["sum"] as ds, dev["value"] as dv:
            c = {"sum": ds.to_host(), "value": dv.to_host()}
        # one output at a time: the working raster is then the arena's, or the caller's sum
        for name in ("value", "sum"):
            op = hd.MFDFlowAccumulation(output=name)
            with op.apply_device(dw) as one:
                assert one.dtype == a[name].dtype and one.to_host().tobytes() == a[name].tobytes()
            assert op.apply(words).tobytes() == a[name].tobytes()
    for name in ("sum", "value"):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes()
    assert schedule_free(stats_a) == schedule_free(stats_c)
    assert np.array_equal(a["sum"], accumulate_ref(words))


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    words = random_acyclic_words((300, 300), seed=9)
    z = random_dem((300, 300), seed=9)
    ctx = backend.context()
    acc, direct = hd.MFDFlowAccumulation(), hd.MFDFlowDirection()
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
def synth_300_500():
    z = hdem_synth.synth_dem(300, 500)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("flats,epsilon", [("keep", 1e-3), ("resolve", 0.0)])
def test_the_chain_against_the_reference_on_its_own_stages(synth_300_500, flats, epsilon):
    chain = hd.DemToMFDArea(epsilon=epsilon, flats=flats, output="sum", keep_partial_results=True)
    got = chain.apply(synth_300_500)
    assert chain.filled.dtype == F32 and chain.codes.dtype == np.uint8
    want_words, _, want_stats = direction_ref(chain.filled, fallback=chain.codes)
    assert np.array_equal(chain.words, want_words)
    want = accumulate_ref(want_words)
    assert np.array_equal(got, want)
    assert int(got[want_words == 0].sum()) == synth_300_500.size << 16
    assert without_times(chain.stats["MFDFlowDirection"]) == want_stats
    assert schedule_free(chain.stats["MFDFlowAccumulation"]) == counts_of(want_words)
    assert ("ResolveFlats" in chain.stats) == (flats == "resolve")
    assert set(chain.stats) - {"ResolveFlats"} == {"SinkFill", "MFDFlowDirection",
                                                  "MFDFlowAccumulation"}
    # the default output, without the stages kept, on the device; another method
    plain = hd.DemToMFDArea(epsilon=epsilon, flats=flats)
    with DeviceRaster.from_host(synth_300_500, dtype=F32) as dz, plain.apply_device(dz) as area:
        assert area.dtype == F32 and np.array_equal(area.to_host(), value_of(want))
    assert plain.filled is None and plain.codes is None and plain.words is None
    quinn = hd.DemToMFDArea(epsilon=epsilon, flats=flats, method="quinn", output="sum",
                            keep_partial_results=True)
    got = quinn.apply(synth_300_500)
    want_words, _, _ = direction_ref(quinn.filled, "quinn", fallback=quinn.codes)
    assert np.array_equal(quinn.words, want_words) and np.array_equal(got, accumulate_ref(want_words))


# ---------------------------------------------------------------------------
# refusals: argument errors that the library returns; the context stays usable
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
    has = mfd.HAS_FLOW
    kinds = {"shares without bit 59": 1, "a main direction without bit 59": 1 << 56,
             "bit 60": has | (1 << 60), "bit 63": 1 << 63, "shares that sum to 256": has | 0x8080}
    for n, (kind, word) in enumerate(kinds.items(), 1):
        bad = words.copy()
        bad[5:5 + n, 66] = word
        with pytest.raises(ValueError, match=f"invalid MFD word in {n} cells: a word is 0, or"):
            hd.MFDFlowAccumulation().apply(bad)
        with DeviceRaster.from_host(bad, dtype=np.uint64) as dw:
            with pytest.raises(ValueError, match=f"invalid MFD word in {n} cells"):
                hd.MFDFlowAccumulation(output="sum").apply_device(dw)
        with pytest.raises(ValueError, match=f"invalid MFD word in {n} cells"):
            accumulate_ref(bad)
        assert kind
    assert_accumulation(words)
    # 255 in all is a word: a lone cell that sends everything but 1 / 256 north-east and north
    ok = np.zeros((70, 90), np.uint64)
    ok[5, 66] = has | 0x807F
    outs, _ = assert_accumulation(ok)
    assert outs["sum"][4, 67] == (1 << 16) + ((1 << 16) * 0x7F >> 8)
    assert outs["sum"][5, 67] == (1 << 16) + 256


def test_a_receiver_outside_the_raster_is_refused():
    words = np.zeros((66, 70), np.uint64)
    none = [0] * 7
    words[0, 3] = mfd.pack(True, 2, none)                  # north of the first row
    words[65, 69] = mfd.pack(True, 6, [100] + none[1:])    # south is outside, south-east too
    words[30, 69] = mfd.pack(True, 4, none[:4] + [9] + none[5:])   # W main, NE share: outside
    words[30, 0] = mfd.pack(True, 1, none)                 # north-east only, inside
    words[40, 0] = mfd.pack(True, 0, none[:2] + [1] + none[3:])    # E main, a NW share: outside
    with pytest.raises(ValueError, match="send flow outside the raster in 4 cells"):
        hd.MFDFlowAccumulation().apply(words)
    with pytest.raises(ValueError, match="outside the raster in 4 cells"):
        accumulate_ref(words)


def test_cycles_are_refused_in_bounded_time():
    none = [0] * 7
    words = np.zeros((40, 130), np.uint64)
    words[7, 7], words[7, 8] = mfd.pack(True, 0, none), mfd.pack(True, 4, none)   # E then W
    with pytest.raises(ValueError, match="form a cycle: 2 cells never resolve"):
        hd.MFDFlowAccumulation().apply(words)
    cells = loop_cells(10, 59, 11)                        # across the seam at column 64
    assert len(cells) == 40
    words = mfd.words_from_d8(path_codes((40, 130), cells + cells[:1]))
    words[3, 3] = mfd.pack(True, 7, [100] + none[1:])     # and a cell that does resolve
    op = hd.MFDFlowAccumulation(output="sum")
    with pytest.raises(ValueError, match="form a cycle: 40 cells never resolve"):
        op.apply(words)
    with pytest.raises(ValueError, match="40 cells never resolve"):
        accumulate_ref(words)
    # a cell that the ring drains into through a share never resolves either
    words[10, 60] = mfd.pack(True, 0, [5] + none[1:])     # (10, 60) also sends north-east
    with pytest.raises(ValueError, match="form a cycle: 41 cells never resolve"):
        op.apply(words)
    assert_accumulation(random_acyclic_words((40, 130), seed=1))


def test_weights_out_of_range_and_a_total_of_2_to_the_48_are_refused():
    words = random_acyclic_words((70, 90), seed=2)
    for bad, n in ((-1.0, 1), (np.inf, 2), (-np.inf, 3), (2.0 ** 15, 4)):
        weights = np.ones((70, 90), F32)
        weights[3, 3:3 + n] = bad
        with pytest.raises(ValueError, match=f"weights out of range in {n} cells"):
            hd.MFDFlowAccumulation(weights=weights).apply(words)
        with pytest.raises(ValueError, match=f"weights out of range in {n} cells"):
            accumulate_ref(words, weights, 16)
    weights = np.full((70, 90), 2 ** 15, np.uint32)
    with pytest.raises(ValueError, match="weights out of range in 6300 cells"):
        hd.MFDFlowAccumulation(weights=weights).apply(words)
    # 131 769 cells of (2^15 - 1) << 16 each: 2^48 and a little
    shape = (363, 363)
    heavy = np.full(shape, 2 ** 15 - 1, np.uint32)
    total = shape[0] * shape[1] * ((2 ** 15 - 1) << 16)
    assert total >= 2 ** 48
    with pytest.raises(ValueError, match=f"the quantised weights sum to {total}: the total must"):
        hd.MFDFlowAccumulation(weights=heavy).apply(np.zeros(shape, np.uint64))
    assert_accumulation(words, weights=np.ones((70, 90), F32))


def test_an_output_of_the_wrong_dtype_is_refused_and_the_c_entry_points_check_their_arguments():
    words = random_acyclic_words((20, 30), seed=4)
    z = random_dem((20, 30), seed=4)
    ctx = backend.context()
    dev_flag = mfd.ON_DEVICE
    with DeviceRaster.from_host(words, dtype=np.uint64) as dw, \
            DeviceRaster.from_host(z, dtype=F32) as dz, \
            DeviceRaster.empty(words.shape, np.uint32, ctx) as wrong, \
            DeviceRaster.empty((20, 31), np.int64, ctx) as wide, \
            DeviceRaster.empty(words.shape, np.int64, ctx) as right, \
            DeviceRaster.empty(words.shape, np.uint64, ctx) as made:
        with pytest.raises(ValueError, match=r"out\['sum'\] is int64, got uint32"):
            mfd.mfdacc_dev(dw, want="sum", out={"sum": wrong})
        with pytest.raises(ValueError, match=r"out\['sum'\] is \(20, 31\), the words \(20, 30\)"):
            mfd.mfdacc_dev(dw, want="sum", out={"sum": wide})
        with pytest.raises(ValueError, match="out has value, which is not wanted"):
            mfd.mfdacc_dev(dw, want="sum", out={"value": right})
        with pytest.raises(ValueError, match="out is uint64, got uint32"):
            mfd.mfd_dev(dz, out=wrong)
        outs, _ = mfd.mfdacc_dev(dw, want="sum", out={"sum": right})
        assert outs["sum"] is right and np.array_equal(right.to_host(), accumulate_ref(words))
        got, _, _ = mfd.mfd_dev(dz, out=made)
        assert got is made and np.array_equal(made.to_host(), direction_ref(z)[0])

        fn = ctx.lib.hdem_mfdacc_u64
        call = lambda frac, s, v, flags, st, wt=0: fn(      # noqa: E731
            ctx.handle, dw.ptr, 20, 30, None, wt, frac, s, v, flags, st)
        assert call(16, None, None, dev_flag, None) == backend.BAD_ARG
        assert b"no output wanted" in ctx.lib.hdem_last_error()
        assert call(17, right.ptr, None, dev_flag, None) == backend.BAD_ARG
        assert b"frac_bits is 0 ... 16, got 17" in ctx.lib.hdem_last_error()
        for flags in (1, dev_flag | 2, -1):
            assert call(16, right.ptr, None, flags, None) == backend.BAD_ARG
            assert b"unknown flags" in ctx.lib.hdem_last_error()
        assert call(16, right.ptr, None, dev_flag, None, 1) == backend.BAD_ARG
        assert b"weight type 1 without a weight raster" in ctx.lib.hdem_last_error()
        assert fn(ctx.handle, dw.ptr, 20, 30, dw.ptr, 7, 16, right.ptr, None, dev_flag,
                  None) == backend.BAD_ARG
        assert b"unknown weight type 7" in ctx.lib.hdem_last_error()
        assert fn(ctx.handle, dw.ptr, 20, 30, None, 0, 16, dw.ptr, None, dev_flag,
                  None) == backend.BAD_ARG
        assert b"sum overlaps words" in ctx.lib.hdem_last_error()
        st = backend._MFDAccStats()                        # pylint: disable=protected-access
        st.struct_size = 0
        assert call(16, right.ptr, None, dev_flag, ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend._MFDAccStats()                        # pylint: disable=protected-access
        st.struct_size = 24                                # a shorter struct
        st.terminal_cells, st.tile_h = -5, -7
        assert call(16, right.ptr, None, dev_flag, ctypes.byref(st)) == backend.OK
        assert st.struct_size == 24 and st.split_cells == counts_of(words)["split_cells"]
        assert st.terminal_cells == -5 and st.tile_h == -7   # nothing beyond it is written
        fake = ctypes.c_void_p(256)                        # never dereferenced
        for flags in (0, dev_flag):
            assert fn(ctx.handle, fake, 65536, 65536, None, 0, 16, fake, None, flags,
                      None) == backend.BAD_ARG
            assert b"2^32" in ctx.lib.hdem_last_error()

        fn = ctx.lib.hdem_mfd_f32
        direct = lambda dx, e, wc, wd, out, flags, st=None: fn(    # noqa: E731
            ctx.handle, dz.ptr, 20, 30, None, dx, 1.0, e, wc, wd, out, None, flags, st)
        for flags in (0, dev_flag):
            assert direct(0.0, 1.1, 1.0, 1.0, made.ptr, flags) == backend.BAD_ARG
            assert b"dx and dy must be finite and positive" in ctx.lib.hdem_last_error()
            for e in (0.2, 16.5, float("nan")):
                assert direct(1.0, e, 1.0, 1.0, made.ptr, flags) == backend.BAD_ARG
                assert b"the exponent is 0.25 ... 16" in ctx.lib.hdem_last_error()
            assert direct(1.0, 1.1, 0.0, 1.0, made.ptr, flags) == backend.BAD_ARG
            assert direct(1.0, 1.1, 1.0, float("inf"), made.ptr, flags) == backend.BAD_ARG
            assert b"w_card and w_diag must be finite and positive" in ctx.lib.hdem_last_error()
            assert direct(1.0, 1.1, 1.0, 1.0, None, flags) == backend.BAD_ARG
            assert direct(1.0, 1.1, 1.0, 1.0, made.ptr, flags | 4) == backend.BAD_ARG
            assert b"unknown flags" in ctx.lib.hdem_last_error()
        st = backend._MFDStats()                           # pylint: disable=protected-access
        st.struct_size = 16                                # up to no_flow
        st.fallback_cells = -9
        assert direct(1.0, 1.1, 1.0, 1.0, made.ptr, dev_flag, ctypes.byref(st)) == backend.OK
        assert st.no_flow == direction_ref(z)[2]["no_flow"] and st.fallback_cells == -9
    # the context is as usable as before
    assert_accumulation(words)


# ---------------------------------------------------------------------------
# poisoned scratch and output memory, and a caller's stream
# ---------------------------------------------------------------------------
def poison_words(shape, seed=33):
    return {"words": random_acyclic_words(shape, seed=seed)}


def poison_dem(shape, seed=33):
    return {"z": random_dem(shape, seed=seed, nan=0.01)}


def poison_run_acc(call, inp):
    """The accumulation for ``value`` alone (the arena's working raster), then for both outputs
    (the caller's or the library's sum as working raster), then weighted."""
    words = inp["words"]
    dw = call.up(words)
    out = {name: call.out(words.shape, dtype) for name, dtype in mfd.OUTPUTS}
    alone, _ = mfd.mfdacc_dev(dw, None, 16, "value", {"value": out["value"]} if call.own else None)
    host = {"alone": alone["value"].to_host()}
    if not call.own:
        call.stack.enter_context(alone["value"])
    dev, stats = mfd.mfdacc_dev(dw, None, 16, ("sum", "value"), out if call.own else None)
    for name, raster in dev.items():
        assert not call.own or raster is out[name]
        host[name] = call.host(raster)
    weights = call.up((words % np.uint64(251)).astype(np.uint8))
    heavy, heavy_stats = mfd.mfdacc_dev(dw, weights, 8, "sum")
    host["weighted"] = call.host(heavy["sum"])
    return host, dict(schedule_free(stats), total=heavy_stats["total"])


def poison_check_acc(inp, got):
    words = inp["words"]
    assert np.array_equal(got["sum"], accumulate_ref(words))
    assert np.array_equal(got["alone"], got["value"])
    assert np.array_equal(got["weighted"],
                          accumulate_ref(words, (words % np.uint64(251)).astype(np.uint8), 8))


def poison_run_direction(call, inp):
    """The direction for the words and the slope, at an exponent that takes the power."""
    dz = call.up(inp["z"])
    made, extras, stats = mfd.mfd_dev(dz, "freeman", None, 1.0, None, mfd.EXTRAS,
                                      call.out(dz.shape, np.uint64))
    host = {name: call.host(raster) for name, raster in {"words": made, **extras}.items()}
    return host, without_times(stats)


def poison_check_direction(inp, got):
    want_words, want_slope, _ = direction_ref(inp["z"])
    assert got["words"].dtype == np.uint64 and np.array_equal(got["words"], want_words)
    assert np.array_equal(got["slope"].view(np.uint32), want_slope.view(np.uint32))


POISON_CASES = [Case("mfdacc", ((130, 197),), poison_words, poison_run_acc, poison_check_acc,
                     True, frozenset()),
                Case("mfd-direction", ((130, 197), WIDE), poison_dem, poison_run_direction,
                     poison_check_direction, True, frozenset())]
POISON_PARAMS = [(entry, shape) for entry in POISON_CASES for shape in entry.shapes]
POISON_IDS = [f"{entry.name}-{IDS(shape)}" for entry, shape in POISON_PARAMS]


@pytest.fixture(scope="module")
def clean_runs():
    """Inputs and the run on a fresh context's own stream, once per case, shape and ``own``."""
    runs = {}

    def run(entry, shape, own):
        key = (entry.name, shape, own)
        if key not in runs:
            inputs = entry.build(shape)
            got, stats = execute(entry, inputs, None, own)
            entry.check(inputs, got)
            runs[key] = (inputs, got, stats)
        return runs[key]
    return run


@pytest.mark.parametrize("entry,shape", POISON_PARAMS, ids=POISON_IDS)
@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
def test_poisoned_memory_changes_no_byte(clean_runs, entry, shape, own):
    inputs, clean, clean_stats = clean_runs(entry, shape, own)
    for byte in (0x00, 0xA5, 0xFF):
        got, stats = execute(entry, inputs, byte, own)
        assert stats == clean_stats
        assert_same_bytes(got, clean, f"{entry.name} {shape} under {byte:#04x}")


@pytest.fixture(scope="module")
def delay():
    return Delay()


@pytest.mark.parametrize("entry,shape", [(POISON_CASES[0], (130, 197)), (POISON_CASES[1], WIDE)],
                         ids=["mfdacc-130x197", "mfd-direction-33x257"])
def test_a_callers_stream_behind_an_unfinished_producer_changes_no_byte(clean_runs, entry, shape,
                                                                        delay):
    inputs, want, want_stats = clean_runs(entry, shape, False)
    got, stats = on_a_callers_stream(entry, inputs, want, False)
    assert_same_bytes(got, want, f"{entry.name} {shape} on an idle stream of the caller's")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} {shape} behind the delay, out= {whose}"
        got, stats = on_a_callers_stream(entry, inputs, want, own, delay)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
