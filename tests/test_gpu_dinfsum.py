"""
Weighted D-infinity flow accumulation on the MI355X (``WeightedDInfFlowAccumulation``,
``hdem_dinfsum_u32[_dev]``).

The definition and the host references are those of tests/test_dinfsum.py and tests/test_dinf.py;
every comparison is ``np.array_equal`` or byte equality.  The weights differ from cell to cell, so
an own term that lands in the wrong cell shows; the shapes are those at which the tile structure
of the accumulation can go wrong (tests/test_gpu_dinf.py) plus the two strips.
"""
import ctypes

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, dinf, flowsum
from hydrodem_amd.backend import DeviceRaster
from test_dinf import accumulate_ref, counts_of, direction_ref, random_dem, value_of
from test_dinfsum import accumulate_weighted_ref, random_weights
from test_flowacc import random_acyclic_codes, terminal_mask
from test_gpu_dinf import random_acyclic_words, schedule_free
from test_gpu_flowacc import path_codes
from test_gpu_scribble import Case, execute

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (2, 9), (3, 3), (64, 64), (65, 63), (130, 197), (1, 200), (65, 1)]
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731
WEIGHTS = [(np.float32, 0), (np.float32, 10), (np.float32, 30), (np.uint8, 0), (np.uint8, 16),
           (np.uint32, 0), (np.uint32, 16)]
Q_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


def assert_weighted(words, weights, frac_bits, want=None):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    q = dinf.quantise(weights, frac_bits)
    assert 0 <= q.min() and q.max() <= Q_MAX
    want = accumulate_weighted_ref(words, q) if want is None else want
    outs, stats = dinf.dinfsum(words, weights, frac_bits, ("sum", "value"))
    assert outs["sum"].dtype == np.int64 and outs["value"].dtype == F32
    assert np.array_equal(outs["sum"], want)
    assert outs["value"].tobytes() == value_of(want, frac_bits).tobytes()
    assert schedule_free(stats) == counts_of(words)
    nan = int(np.isnan(weights).sum()) if weights.dtype == F32 else 0
    assert stats["nan_weights"] == nan and stats["bad_weights"] == 0
    assert stats["total"] == int(q.sum()) == int(want[words >> 16 == 0].sum())
    assert stats["rounds"] >= 1 and "struct_size" not in stats
    return outs, stats


@pytest.mark.parametrize("source", ["direction", "acyclic"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_weight_type_against_the_reference(shape, source):
    seed = shape[0] * 7 + shape[1]
    if source == "direction":
        words, _, _, _ = direction_ref(random_dem(shape, seed=seed, nan=0.01))
    else:
        words = random_acyclic_words(shape, seed=seed)
    for k, (dtype, frac_bits) in enumerate(WEIGHTS):
        weights = random_weights(shape, seed + k, dtype, nan=0.05)
        assert_weighted(words, weights, frac_bits)


@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles(upright):
    n = 4097
    codes = np.zeros((5, n), np.uint8)
    codes[2, :n - 1] = 1                                  # eastwards
    weights = random_weights((5, n), 4, F32)
    if upright:
        codes = np.ascontiguousarray(np.where(codes.T, 4, 0).astype(np.uint8))
        weights = np.ascontiguousarray(weights.T)
    q = dinf.quantise(weights, 16)
    want = q.copy()
    line = np.cumsum(q[:, 2] if upright else q[2])
    if upright:
        want[:, 2] = line
    else:
        want[2] = line
    _, stats = assert_weighted(dinf.words_from_d8(codes), weights, 16, want)
    assert stats["rounds"] > 1 and stats["terminal_cells"] == 4 * n + 1


def test_a_zigzag_of_1000_diagonal_steps_along_a_tile_seam():
    cells = [(k, 63 + k % 2) for k in range(1001)]         # crosses column 63 | 64 every step
    words = dinf.words_from_d8(path_codes((1001, 128), cells))
    weights = random_weights((1001, 128), 8, np.uint32)
    q = dinf.quantise(weights, 3)
    want = q.copy()
    run = 0
    for y, x in cells:
        run += int(q[y, x])
        want[y, x] = run
    _, stats = assert_weighted(words, weights, 3, want)
    assert stats["rounds"] > 1


@pytest.mark.parametrize("frac_bits", [0, 7, 16])
def test_unit_weights_give_the_bytes_of_the_unweighted_operator(frac_bits):
    words = random_acyclic_words((130, 197), seed=12)
    ones = np.ones(words.shape, np.uint8)
    got, stats = dinf.dinfsum(words, ones, frac_bits, ("sum", "value"))
    want, want_stats = dinf.dinfacc(words, frac_bits, ("sum", "value"))
    for name in ("sum", "value"):
        assert got[name].tobytes() == want[name].tobytes()
    assert schedule_free(stats) == schedule_free(want_stats)
    assert stats["total"] == words.size << frac_bits
    assert np.array_equal(want["sum"], accumulate_ref(words, frac_bits))


def test_canonical_words_give_the_weighted_d8_sum():
    codes = random_acyclic_codes(150, 210, seed=5, ramp=True)
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    words = dinf.words_from_d8(codes)
    for weights, frac_bits in ((random_weights(codes.shape, 1, F32, nan=0.02), 10),
                               (random_weights(codes.shape, 2, np.uint32), 0),
                               (random_weights(codes.shape, 3, np.uint8), 0)):
        want, _ = flowsum.flowsum(codes, weights, frac_bits, "sum")
        got = hd.WeightedDInfFlowAccumulation(weights, frac_bits, "sum").apply(words)
        assert got.tobytes() == want["sum"].tobytes()


def test_two_runs_and_both_forms_give_identical_bytes():
    words = random_acyclic_words((257, 130), seed=21)
    weights = random_weights(words.shape, 21, F32, nan=0.03)
    a, stats_a = dinf.dinfsum(words, weights, 16, ("sum", "value"))
    b, _ = dinf.dinfsum(words, weights, 16, ("sum", "value"))
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.from_host(weights, dtype=F32) as dq:
        dev, stats_c = dinf.dinfsum_dev(dw, dq, 16, ("sum", "value"))
        with dev["sum"] as ds, dev["value"] as dv:
            c = {"sum": ds.to_host(), "value": dv.to_host()}
        # one output at a time: the working raster is then the arena's, or the caller's sum
        for name in ("value", "sum"):
            op = hd.WeightedDInfFlowAccumulation(dq, output=name)
            with op.apply_device(dw) as one:
                assert one.dtype == a[name].dtype and one.to_host().tobytes() == a[name].tobytes()
            assert op.apply(words).tobytes() == a[name].tobytes()
            assert op.stats["total"] == stats_a["total"]
    for name in ("sum", "value"):
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes()
    assert schedule_free(stats_a) == schedule_free(stats_c)
    assert np.array_equal(a["sum"], accumulate_weighted_ref(words, dinf.quantise(weights, 16)))


# ---------------------------------------------------------------------------
# poisoned scratch and output memory
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=33):
    words = random_acyclic_words(shape, seed=seed)
    return {"words": words, "weights": random_weights(words.shape, seed, F32, nan=0.02)}


def poison_run(call, inp):
    """The device call for ``value`` alone (the arena's working raster) and for both outputs (the
    caller's or the library's ``sum`` as working raster)."""
    words = inp["words"]
    dw, dq = call.up(words), call.up(inp["weights"])
    out = {name: call.out(words.shape, dtype) for name, dtype in dinf.OUTPUTS}
    alone, _ = dinf.dinfsum_dev(dw, dq, 16, "value", {"value": out["value"]} if call.own else None)
    host = {"alone": alone["value"].to_host()}
    if not call.own:
        call.stack.enter_context(alone["value"])
    dev, stats = dinf.dinfsum_dev(dw, dq, 16, ("sum", "value"), out if call.own else None)
    for name, raster in dev.items():
        assert not call.own or raster is out[name]
        host[name] = call.host(raster)
    return host, stats


def poison_check(inp, got):
    assert np.array_equal(got["sum"], accumulate_weighted_ref(inp["words"],
                                                              dinf.quantise(inp["weights"], 16)))
    assert np.array_equal(got["alone"], got["value"])


# rounds, tile_visits: a tile reads what its neighbours write in the same launch
POISON_CASE = Case("dinfsum", ((130, 197),), poison_inputs, poison_run, poison_check, True,
                   frozenset(("rounds", "tile_visits")))


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
def test_poisoned_memory_changes_no_byte(own):
    inp = POISON_CASE.build((130, 197))
    clean, clean_stats = execute(POISON_CASE, inp, None, own)
    POISON_CASE.check(inp, clean)
    for byte in (0x00, 0xFF):           # 0xFF: FINAL set in every word classify does not write
        got, stats = execute(POISON_CASE, inp, byte, own)
        assert stats == clean_stats
        for name, raster in clean.items():
            assert got[name].tobytes() == raster.tobytes(), (name, hex(byte))


# ---------------------------------------------------------------------------
# refusals: the context stays usable
# ---------------------------------------------------------------------------
def c_call(ctx, fn, words, weights, weight_type, frac_bits, h=None, w=None, sum_=None,
           value=None, flags=0):
    """One call of the C entry ``fn`` on device rasters (or raw addresses): status, the text and
    the stats struct."""
    st = backend._DInfSumStats()                          # pylint: disable=protected-access
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ptr   # noqa: E731
    h, w = (h, w) if h else words.shape
    rc = fn(ctx.handle, ptr(words), h, w, ptr(weights), weight_type, frac_bits,
            ptr(sum_), ptr(value), flags, ctypes.byref(st))
    return rc, ctx.lib.hdem_last_error().decode(), st


def test_weights_out_of_range_are_refused_with_their_count():
    words = random_acyclic_words((70, 90), seed=2)
    weights = random_weights(words.shape, 2, F32)
    bad = weights.copy()
    bad[3, 66], bad[69, 0] = -1.0, -np.inf
    bad[40, 64] = np.inf
    bad[0, 89] = 32768.5                                  # q = 2^31 + 2^15 at frac_bits 16
    bad[5, 5] = -0.0                                      # counts 0: no refusal
    text = "weights out of range in 4 cells: 2 negative, 1 infinite, 1 above 2\\^31 - 1"
    with pytest.raises(ValueError, match=text):
        hd.WeightedDInfFlowAccumulation(bad).apply(words)
    ctx = backend.context()
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.from_host(bad, dtype=F32) as dq, \
            DeviceRaster.empty(words.shape, np.int64, ctx) as ds:
        with pytest.raises(ValueError, match=text):
            hd.WeightedDInfFlowAccumulation(dq, output="sum").apply_device(dw)
        rc, said, st = c_call(ctx, ctx.lib.hdem_dinfsum_u32_dev, dw, dq, 1, 16, sum_=ds)
        assert rc == backend.BAD_ARG and "frac_bits 16" in said and st.bad_weights == 4
        assert st.rounds == 0 and st.tile_visits == 0      # refused after classify
    whole = np.full(words.shape, Q_MAX, np.uint32)
    whole[1, 1], whole[2, 2] = Q_MAX + 1, 0xFFFFFFFF
    with pytest.raises(ValueError, match="in 2 cells: 0 negative, 0 infinite, 2 above"):
        hd.WeightedDInfFlowAccumulation(whole, 0).apply(words)
    with pytest.raises(ValueError, match=f"in {int((whole > 32767).sum())} cells"):
        hd.WeightedDInfFlowAccumulation(whole, 16).apply(words)
    # 2^31 - 1 itself is taken
    whole[1, 1] = whole[2, 2] = Q_MAX
    assert_weighted(words, whole, 0)
    assert_weighted(words, weights, 16)


@pytest.mark.parametrize("shape,refused", [((1, 131072), False), ((1, 131073), True),
                                           ((363, 363), True)], ids=str)
def test_a_total_of_2_48_or_more_is_refused(shape, refused):
    """2^17 + 1 cells of 2^31 - 1 are the fewest that reach 2^48; one fewer stays below it."""
    ctx = backend.context()
    n = shape[0] * shape[1]
    with DeviceRaster.from_host(np.zeros(shape, np.uint32), dtype=np.uint32) as dw, \
            DeviceRaster.from_host(np.full(shape, Q_MAX, np.uint32), dtype=np.uint32) as dq, \
            DeviceRaster.empty(shape, np.int64, ctx) as ds:
        rc, said, st = c_call(ctx, ctx.lib.hdem_dinfsum_u32_dev, dw, dq, 2, 0, sum_=ds)
        assert st.total == n * Q_MAX and (st.total >= 2 ** 48) == refused
        if refused:
            assert rc == backend.BAD_ARG and st.rounds == 0
            assert said == (f"the quantised weights sum to {n * Q_MAX}: the total must stay below "
                            "2^48 (frac_bits 0)")
        else:
            assert rc == backend.OK and (ds.to_host() == Q_MAX).all()


def test_invalid_words_and_cycles_are_still_refused():
    words = random_acyclic_words((70, 90), seed=2)
    weights = random_weights(words.shape, 2, F32)
    bad = words.copy()
    bad[5:8, 66] = 9 << 16
    with pytest.raises(ValueError, match="invalid D-infinity word in 3 cells: the facet"):
        hd.WeightedDInfFlowAccumulation(weights).apply(bad)
    out = np.zeros((66, 70), np.uint32)
    out[0, 3] = dinf.pack(2, 0)
    with pytest.raises(ValueError, match="send flow outside the raster in 1 cells"):
        hd.WeightedDInfFlowAccumulation(np.ones(out.shape, np.uint8)).apply(out)
    loop = np.zeros((40, 130), np.uint32)
    loop[7, 63:65] = dinf.pack(np.array([1, 4]), np.array([0, 0]))     # E then W over a seam
    with pytest.raises(ValueError, match="form a cycle: 2 cells never resolve"):
        hd.WeightedDInfFlowAccumulation(np.ones(loop.shape, F32)).apply(loop)
    # invalid words come first in the text, bad weights after
    weights[0, 0] = -1
    with pytest.raises(ValueError, match="invalid D-infinity word in 3 cells"):
        hd.WeightedDInfFlowAccumulation(weights).apply(bad)
    assert_weighted(words, random_weights(words.shape, 3, np.uint8), 16)


def test_overlapping_pointers_wrong_dtypes_and_the_other_checks_of_the_c_entry():
    words = random_acyclic_words((20, 30), seed=4)
    weights = random_weights(words.shape, 4, F32)
    ctx = backend.context()
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.from_host(weights, dtype=F32) as dq, \
            DeviceRaster.empty(words.shape, np.uint32, ctx) as wrong, \
            DeviceRaster.empty(words.shape, np.int64, ctx) as right, \
            DeviceRaster.empty(words.shape, F32, ctx) as dv:
        with pytest.raises(ValueError, match=r"out\['sum'\] is int64, got uint32"):
            dinf.dinfsum_dev(dw, dq, want="sum", out={"sum": wrong})
        with pytest.raises(ValueError, match="out has value, which is not wanted"):
            dinf.dinfsum_dev(dw, dq, want="sum", out={"value": dv})
        with pytest.raises(ValueError, match="the weights are float32, uint32 or uint8, got int64"):
            dinf.dinfsum_dev(dw, right)
        fn = ctx.lib.hdem_dinfsum_u32_dev
        for kw, text in (
                (dict(sum_=None), "no output wanted"),
                (dict(weights=None), "the weight raster is null"),
                (dict(weight_type=0), "unknown weight type 0"),
                (dict(weight_type=4), "unknown weight type 4"),
                (dict(frac_bits=31), "frac_bits is 0 ... 30, got 31"),
                (dict(frac_bits=-1), "frac_bits is 0 ... 30, got -1"),
                (dict(weight_type=2, frac_bits=17), "integer weights take frac_bits 0 ... 16, got 17"),
                (dict(weight_type=3, frac_bits=17), "integer weights take frac_bits 0 ... 16, got 17"),
                (dict(flags=1), "unknown flags 0x1"),
                (dict(sum_=dw.ptr), "sum overlaps words"),
                (dict(sum_=None, value=dw.ptr), "value overlaps words"),
                (dict(sum_=None, value=dq.ptr), "value overlaps weights"),
                (dict(sum_=None, value=dq.ptr + 4 * (words.size - 1)), "value overlaps weights"),
                (dict(value=right.ptr + 8), "value overlaps sum"),
                (dict(h=65536, w=65536), "2^32")):
            args = dict(words=dw, weights=dq, weight_type=1, frac_bits=16, sum_=right)
            args.update(kw)
            rc, said, _ = c_call(ctx, fn, **args)
            assert rc == backend.BAD_ARG and text in said, (kw, said)
        st = backend._DInfSumStats()                       # pylint: disable=protected-access
        st.struct_size = 0
        assert fn(ctx.handle, dw.ptr, 20, 30, dq.ptr, 1, 16, right.ptr, None, 0,
                  ctypes.byref(st)) == backend.BAD_ARG
        assert b"hdem_dinfsum_stats.struct_size" in ctx.lib.hdem_last_error()
        st = backend._DInfSumStats()                       # pylint: disable=protected-access
        st.struct_size = 80                                # only the unweighted fields
        st.nan_weights, st.total = -5, 7
        assert fn(ctx.handle, dw.ptr, 20, 30, dq.ptr, 1, 16, right.ptr, dv.ptr, 0,
                  ctypes.byref(st)) == backend.OK
        assert st.struct_size == 80 and st.split_cells == counts_of(words)["split_cells"]
        assert st.nan_weights == -5 and st.total == 7       # nothing beyond it is written
        want = accumulate_weighted_ref(words, dinf.quantise(weights, 16))
        assert np.array_equal(right.to_host(), want)
        assert dv.to_host().tobytes() == value_of(want, 16).tobytes()


def test_profiling_fills_the_phase_times():
    words = random_acyclic_words((300, 300), seed=9)
    op = hd.WeightedDInfFlowAccumulation(random_weights(words.shape, 9, F32))
    op.apply(words)
    assert op.stats["ms_classify"] == 0 and op.stats["ms_relax"] == 0 and op.stats["ms_final"] == 0
    ctx = backend.context()
    ctx.profile(True)
    try:
        op.apply(words)
    finally:
        ctx.profile(False)
    assert op.stats["ms_classify"] > 0 and op.stats["ms_relax"] > 0 and op.stats["ms_final"] > 0
