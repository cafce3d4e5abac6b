"""
Weighted D8 flow accumulation on the MI355X (``WeightedFlowAccumulation``,
``hdem_flowsum_u8[_dev]``): unit weights against ``FlowAccumulation``, random weights against
the int64 Kahn reference of tests/test_flowsum.py, sums that carry past 2^32 inside a tile and
across many, marked points, the ``value`` and ``mask`` formulas bit for bit, host / device /
repeat equality, poisoned scratch and output memory, and the refusals, each followed by a
correct call on the same context.
"""
import ctypes
import functools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, flowsum
from hydrodem_amd.backend import DeviceRaster
from test_flowacc import random_acyclic_codes
from test_flowsum import downstream_union, wsum_kahn
from test_gpu_flowacc import E, N, S, W_, path_codes, snake
from test_gpu_scribble import Case, execute

pytestmark = pytest.mark.gpu

Q_MAX = 2 ** 31 - 1
# one cell; below, at and above one tile; partial tiles in both directions; strips; 3 x 4 tiles
SHAPES = [(1, 1), (63, 63), (64, 64), (65, 65), (127, 129), (7, 1000), (130, 197)]
CASES = [(shape, ramp) for shape in SHAPES for ramp in (False, True)] + [((4097, 300), True)]
CASE_IDS = [f"{h}x{w}-{'ramp' if ramp else 'noise'}" for (h, w), ramp in CASES]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


@functools.lru_cache(maxsize=None)
def codes_of(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def unweighted(shape, ramp):
    acc = hd.FlowAccumulation().apply(codes_of(shape, ramp))
    acc.setflags(write=False)
    return acc


def sums(codes, weights, frac_bits=0):
    outs, stats = flowsum.flowsum(np.ascontiguousarray(codes), weights, frac_bits, "sum")
    assert outs["sum"].dtype == np.int64 and outs["sum"].shape == codes.shape
    return outs["sum"], stats


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# unit weights: the count of cells
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ramp", CASES, ids=CASE_IDS)
def test_unit_weights_count_cells(shape, ramp):
    codes, want = codes_of(shape, ramp), unweighted(shape, ramp).astype(np.int64)
    for dtype in (np.uint8, np.uint32, np.float32):
        got, stats = sums(codes, np.ones(shape, dtype))
        assert np.array_equal(got, want), dtype
        assert stats["nan_weights"] == 0 and stats["tile_h"] == 64 and stats["tile_w"] == 64


# ---------------------------------------------------------------------------
# random weights against the Kahn reference
# ---------------------------------------------------------------------------
def random_weights(kind, shape, rng):
    """The weights and frac_bits of one kind of the issue's list."""
    if kind == "u32":
        w = rng.integers(0, 2 ** 31, size=shape, dtype=np.int64).astype(np.uint32)
        w.flat[0] = Q_MAX                                       # the bound itself
        return w, 0
    if kind == "u8":
        return rng.integers(0, 256, size=shape, dtype=np.int64).astype(np.uint8), 0
    frac_bits = int(kind[1:].rstrip("n"))
    w = (rng.random(shape, dtype=np.float32) * np.float32(2.0 if frac_bits == 30 else 100.0))
    w = np.minimum(w, np.nextafter(np.float32(2.0 if frac_bits == 30 else 100.0), np.float32(0)))
    if kind.endswith("n"):                                      # 1 % NaN
        w[rng.random(shape) < 0.01] = np.nan
        w.flat[0] = np.nan
    return w, frac_bits


@pytest.mark.parametrize("kind", ["u32", "u8", "f0", "f16", "f30", "f16n"])
@pytest.mark.parametrize("shape,ramp", CASES, ids=CASE_IDS)
def test_random_weights_match_the_kahn_reference(shape, ramp, kind):
    codes = codes_of(shape, ramp)
    rng = np.random.default_rng(shape[0] * 13 + shape[1] + 1000 * ramp)
    w, frac_bits = random_weights(kind, shape, rng)
    q = flowsum.quantise(w, frac_bits)
    assert q.min() >= 0 and q.max() <= Q_MAX
    got, stats = sums(codes, w, frac_bits)
    assert np.array_equal(got, wsum_kahn(codes, q))
    nans = int(np.isnan(w).sum()) if w.dtype == np.float32 else 0
    assert stats["nan_weights"] == nans
    assert nans > 0 or not kind.endswith("n")


# ---------------------------------------------------------------------------
# carries
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_carry_past_32_bits():
    want = np.arange(1, 10001, dtype=np.int64) * Q_MAX          # 2^32 inside the first tile
    assert want[2] > 2 ** 32 and want[-1] > 2 ** 44
    got, stats = sums(np.full((1, 10000), E, np.uint8), np.full((1, 10000), Q_MAX, np.uint32))
    assert np.array_equal(got[0], want)
    assert stats["exits"] == 156 and stats["max_hops"] >= 155  # 156 tile crossings
    got, _ = sums(np.full((10000, 1), S, np.uint8), np.full((10000, 1), Q_MAX, np.uint32))
    assert np.array_equal(got[:, 0], want)


def test_a_snake_through_every_tile_against_the_closed_form():
    cells = snake(512, 512)
    codes = path_codes((512, 512), cells)
    k = np.arange(len(cells), dtype=np.int64)
    ys, xs = np.array(cells).T
    w = np.zeros((512, 512), np.uint8)
    w[ys, xs] = k % 251
    # sum of j mod 251 for j <= k: whole periods, then 0 + 1 + ... + k mod 251
    want = np.zeros((512, 512), np.int64)
    want[ys, xs] = (k // 251) * (250 * 251 // 2) + (k % 251) * (k % 251 + 1) // 2
    got, stats = sums(codes, w)
    assert np.array_equal(got, want)
    assert stats["max_hops"] >= 63


# ---------------------------------------------------------------------------
# marked points; value and mask
# ---------------------------------------------------------------------------
def test_marked_points_mask_their_downstream_paths():
    codes = random_acyclic_codes(300, 300, seed=21, ramp=True)
    cells = np.random.default_rng(4).choice(codes.size, 20, replace=False)
    w = np.zeros(codes.size, np.uint8)
    w[cells] = 1
    f = hd.WeightedFlowAccumulation(w.reshape(codes.shape), 0, "mask", 1)
    got = f.apply(codes)
    assert got.dtype == np.uint8
    want = downstream_union(codes, cells)
    assert want.sum() > 20
    assert np.array_equal(got, want)


@pytest.mark.parametrize("frac_bits,threshold", [(0, 700), (16, 650.25), (30, 1.5)])
def test_value_and_mask_are_the_numpy_formulas_of_the_sum(frac_bits, threshold):
    shape = (127, 129)
    codes = codes_of(shape, True)
    w, _ = random_weights(f"f{frac_bits}", shape, np.random.default_rng(frac_bits))
    outs, _ = flowsum.flowsum(codes, w, frac_bits, ("sum", "value", "mask"), threshold)
    total = outs["sum"]
    assert np.array_equal(total, wsum_kahn(codes, flowsum.quantise(w, frac_bits)))
    assert total.max() > 2 ** 24 or frac_bits == 0             # value really rounds
    want = (total.astype(np.float64) * 2.0 ** -frac_bits).astype(np.float32)
    assert same_bytes(outs["value"], want)
    units = int(np.ceil(threshold * 2.0 ** frac_bits))
    want_mask = (total >= units).astype(np.uint8)
    assert 0 < want_mask.sum() < want_mask.size
    assert same_bytes(outs["mask"], want_mask)
    # any subset holds the bytes the call for all of them writes
    for name in ("value", "mask"):
        alone, _ = flowsum.flowsum(codes, w, frac_bits, name,
                                   threshold if name == "mask" else None)
        assert list(alone) == [name] and same_bytes(alone[name], outs[name])
    # the filter returns the same three
    for name in ("sum", "value", "mask"):
        f = hd.WeightedFlowAccumulation(w, frac_bits, name, threshold if name == "mask" else None)
        got = f.apply(codes)
        assert got.dtype == f.dtype and same_bytes(got, outs[name])


def test_the_mask_goes_into_streamorder_as_a_host_mask_does():
    shape = (130, 197)
    codes = codes_of(shape, True)
    w, _ = random_weights("f16", shape, np.random.default_rng(8))
    host_mask = hd.WeightedFlowAccumulation(w, 16, "mask", 900.0).apply(codes)
    assert 0 < host_mask.sum() < host_mask.size
    want = hd.StreamOrder(host_mask).apply(codes)
    with DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        with hd.WeightedFlowAccumulation(w, 16, "mask", 900.0).apply_device(dc) as dmask:
            assert dmask.dtype == np.uint8
            with hd.StreamOrder(dmask).apply_device(dc) as order:
                got = order.to_host()
    assert want.max() >= 2
    assert same_bytes(got, want)


# ---------------------------------------------------------------------------
# host form, device form, a repeat; the chain
# ---------------------------------------------------------------------------
def test_host_and_device_forms_and_a_repeat_are_byte_equal():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    w, _ = random_weights("f16n", codes.shape, np.random.default_rng(5))
    want = ("sum", "value", "mask")
    a, stats_a = flowsum.flowsum(codes, w, 16, want, 1000.0)
    b, _ = flowsum.flowsum(codes, w, 16, want, 1000.0)
    with DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            DeviceRaster.from_host(w, dtype=np.float32) as dw:
        dev, stats_c = flowsum.flowsum_dev(dc, dw, 16, want, 1000.0)
        c = {}
        for name, raster in dev.items():
            with raster:
                c[name] = raster.to_host()
    for name in want:
        assert same_bytes(a[name], b[name]) and same_bytes(a[name], c[name]), name
    for key in ("exits", "nan_weights", "tile_h", "tile_w"):
        assert stats_a[key] == stats_c[key]
    assert stats_a["exits"] > 0 and stats_a["max_hops"] > 0


def test_the_chain_from_a_dem_equals_the_staged_calls_and_the_reference():
    z = hdem_synth.synth_dem(1024, 1024)
    rain = np.random.default_rng(9).random(z.shape, dtype=np.float32) * np.float32(50.0)
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(epsilon=1e-3), hd.D8FlowDirection(),
                     hd.WeightedFlowAccumulation(rain)]
    got = chain.apply(z)
    assert got.dtype == np.float32
    codes = hd.D8FlowDirection().apply(hd.SinkFill(epsilon=1e-3).apply(z))
    staged = hd.WeightedFlowAccumulation(rain).apply(codes)
    assert same_bytes(got, staged)
    total = wsum_kahn(codes, flowsum.quantise(rain, 16))
    assert same_bytes(got, (total.astype(np.float64) * 2.0 ** -16).astype(np.float32))
    assert chain.filters[2].stats["exits"] > 0
    # and with the weights already on the device
    with DeviceRaster.from_host(rain, dtype=np.float32) as drain, \
            DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        with hd.WeightedFlowAccumulation(drain, output="sum").apply_device(dc) as dsum:
            assert dsum.dtype == np.int64
            assert np.array_equal(dsum.to_host(), total)


# ---------------------------------------------------------------------------
# poisoned scratch and output memory
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=None):
    codes = codes_of(shape, True) if shape[1] > 1 else np.full(shape, S, np.uint8)
    return {"codes": codes, "w": random_weights("f16n", shape, np.random.default_rng(shape[0]))[0]}


def poison_run(call, inp):
    """One device call for all three outputs."""
    codes = inp["codes"]
    dc, dw = call.up(np.ascontiguousarray(codes)), call.up(inp["w"])
    out = None
    if call.own:
        out = {name: call.out(codes.shape, dtype) for name, dtype in flowsum.FS_OUTPUTS}
    dev, stats = flowsum.flowsum_dev(dc, dw, 16, ("sum", "value", "mask"), 100.0, out=out)
    for name, raster in dev.items():
        assert not call.own or raster is out[name]
    return {name: call.host(raster) for name, raster in dev.items()}, stats


def poison_check(inp, got):
    assert np.array_equal(got["sum"], wsum_kahn(inp["codes"], flowsum.quantise(inp["w"], 16)))


POISON_SHAPES = [(130, 197), (65, 1)]
# max_hops: the walk that goes on at a node is the one whose atomic arrives last
POISON_CASE = Case("flowsum-all", tuple(POISON_SHAPES), poison_inputs, poison_run, poison_check,
                   True, frozenset(("max_hops",)))


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
@pytest.mark.parametrize("shape", POISON_SHAPES)
def test_poisoned_memory_changes_nothing(shape, own):
    inp = POISON_CASE.build(shape)
    clean, clean_stats = execute(POISON_CASE, inp, None, own)
    POISON_CASE.check(inp, clean)
    for byte in (0x00, 0xFF):                                   # 0x00 first
        got, stats = execute(POISON_CASE, inp, byte, own)
        for name in clean:
            assert same_bytes(got[name], clean[name]), (name, byte)
        assert stats == clean_stats, byte


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def check_the_next_call():
    cells = snake(130, 70)
    codes = path_codes((130, 70), cells)
    ys, xs = np.array(cells).T
    w = np.zeros((130, 70), np.float32)
    w[ys, xs] = 0.5
    want = np.zeros((130, 70), np.int64)
    want[ys, xs] = (np.arange(len(cells), dtype=np.int64) + 1) * 32768
    got, _ = sums(codes, w, 16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bad,frac_bits,words", [
    (-1e-3, 16, "1 negative"), (-np.inf, 16, "1 negative"), (np.inf, 16, "1 infinite"),
    (2.0 ** 15, 16, "1 above 2\\^31 - 1"), (2.0 ** 31, 0, "1 above 2\\^31 - 1")],
    ids=["negative", "minus_inf", "plus_inf", "2^15_at_16", "2^31_at_0"])
def test_weights_out_of_range_raise_with_their_count(bad, frac_bits, words):
    codes = codes_of((130, 197), True)
    w = np.ones(codes.shape, np.float32)
    w[77, 150] = bad
    with pytest.raises(ValueError, match="weights out of range in 1 cells.*" + words):
        sums(codes, w, frac_bits)
    check_the_next_call()
    w[77, 150] = -0.0                                           # counts as 0
    w[78, 150] = np.nextafter(np.float32(2.0 ** (31 - frac_bits)), np.float32(0))
    got, _ = sums(codes, w, frac_bits)
    assert np.array_equal(got, wsum_kahn(codes, flowsum.quantise(w, frac_bits)))


def test_integer_weights_above_the_bound_raise():
    codes = codes_of((65, 65), False)
    w = np.ones(codes.shape, np.uint32)
    w[3, 3], w[64, 64] = 2 ** 31, 2 ** 32 - 1
    with pytest.raises(ValueError, match="weights out of range in 2 cells.*2 above"):
        sums(codes, w)
    check_the_next_call()


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        sums(codes, np.ones(codes.shape, np.uint8))
    check_the_next_call()


def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="cycle"):
        sums(np.array([[E, W_]], np.uint8), np.ones((1, 2), np.float32), 16)
    check_the_next_call()
    codes = np.zeros((256, 256), np.uint8)               # clockwise round a 200 x 200 rim
    y0, x0, n = 10, 20, 200
    codes[y0, x0:x0 + n - 1] = E
    codes[y0:y0 + n - 1, x0 + n - 1] = S
    codes[y0 + n - 1, x0 + 1:x0 + n] = W_
    codes[y0 + 1:y0 + n, x0] = N
    assert int((codes != 0).sum()) == 796
    with pytest.raises(ValueError, match="cycle"):
        sums(codes, np.full(codes.shape, 7, np.uint8))
    check_the_next_call()


def test_argument_errors_of_the_c_abi_come_before_any_launch():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_flowsum_u8_dev, ctx.lib.hdem_flowsum_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, fake, 1, 16, 0, fake, None, None, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    # distinct fake rasters of 4 x 4 cells, 4 KiB apart: every refusal below is made on the
    # arguments alone
    d8, w, total, value, mask = (ctypes.c_void_p(4096 * k) for k in range(1, 6))
    fn = ctx.lib.hdem_flowsum_u8_dev
    for args, words in (
            ((d8, 4, 4, w, 1, 16, 0, None, None, None, None), b"no output wanted"),
            ((d8, 4, 4, w, 1, 16, 0, None, None, mask, None), b"mask needs a threshold >= 1"),
            ((d8, 4, 4, w, 1, 16, -5, None, None, mask, None), b"mask needs a threshold >= 1"),
            ((d8, 4, 4, w, 1, 16, 5, total, None, None, None), b"a threshold goes with mask"),
            ((d8, 4, 4, w, 1, 31, 0, total, None, None, None), b"frac_bits is 0 ... 30"),
            ((d8, 4, 4, w, 1, -1, 0, total, None, None, None), b"frac_bits is 0 ... 30"),
            ((d8, 4, 4, w, 2, 16, 0, total, None, None, None), b"integer weights take frac_bits 0"),
            ((d8, 4, 4, w, 3, 1, 0, total, None, None, None), b"integer weights take frac_bits 0"),
            ((d8, 4, 4, w, 0, 0, 0, total, None, None, None), b"unknown weight type 0"),
            ((d8, 4, 4, w, 4, 0, 0, total, None, None, None), b"unknown weight type 4"),
            ((d8, 4, 4, None, 1, 16, 0, total, None, None, None), b"weight raster is null"),
            ((d8, 4, 4, w, 1, 16, 0, w, None, None, None), b"sum overlaps weights"),
            ((d8, 4, 4, w, 1, 16, 0, total, total, None, None), b"value overlaps sum"),
            ((d8, 4, 4, w, 1, 16, 3, total, value, ctypes.c_void_p(4096 + 15), None),
             b"mask overlaps d8"),
            ((d8, 4, 4, w, 1, 16, 0, ctypes.c_void_p(4096 * 2 + 56), None, None, None),
             b"sum overlaps weights")):
        assert fn(ctx.handle, *args) == backend.BAD_ARG, words
        assert words in ctx.lib.hdem_last_error(), (words, ctx.lib.hdem_last_error())
    short = backend._FlowSumStats()                  # pylint: disable=protected-access
    short.struct_size = 2
    assert fn(ctx.handle, d8, 4, 4, w, 1, 16, 0, total, None, None,
              ctypes.byref(short)) == backend.BAD_ARG
    assert b"hdem_flowsum_stats.struct_size" in ctx.lib.hdem_last_error()
    check_the_next_call()


def test_a_shorter_stats_struct_is_filled_as_far_as_it_goes():
    codes = np.full((1, 200), E, np.uint8)
    w = np.ones((1, 200), np.uint8)
    out = np.zeros((1, 200), np.int64)
    ctx = backend.context()
    st = backend._FlowSumStats()                     # pylint: disable=protected-access
    st.struct_size = 16                              # struct_size, max_hops, exits
    st.nan_weights, st.tile_h = -7, -7
    rc = ctx.lib.hdem_flowsum_u8(ctx.handle, codes.ctypes.data, 1, 200, w.ctypes.data, 3, 0, 0,
                                 out.ctypes.data, None, None, ctypes.byref(st))
    assert rc == backend.OK and np.array_equal(out[0], np.arange(1, 201))
    assert st.struct_size == 16 and st.exits == 3 and st.max_hops == 2
    assert st.nan_weights == -7 and st.tile_h == -7


def test_profiling_fills_the_phase_times_and_adds_no_kernel_id():
    ctx = backend.context()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        f = hd.WeightedFlowAccumulation(np.ones((300, 300), np.float32))
        f.apply(random_acyclic_codes(300, 300, seed=5, ramp=True))
        unweighted_launches = ctx.profile_get(backend.K_FLOWACC)["launches"]
    finally:
        ctx.profile(False)
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0
    assert unweighted_launches == 0
    g = hd.WeightedFlowAccumulation(np.ones((64, 64), np.float32))
    g.apply(np.zeros((64, 64), np.uint8))
    assert g.stats["ms_tile"] == 0 and g.stats["ms_final"] == 0     # profiling is off
