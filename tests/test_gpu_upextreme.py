"""
Upstream D8 extremes and depression breaching on the MI355X (``UpstreamExtreme``,
``BreachDepressions``, ``hdem_upextreme_u8[_dev]``, ``hdem_breach_f32[_dev]``): both modes, both
value types and both outputs against the Kahn reference of tests/test_upextreme.py byte for
byte, NaN values, ties, a snake through every tile, a row and a column of 157 tiles, either
output alone, host / device / repeat equality, poisoned scratch and output memory, the carved
DEM against the NumPy carving and against the library's own fill, a trench with a closed form,
and the refusals, each followed by a correct call on the same context.
"""
import ctypes
import functools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, upextreme
from hydrodem_amd.backend import DeviceRaster
from test_flowacc import random_acyclic_codes
from test_gpu_flowacc import E, N, S, W_, path_codes, snake
from test_gpu_scribble import Case, execute
from test_upextreme import NOWHERE, QUIET_NAN, carve_ref, raster_of, same_bytes, upext_kahn

pytestmark = pytest.mark.gpu

# one cell; below, at and above one tile; partial tiles in both directions; strips; 3 x 4 tiles
SHAPES = [(1, 1), (63, 63), (64, 64), (65, 65), (127, 129), (7, 1000), (130, 197)]
CASES = [(shape, ramp) for shape in SHAPES for ramp in (False, True)] + [((4097, 300), True)]
CASE_IDS = [f"{h}x{w}-{'ramp' if ramp else 'noise'}" for (h, w), ramp in CASES]
BOTH = ("extreme", "where")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


@functools.lru_cache(maxsize=None)
def codes_of(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    codes.setflags(write=False)
    return codes


def extremes(codes, values, mode, want=BOTH):
    outs, stats = upextreme.upextreme(np.ascontiguousarray(codes), values, mode, want)
    for name, out in outs.items():
        assert out.shape == codes.shape
        assert out.dtype == (np.uint32 if name == "where" else values.dtype)
    return outs, stats


def random_values(kind, shape, rng):
    """The values of one kind of the issue's list."""
    if kind == "u32":
        v = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
        v.flat[v.size // 2] = 0                                 # ordinary values, both of them
        v.flat[-1] = 0xFFFFFFFF
        return v
    if kind == "ties":                                          # eight distinct numbers
        pool = np.array([-np.inf, -3.5, -0.0, 0.0, 1.0, 1.5, 1e30, np.inf], np.float32)
        return pool[rng.integers(0, 8, size=shape)]
    v = (rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2000)
    if kind == "f32n":                                          # 1 % NaN
        v[rng.random(shape) < 0.01] = np.nan
        v.flat[0] = np.nan
    return v


# ---------------------------------------------------------------------------
# against the Kahn reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "u32", "f32n", "ties"])
@pytest.mark.parametrize("shape,ramp", CASES, ids=CASE_IDS)
def test_both_modes_and_outputs_match_the_kahn_reference(shape, ramp, kind):
    codes = codes_of(shape, ramp)
    v = random_values(kind, shape, np.random.default_rng(shape[0] * 13 + shape[1] + 1000 * ramp))
    nans = int(np.isnan(v).sum()) if v.dtype == np.float32 else 0
    assert (nans > 0) == (kind == "f32n")
    for mode in ("min", "max"):
        outs, stats = extremes(codes, v, mode)
        want_extreme, want_where = upext_kahn(codes, v, mode)
        assert same_bytes(outs["extreme"], want_extreme), mode
        assert same_bytes(outs["where"], want_where), mode
        assert stats["absent"] == nans
        assert stats["tile_h"] == 64 and stats["tile_w"] == 64
        # the holder holds the extreme wherever a value is present
        present = outs["where"] != NOWHERE
        assert same_bytes(v.ravel()[outs["where"][present]], outs["extreme"][present])
        if v.dtype == np.float32:
            assert np.all(outs["extreme"].view(np.uint32)[~present] == QUIET_NAN)
        else:
            assert present.all()


def test_a_snake_through_every_tile_against_the_running_extremes():
    cells = snake(512, 512)
    codes = path_codes((512, 512), cells)
    ys, xs = np.array(cells).T
    along = (np.arange(len(cells), dtype=np.int64) * 7919) % 10007
    for dtype in (np.uint32, np.float32):
        v = np.zeros((512, 512), dtype)
        v[ys, xs] = along
        for mode, running in (("min", np.minimum.accumulate), ("max", np.maximum.accumulate)):
            outs, stats = extremes(codes, v, mode)
            assert np.array_equal(outs["extreme"][ys, xs], running(along).astype(dtype))
            assert same_bytes(v.ravel()[outs["where"]], outs["extreme"])
            assert stats["max_hops"] >= 63


@pytest.mark.parametrize("mode", ["min", "max"])
def test_a_row_and_a_column_carry_the_extreme_from_the_far_end(mode):
    k = np.arange(10000, dtype=np.uint32)
    far = k + 5 if mode == "min" else 20000 - k           # the extreme at the head of the path
    near = 20000 - k if mode == "min" else k + 5          # ... and at every cell itself
    for codes, shape in ((np.full((1, 10000), E, np.uint8), (1, 10000)),
                         (np.full((10000, 1), S, np.uint8), (10000, 1))):
        outs, stats = extremes(codes, far.reshape(shape), mode)
        assert np.all(outs["extreme"] == far[0]) and np.all(outs["where"] == 0)
        assert stats["exits"] == 156 and stats["max_hops"] >= 155  # 156 tile crossings
        v = near.astype(np.float32).reshape(shape)
        outs, _ = extremes(codes, v, mode)
        assert same_bytes(outs["extreme"], v)
        assert np.array_equal(outs["where"].ravel(), k)


# ---------------------------------------------------------------------------
# either output alone; host form, device form, a repeat
# ---------------------------------------------------------------------------
def test_either_output_alone_holds_the_bytes_of_the_call_for_both():
    shape = (127, 129)
    codes = codes_of(shape, True)
    for kind in ("f32n", "u32"):
        v = random_values(kind, shape, np.random.default_rng(17))
        for mode in ("min", "max"):
            both, _ = extremes(codes, v, mode)
            for name in BOTH:
                alone, _ = extremes(codes, v, mode, name)
                assert list(alone) == [name] and same_bytes(alone[name], both[name])
                f = hd.UpstreamExtreme(v, mode, name)
                got = f.apply(codes)
                assert got.dtype == f.dtype and same_bytes(got, both[name])
                assert f.stats["exits"] > 0


def test_host_and_device_forms_and_a_repeat_are_byte_equal():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    v = random_values("f32n", codes.shape, np.random.default_rng(5))
    a, stats_a = upextreme.upextreme(codes, v, "min", BOTH)
    b, _ = upextreme.upextreme(codes, v, "min", BOTH)
    with DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            DeviceRaster.from_host(v, dtype=np.float32) as dv:
        dev, stats_c = upextreme.upextreme_dev(dc, dv, "min", BOTH)
        c = {}
        for name, raster in dev.items():
            with raster:
                c[name] = raster.to_host()
        with hd.UpstreamExtreme(dv, "min", "where").apply_device(dc) as where:
            assert where.dtype == np.uint32 and same_bytes(where.to_host(), a["where"])
    for name in BOTH:
        assert same_bytes(a[name], b[name]) and same_bytes(a[name], c[name]), name
    for key in ("exits", "absent", "tile_h", "tile_w"):
        assert stats_a[key] == stats_c[key]
    assert stats_a["exits"] > 0 and stats_a["max_hops"] > 0
    assert same_bytes(a["where"], upext_kahn(codes, v, "min")[1])


# ---------------------------------------------------------------------------
# poisoned scratch and output memory
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=None):
    codes = codes_of(shape, True) if shape[1] > 1 else np.full(shape, S, np.uint8)
    return {"codes": codes, "v": random_values("f32n", shape, np.random.default_rng(shape[0]))}


def poison_run(call, inp):
    """One device call of each operator for all its outputs."""
    codes, v = inp["codes"], inp["v"]
    dtypes = {"extreme": v.dtype, "where": np.uint32, "carved": np.float32, "source": np.uint32}
    dc, dv = call.up(np.ascontiguousarray(codes)), call.up(v)
    out = {name: call.out(codes.shape, dtype) for name, dtype in dtypes.items()}
    dev, stats = upextreme.upextreme_dev(
        dc, dv, "max", BOTH, out={k: out[k] for k in BOTH} if call.own else None)
    carved, breach_stats = upextreme.breach_dev(
        dv, dc, ("carved", "source"),
        out={k: out[k] for k in ("carved", "source")} if call.own else None)
    dev.update(carved)
    for name, raster in dev.items():
        assert not call.own or raster is out[name]
    host = {name: call.host(raster) for name, raster in dev.items()}
    stats = {**{k: n for k, n in stats.items() if not k.startswith("ms_")},
             **{"breach_" + k: n for k, n in breach_stats.items() if not k.startswith("ms_")}}
    return host, stats


def poison_check(inp, got):
    codes, v = inp["codes"], inp["v"]
    want_extreme, want_where = upext_kahn(codes, v, "max")
    assert same_bytes(got["extreme"], want_extreme) and same_bytes(got["where"], want_where)
    want_carved, want_source, _, _ = carve_ref(v, codes)
    assert same_bytes(got["carved"], want_carved) and same_bytes(got["source"], want_source)


POISON_SHAPES = [(130, 197), (65, 1)]
# max_hops: the walk that goes on at a node is the one whose atomic arrives last
POISON_CASE = Case("upextreme-max-and-breach", tuple(POISON_SHAPES), poison_inputs, poison_run,
                   poison_check, True, frozenset(("max_hops", "breach_max_hops")))


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
@pytest.mark.parametrize("shape", POISON_SHAPES)
def test_poisoned_memory_changes_nothing(shape, own):
    inp = POISON_CASE.build(shape)
    clean, clean_stats = execute(POISON_CASE, inp, None, own)
    POISON_CASE.check(inp, clean)
    _, _, pits, lowered = carve_ref(inp["v"], inp["codes"])
    assert clean_stats["breach_pits"] == pits and clean_stats["breach_lowered"] == lowered
    for byte in (0x00, 0xFF):                                   # 0x00 first
        got, stats = execute(POISON_CASE, inp, byte, own)
        for name in clean:
            assert same_bytes(got[name], clean[name]), (name, byte)
        assert stats == clean_stats, byte


# ---------------------------------------------------------------------------
# breaching
# ---------------------------------------------------------------------------
def dem_of(kind, shape):
    return hdem_synth.synth_dem(*shape) if shape == (4097, 300) else raster_of(kind, shape)


@pytest.mark.parametrize("kind,shape", [
    ("noise", (65, 65)), ("noise", (130, 197)), ("steps", (65, 65)), ("steps", (130, 197)),
    ("synth", (300, 300)), ("synth", (4097, 300))],
    ids=["noise-65x65", "noise-130x197", "steps-65x65", "steps-130x197", "synth-300x300-nan",
         "synth-4097x300"])
def test_the_carved_dem_matches_the_reference_and_is_its_own_fill(kind, shape):
    dem = dem_of(kind, shape)
    f = hd.BreachDepressions(keep_partial_results=True)
    carved = f.apply(dem)
    assert carved.dtype == np.float32 and isinstance(f.codes, np.ndarray)
    assert f.codes.dtype == np.uint8 and f.filled.dtype == np.float32
    want, want_source, pits, lowered = carve_ref(dem, f.codes)
    assert same_bytes(carved, want) and same_bytes(f.source, want_source)
    stats = f.stats["BreachDepressions"]
    assert stats["pits"] == pits and stats["lowered"] == lowered and lowered > 0
    assert stats["absent"] == dem.size - pits
    assert set(f.stats) == {"SinkFill", "ResolveFlats", "BreachDepressions"}
    changed = f.source != NOWHERE
    assert same_bytes(dem.ravel()[f.source[changed]], carved[changed])
    if kind == "synth" and shape == (300, 300):
        assert np.isnan(dem).sum() == 201
    # no sinks: the exact fill of the carved DEM is the carved DEM
    chain = hd.HydroConditioning(epsilon=0.0)
    chain.apply(carved)
    assert same_bytes(chain.filled, carved)
    # and carving it again changes nothing
    g = hd.BreachDepressions()
    assert same_bytes(g.apply(carved), carved)
    assert g.stats["BreachDepressions"]["lowered"] == 0
    assert g.filled is None and g.codes is None and g.source is None


def test_the_breach_on_the_device_leaves_rasters_to_their_caller():
    dem = raster_of("noise", (130, 197))
    want = hd.BreachDepressions().apply(dem)
    with DeviceRaster.from_host(dem, dtype=np.float32) as dz:
        f = hd.BreachDepressions(keep_partial_results=True)
        with f.apply_device(dz) as carved:
            assert same_bytes(carved.to_host(), want)
        kept = {name: getattr(f, name) for name in ("filled", "codes", "source")}
        assert all(backend.is_device_raster(r) for r in kept.values())
        with kept["filled"], kept["codes"], kept["source"]:
            codes = kept["codes"].to_host()
            assert same_bytes(kept["source"].to_host(), carve_ref(dem, codes)[1])
            # the staged calls give the same bytes
            outs, _ = upextreme.breach(dem, codes, ("carved", "source"))
            assert same_bytes(outs["carved"], want)
        g = hd.BreachDepressions()
        with g.apply_device(dz) as carved:
            assert same_bytes(carved.to_host(), want)
        assert g.filled is None and g.codes is None and g.source is None


def test_a_trench_through_79_tiles_against_the_closed_form():
    """The pit at (2, 1) is cut through to the raster's edge: every cell of row 2 east of it
    comes down to the pit's level, the outlet cell on the ring too (it lies on the pit's D8
    path like any other).  The pit itself is unchanged, so it names no source."""
    dem = np.full((5, 5000), 1000.0, np.float32)
    dem[2] = 500 - np.float32(0.1) * np.arange(5000, dtype=np.float32)
    dem[2, 1] = -50
    f = hd.BreachDepressions(keep_partial_results=True)
    carved = f.apply(dem)
    want = dem.copy()
    want[2, 1:] = -50
    assert same_bytes(carved, want)
    want_source = np.full(dem.shape, NOWHERE, np.uint32)
    want_source[2, 2:] = 2 * 5000 + 1
    assert same_bytes(f.source, want_source)
    stats = f.stats["BreachDepressions"]
    assert stats["pits"] == 1 and stats["lowered"] == 4998 and stats["exits"] >= 78


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def valley(w):
    """Five rows that descend east, the middle one lowest, with one pit at (2, 1)."""
    yy, xx = np.indices((5, w))
    dem = (100 * np.abs(yy - 2) + 2 * w - xx).astype(np.float32)
    dem[2, 1] = 0.5
    return dem


def check_the_next_call():
    cells = snake(130, 70)
    codes = path_codes((130, 70), cells)
    ys, xs = np.array(cells).T
    v = np.zeros((130, 70), np.uint32)
    v[ys, xs] = np.arange(len(cells))
    outs, _ = extremes(codes, v, "max")
    assert same_bytes(outs["extreme"], v)
    assert np.array_equal(outs["where"].ravel(), np.arange(v.size))
    dem = valley(70)
    carved, _ = upextreme.breach(dem, np.full((5, 70), E, np.uint8))
    assert np.all(carved["carved"][2, 1:] == 0.5) and same_bytes(carved["carved"][1], dem[1])


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        extremes(codes, np.ones(codes.shape, np.uint32), "min")
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        upextreme.breach(np.ones(codes.shape, np.float32), codes)
    check_the_next_call()


def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="cycle: 2 cells never drain"):
        extremes(np.array([[E, W_]], np.uint8), np.ones((1, 2), np.float32), "max")
    check_the_next_call()
    codes = np.zeros((256, 256), np.uint8)               # clockwise round a 200 x 200 rim
    y0, x0, n = 10, 20, 200
    codes[y0, x0:x0 + n - 1] = E
    codes[y0:y0 + n - 1, x0 + n - 1] = S
    codes[y0 + n - 1, x0 + 1:x0 + n] = W_
    codes[y0 + 1:y0 + n, x0] = N
    assert int((codes != 0).sum()) == 796
    for mode in ("min", "max"):
        with pytest.raises(ValueError, match="cycle"):
            extremes(codes, np.full(codes.shape, 7, np.uint32), mode)
    with pytest.raises(ValueError, match="cycle"):
        upextreme.breach(np.ones(codes.shape, np.float32), codes)
    check_the_next_call()


def test_argument_errors_of_the_c_abi_come_before_any_launch():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_upextreme_u8_dev, ctx.lib.hdem_upextreme_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, fake, 1, 0, fake, None, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    for fn in (ctx.lib.hdem_breach_f32_dev, ctx.lib.hdem_breach_f32):
        rc = fn(ctx.handle, fake, fake, 65536, 65536, fake, None, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    # distinct fake rasters of 4 x 4 cells, 4 KiB apart: every refusal below is made on the
    # arguments alone
    d8, v, extreme, where = (ctypes.c_void_p(4096 * k) for k in range(1, 5))
    fn = ctx.lib.hdem_upextreme_u8_dev
    for args, words in (
            ((d8, 4, 4, v, 1, 0, None, None, None), b"no output wanted"),
            ((d8, 4, 4, v, 0, 0, extreme, None, None), b"unknown value type 0"),
            ((d8, 4, 4, v, 3, 0, extreme, None, None), b"unknown value type 3"),
            ((d8, 4, 4, v, 1, 2, extreme, None, None), b"unknown mode 2"),
            ((d8, 4, 4, v, 2, -1, extreme, None, None), b"unknown mode -1"),
            ((d8, 4, 4, None, 1, 0, extreme, None, None), b"value raster is null"),
            ((None, 4, 4, v, 1, 0, extreme, None, None), b"null raster pointer"),
            ((d8, 4, 4, v, 1, 0, v, None, None), b"extreme overlaps values"),
            ((d8, 4, 4, v, 1, 0, extreme, extreme, None), b"where overlaps extreme"),
            ((d8, 4, 4, v, 1, 1, extreme, ctypes.c_void_p(4096 + 15), None),
             b"where overlaps d8"),
            ((d8, 4, 4, v, 1, 0, None, ctypes.c_void_p(4096 * 2 + 60), None),
             b"where overlaps values")):
        assert fn(ctx.handle, *args) == backend.BAD_ARG, words
        assert words in ctx.lib.hdem_last_error(), (words, ctx.lib.hdem_last_error())
    short = backend._UpExtremeStats()                # pylint: disable=protected-access
    short.struct_size = 2
    assert fn(ctx.handle, d8, 4, 4, v, 1, 0, extreme, None, ctypes.byref(short)) == backend.BAD_ARG
    assert b"hdem_upextreme_stats.struct_size" in ctx.lib.hdem_last_error()
    dem, carved, source = v, extreme, where
    fn = ctx.lib.hdem_breach_f32_dev
    for args, words in (
            ((None, d8, 4, 4, carved, None, None), b"null raster pointer"),
            ((dem, d8, 4, 4, None, source, None), b"null raster pointer"),
            ((dem, None, 4, 4, carved, None, None), b"code raster is null"),
            ((dem, d8, 4, 4, dem, None, None), b"carved overlaps dem"),
            ((dem, d8, 4, 4, ctypes.c_void_p(4096 - 60), None, None), b"carved overlaps d8"),
            ((dem, d8, 4, 4, carved, carved, None), b"source overlaps carved"),
            ((dem, d8, 4, 4, carved, dem, None), b"source overlaps dem")):
        assert fn(ctx.handle, *args) == backend.BAD_ARG, words
        assert words in ctx.lib.hdem_last_error(), (words, ctx.lib.hdem_last_error())
    short = backend._BreachStats()                   # pylint: disable=protected-access
    short.struct_size = 3
    assert fn(ctx.handle, dem, d8, 4, 4, carved, None, ctypes.byref(short)) == backend.BAD_ARG
    assert b"hdem_breach_stats.struct_size" in ctx.lib.hdem_last_error()
    check_the_next_call()


def test_a_shorter_stats_struct_is_filled_as_far_as_it_goes():
    codes = np.full((1, 200), E, np.uint8)
    v = np.arange(200, dtype=np.uint32).reshape(1, 200)
    out = np.zeros((1, 200), np.uint32)
    ctx = backend.context()
    st = backend._UpExtremeStats()                   # pylint: disable=protected-access
    st.struct_size = 16                              # struct_size, max_hops, exits
    st.absent, st.tile_h = -7, -7
    rc = ctx.lib.hdem_upextreme_u8(ctx.handle, codes.ctypes.data, 1, 200, v.ctypes.data, 2, 1,
                                   out.ctypes.data, None, ctypes.byref(st))
    assert rc == backend.OK and np.array_equal(out, v)
    assert st.struct_size == 16 and st.exits == 3 and st.max_hops == 2
    assert st.absent == -7 and st.tile_h == -7
    # the breach's struct cut down to the extreme's: pits and lowered stay the caller's
    dem = valley(200)
    codes = np.full((5, 200), E, np.uint8)
    carved = np.zeros((5, 200), np.float32)
    bst = backend._BreachStats()                     # pylint: disable=protected-access
    bst.struct_size = 48
    bst.pits, bst.lowered = -7, -7
    rc = ctx.lib.hdem_breach_f32(ctx.handle, dem.ctypes.data, codes.ctypes.data, 5, 200,
                                 carved.ctypes.data, None, ctypes.byref(bst))
    assert rc == backend.OK and np.all(carved[2, 1:] == 0.5) and same_bytes(carved[1], dem[1])
    assert bst.struct_size == 48 and bst.exits == 15 and bst.absent == 999 and bst.tile_h == 64
    assert bst.pits == -7 and bst.lowered == -7
    bst = backend._BreachStats()                     # pylint: disable=protected-access
    rc = ctx.lib.hdem_breach_f32(ctx.handle, dem.ctypes.data, codes.ctypes.data, 5, 200,
                                 carved.ctypes.data, None, ctypes.byref(bst))
    assert rc == backend.OK and bst.pits == 1 and bst.lowered == 198


def test_profiling_fills_the_phase_times_and_adds_no_kernel_id():
    ctx = backend.context()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        f = hd.UpstreamExtreme(np.ones((300, 300), np.float32))
        f.apply(random_acyclic_codes(300, 300, seed=5, ramp=True))
        b = hd.BreachDepressions()
        b.apply(raster_of("noise", (130, 197)))
        unweighted_launches = ctx.profile_get(backend.K_FLOWACC)["launches"]
    finally:
        ctx.profile(False)
    for stats in (f.stats, b.stats["BreachDepressions"]):
        assert stats["ms_tile"] > 0 and stats["ms_forest"] > 0 and stats["ms_final"] > 0
    assert unweighted_launches == 0
    g = hd.UpstreamExtreme(np.ones((64, 64), np.float32))
    g.apply(np.zeros((64, 64), np.uint8))
    assert g.stats["ms_tile"] == 0 and g.stats["ms_final"] == 0     # profiling is off
