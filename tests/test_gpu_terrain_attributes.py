"""
The fused terrain-attribute kernel (``hdem_terrain_f32[_dev]``, ``TerrainAttributes``) on the
MI355X against the reference of tests/test_terrain_attributes.py.

Shapes: the smallest at which a kernel of 256 x 32 tiles with 4 cells per lane can go wrong
(strips and tiny rasters, one exact tile, one cell past it both ways, ``W % 4 != 0``, three
tile columns with a partial last one).  Rasters: ``synth_dem`` with NaN on the border, on both
sides of the tile seams and in a block, plus a constant block (flat cells, floored slopes), and
the regimes of tests/elevation_regimes.py.

Bars.  ``dzdx``, ``dzdy`` and ``d8_slope`` are the reference's bits (a NaN is a NaN, whatever
its sign and payload: x86 and gfx950 make different ones from inf - inf); ``tangent`` within
1 ulp; ``spi`` within 2.  ``degrees``, ``aspect`` and ``twi`` are held to the float64 functions
of the REFERENCE's float32 ``dzdx``, ``dzdy``, ``tangent`` by
``|got - want| <= N * spacing(float32(max(|want|, floor)))``: N is the OpenCL full-profile
limit of the function (atan 5, atan2 6, log 3 ulp) plus one ulp per further rounding (2 for
degrees and aspect: the constant 180 / pi and the product; 3 for twi), so 7, 8 and 6;
``floor`` is 0, 360 (around the circle) and 1.  The largest error seen is printed per output
(``-s``) and recorded in DESIGN 3.19: 1.80, 0.87 and 1.91; tangent and spi were bit-equal.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from elevation_regimes import REGIMES, regime_raster
from hydrodem_amd import backend as B
from hydrodem_amd import terrain as T
from hydrodem_amd.backend import DeviceRaster
from test_gpu_scribble import POISON, Case, assert_same_bytes, execute
from test_terrain_attributes import (aspect_f64, d8_slope_f32, degrees_f64, floored,
                                     gradient_f32, invalid_codes, spi_f32, twi_f64)

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (32, 256), (33, 257), (64, 33), (131, 157),
          (70, 515)]
REGIME_SHAPE = (131, 157)
FINITE_REGIMES = ("below_sea", "zero_cross", "high_8000", "milli")
DY, DX, ZF, MIN_SLOPE = 30.0, 10.0, 2.0, 1e-3            # anisotropic cells on purpose
ALL = T.TERRAIN_OUTPUTS
N_ULP = {"degrees": 7, "aspect": 8, "twi": 6}
FLOOR = {"degrees": 0.0, "aspect": 360.0, "twi": 1.0}
CODES = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128], np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


# ---------------------------------------------------------------------------
# inputs and their reference, made once
# ---------------------------------------------------------------------------
def planted(shape):
    """``synth_dem`` with NaN on the border, on both sides of the tile seams and in a 4 x 20
    block, and a constant block, wherever the shape has room for them."""
    h, w = shape
    z = hdem_synth.synth_dem(h, w).copy()
    if h >= 9 or w >= 9:
        z[0, w // 2] = z[h - 1, 0] = z[h // 2, w - 1] = np.nan
    if h > 33:
        z[31:33, 5 % w] = np.nan                         # both sides of the row seam
        z[31, w - 2] = z[32, w - 3] = np.nan
    if w > 257:
        z[h // 3, 255:257] = np.nan                      # both sides of the column seam
        z[h - 2, 255] = z[h - 3, 256] = np.nan
    if h > 33 and w > 257:
        z[31:33, 255:257] = np.nan                       # the corner of four tiles
    if h >= 20 and w >= 30:
        z[12:16, 5:25] = np.nan                          # the 4 x 20 block
        z[3:9, 4:28] = z[3, 4]                           # flat cells, slopes under the floor
    return z


@functools.lru_cache(maxsize=None)
def inputs(kind, shape):
    z = planted(shape) if kind == "synth" else regime_raster(kind, shape)
    rng = np.random.default_rng([7, *shape])
    codes = CODES[rng.integers(0, CODES.size, shape)]
    acc = rng.integers(0, 5000, shape).astype(np.uint32)
    acc.ravel()[::17] = 0                                # ln 0
    acc.ravel()[5::23] = 0xFFFFFFFF                      # the largest area
    for a in (z, codes, acc):
        a.setflags(write=False)
    return {"dem": z, "codes": codes, "acc": acc}


@functools.lru_cache(maxsize=None)
def reference(kind, shape, slope="horn"):
    inp = inputs(kind, shape)
    dzdx, dzdy, s2, tangent = gradient_f32(inp["dem"], DX, DY, ZF)
    d8 = d8_slope_f32(inp["dem"], inp["codes"], DX, DY, ZF)
    t = d8 if slope == "d8" else tangent
    low = floored(t, MIN_SLOPE)
    return {"dzdx": dzdx, "dzdy": dzdy, "s2": s2, "tangent": tangent,
            "degrees": degrees_f64(tangent), "aspect": aspect_f64(dzdx, dzdy), "d8_slope": d8,
            "twi": twi_f64(inp["acc"], t, DX, DY, MIN_SLOPE), "spi": spi_f32(inp["acc"], t, DX, DY),
            "stats": {"nan_cells": int(np.isnan(inp["dem"]).sum()),
                      "flat_cells": int(((dzdx == 0) & (dzdy == 0)).sum()),
                      "floored_cells": int(low.sum()), "invalid_codes": 0}}


def run_dev(inp, want, slope="horn", ctx=None, out=None):
    """One device call on host inputs: ``{name: host array}`` and the stats."""
    ctx = ctx or B.context()
    with contextlib.ExitStack() as stack:
        def up(a):
            return stack.enter_context(DeviceRaster.from_host(a, dtype=a.dtype, ctx=ctx))
        needs_codes = slope == "d8" or "d8_slope" in want
        needs_acc = "twi" in want or "spi" in want
        outs, stats = T.terrain_dev(up(inp["dem"]), want, (DY, DX), ZF,
                                    up(inp["codes"]) if needs_codes else None,
                                    up(inp["acc"]) if needs_acc else None, MIN_SLOPE, slope,
                                    out=out)
        for raster in outs.values():
            if out is None or not any(raster is r for r in out.values()):
                stack.enter_context(raster)
        return {name: raster.to_host() for name, raster in outs.items()}, stats


@functools.lru_cache(maxsize=None)
def device(kind, shape, slope="horn"):
    return run_dev(inputs(kind, shape), ALL, slope)


CASES = [("synth", shape) for shape in SHAPES] + [(name, REGIME_SHAPE) for name in REGIMES]
IDS = [f"{kind}-{shape[0]}x{shape[1]}" for kind, shape in CASES]


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def same_bits(got, want):
    """Bit-equal where the reference is a number (infinities are numbers), NaN where it is NaN."""
    assert got.dtype == want.dtype == np.dtype(F32) and got.shape == want.shape
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def ulps_f32(got, want):
    """|got - want| in units of the float32 spacing at ``want``, over the cells where ``want`` is
    finite; the others must agree exactly (an infinity) or be NaN (a NaN)."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    if not fin.any():
        return 0.0
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    unit = np.spacing(np.abs(want[fin]).astype(F32)).astype(np.float64)
    return float((np.abs(g - w) / unit).max())


def worst(name, got, want, keep):
    """The largest error of a transcendental output over the cells ``keep``, in units of
    ``spacing(float32(max(|want|, floor)))``; infinities must agree exactly."""
    got, want = got[keep].astype(np.float64), want[keep]
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), name
    got, want = got[~inf], want[~inf]
    if not got.size:
        return 0.0
    assert np.isfinite(got).all(), name
    err = np.abs(got - want)
    if name == "aspect":
        flat = want == -1
        assert np.array_equal(got == -1, flat), "aspect -1 must match exactly"
        err = np.where(flat, 0.0, np.minimum(err, 360.0 - err))
    unit = np.spacing(np.maximum(np.abs(want), FLOOR[name]).astype(F32)).astype(np.float64)
    return float((err / unit).max())


def usable(ref):
    """The cells of the transcendental comparison: the reference's own float32 dzdx, dzdy and
    s2 are finite.  Returns them and the cells left out that are not NaN cells of the DEM."""
    fin = np.isfinite(ref["dzdx"]) & np.isfinite(ref["dzdy"]) & np.isfinite(ref["s2"])
    return fin, ~fin & ~np.isnan(ref["dzdx"])


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_every_output_against_the_reference(kind, shape):
    ref = reference(kind, shape)
    got, stats = device(kind, shape)
    assert same_bits(got["dzdx"], ref["dzdx"]) and same_bits(got["dzdy"], ref["dzdy"])
    assert same_bits(got["d8_slope"], ref["d8_slope"])
    tangent_ulp = ulps_f32(got["tangent"], ref["tangent"])
    spi_ulp = ulps_f32(got["spi"], ref["spi"])
    fin, left_out = usable(ref)
    if kind == "synth" or kind in FINITE_REGIMES:
        assert not left_out.any()
    hole = np.isnan(inputs(kind, shape)["dem"])
    seen = {}
    for name in ("degrees", "aspect", "twi"):
        assert np.isnan(got[name][hole]).all() and not np.isnan(got[name][~hole & fin]).any()
        seen[name] = worst(name, got[name], ref[name], fin)
    print(f"\nterrain ulp {kind} {shape}: tangent {tangent_ulp:.3f} spi {spi_ulp:.3f} " +
          " ".join(f"{k} {v:.3f}" for k, v in seen.items()) +
          f" bit-equal tangent {same_bits(got['tangent'], ref['tangent'])}")
    assert tangent_ulp <= 1 and spi_ulp <= 2
    for name, n in N_ULP.items():
        assert seen[name] <= n, (name, seen[name])
    assert {k: v for k, v in stats.items() if k != "ms_total"} == ref["stats"]


@pytest.mark.parametrize("shape", [(33, 257), (131, 157)], ids=str)
def test_wetness_along_the_d8_slope(shape):
    ref = reference("synth", shape, "d8")
    got, stats = device("synth", shape, "d8")
    horn, _ = device("synth", shape)
    for name in ("dzdx", "dzdy", "tangent", "degrees", "aspect", "d8_slope"):
        assert_same_bytes({name: got[name]}, {name: horn[name]}, name)
    assert ulps_f32(got["spi"], ref["spi"]) <= 2
    keep = ~np.isnan(ref["twi"])
    assert np.isnan(got["twi"][~keep]).all()
    assert worst("twi", got["twi"], ref["twi"], keep) <= N_ULP["twi"]
    assert stats["floored_cells"] == ref["stats"]["floored_cells"] > 0


def test_flat_and_floored_cells_are_there_to_count():
    ref = reference("synth", (131, 157))
    assert ref["stats"]["flat_cells"] > 50 and ref["stats"]["floored_cells"] > 50
    assert ref["stats"]["nan_cells"] > 80


# ---------------------------------------------------------------------------
# host and device forms, subsets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 9), (33, 257), (131, 157)], ids=str)
def test_the_host_form_returns_the_bytes_of_the_device_form(shape):
    inp = inputs("synth", shape)
    want, want_stats = device("synth", shape)
    got, stats = T.terrain(inp["dem"], ALL, (DY, DX), ZF, inp["codes"], inp["acc"], MIN_SLOPE)
    assert_same_bytes(got, want, f"host form {shape}")
    assert {k: v for k, v in stats.items() if k != "ms_total"} == \
        {k: v for k, v in want_stats.items() if k != "ms_total"}


SUBSETS = [(name,) for name in ALL] + [("dzdx", "aspect"), ("tangent", "twi", "spi"),
                                       ("degrees", "d8_slope", "twi")]


@pytest.mark.parametrize("slope", T.SLOPES)
@pytest.mark.parametrize("want", SUBSETS, ids="+".join)
def test_a_subset_returns_the_bytes_of_the_call_for_all(want, slope):
    for shape in ((33, 257), (131, 157)):
        whole, _ = device("synth", shape, slope)
        got, _ = run_dev(inputs("synth", shape), want, slope)
        assert_same_bytes(got, {name: whole[name] for name in want}, f"{want} {slope} {shape}")


def test_the_filters_return_what_the_binding_returns():
    shape = (131, 157)
    inp = inputs("synth", shape)
    z = inp["dem"]
    whole, _ = run_dev(inp, ALL, "horn")
    plain, _ = T.terrain(z, ("degrees", "tangent", "aspect"))           # unit cells
    assert np.array_equal(hd.Slope().apply(z), plain["degrees"], equal_nan=True)
    assert np.array_equal(hd.Slope("tangent").apply(z), plain["tangent"], equal_nan=True)
    assert np.array_equal(hd.Slope("percent").apply(z), plain["tangent"] * F32(100),
                          equal_nan=True)
    assert np.array_equal(hd.Aspect().apply(z), plain["aspect"], equal_nan=True)
    f = hd.TerrainAttributes(("twi", "spi", "d8_slope"), (DY, DX), ZF, inp["codes"], inp["acc"],
                             MIN_SLOPE, keep_partial_results=True)
    assert np.array_equal(f.apply(z), whole["twi"], equal_nan=True)
    assert np.array_equal(f.spi, whole["spi"], equal_nan=True)
    assert np.array_equal(f.d8_slope, whole["d8_slope"], equal_nan=True) and f.twi is None
    w = hd.WetnessIndex(inp["acc"], cellsize=(DY, DX), z_factor=ZF)
    assert np.array_equal(w.apply(z), whole["twi"], equal_nan=True)
    assert w.stats["floored_cells"] == reference("synth", shape)["stats"]["floored_cells"]


# ---------------------------------------------------------------------------
# refusals of the library
# ---------------------------------------------------------------------------
def test_a_bad_code_byte_is_refused_and_counted():
    inp = inputs("synth", (64, 33))
    codes = inp["codes"].copy()
    codes[5, 7], codes[63, 32], codes[0, 0] = 3, 255, 129
    assert invalid_codes(codes) == 3
    with pytest.raises(ValueError, match="invalid D8 code in 3 cells"):
        T.terrain(inp["dem"], "d8_slope", codes=codes)
    ctx = B.context()
    st = B._TerrainStats()                               # pylint: disable=protected-access
    out = np.empty(codes.shape, F32)
    null = ctypes.c_void_p()
    rc = ctx.lib.hdem_terrain_f32(ctx.handle, inp["dem"].ctypes.data, *codes.shape, null,
                                  codes.ctypes.data, 1.0, 1.0, 1.0, 1e-3, null, null, null, null,
                                  null, out.ctypes.data, null, null, 0, ctypes.byref(st))
    assert rc == B.BAD_ARG and st.invalid_codes == 3
    assert st.nan_cells == int(np.isnan(inp["dem"]).sum())


def test_the_library_refuses_before_any_launch():
    ctx = B.context()
    z = np.zeros((4, 4), F32)
    acc, codes, out = np.ones((4, 4), np.uint32), np.ones((4, 4), np.uint8), np.empty((4, 4), F32)
    null = ctypes.c_void_p()
    ptr = lambda a: null if a is None else a.ctypes.data  # noqa: E731

    def call(dem=z, a=None, c=None, cell=(1.0, 1.0), zf=1.0, ms=1e-3, outs=(None,) * 8, flags=0):
        return ctx.lib.hdem_terrain_f32(ctx.handle, ptr(dem), 4, 4, ptr(a), ptr(c), cell[0],
                                        cell[1], zf, ms, *[ptr(o) for o in outs], flags, None)
    only = lambda k, o=out: tuple(o if j == k else None for j in range(8))  # noqa: E731
    assert call(outs=only(3)) == B.OK
    assert call() == B.BAD_ARG                                       # no output
    assert call(outs=only(6)) == B.BAD_ARG                           # twi without acc
    assert call(outs=only(7), c=codes) == B.BAD_ARG                  # spi without acc
    assert call(outs=only(5), a=acc) == B.BAD_ARG                    # d8_slope without codes
    assert call(outs=only(6), a=acc, flags=1) == B.BAD_ARG           # the flag without codes
    assert call(outs=only(3), flags=2) == B.BAD_ARG                  # unknown flag
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(outs=only(3), cell=(bad, 1.0)) == B.BAD_ARG
        assert call(outs=only(3), cell=(1.0, bad)) == B.BAD_ARG
        assert call(outs=only(3), zf=bad) == B.BAD_ARG
        assert call(outs=only(3), ms=bad) == B.BAD_ARG
    assert call(outs=only(3, z)) == B.BAD_ARG                        # an output over the dem
    assert call(outs=(out, out) + (None,) * 6) == B.BAD_ARG          # two outputs in one place
    assert call(outs=only(6, acc.view(F32)), a=acc) == B.BAD_ARG     # an output over acc


# ---------------------------------------------------------------------------
# the chain, zonal statistics over a slope raster
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("slope", T.SLOPES)
def test_dem_to_wetness_equals_its_stages(slope):
    z = hdem_synth.synth_dem(130, 197)
    conditioning = hd.HydroConditioning(epsilon=1e-3)
    codes = conditioning.apply(z)
    acc = hd.FlowAccumulation().apply(codes)
    stage = hd.WetnessIndex(acc, codes=codes, cellsize=30.0, slope=slope)
    want = stage.apply(conditioning.filled)
    chain = hd.DemToWetness(cellsize=30.0, slope=slope, keep_partial_results=True)
    got = chain.apply(z)
    assert_same_bytes({"twi": got, "filled": chain.filled, "codes": chain.codes,
                       "acc": chain.accumulation},
                      {"twi": want, "filled": conditioning.filled, "codes": codes, "acc": acc},
                      "DemToWetness.apply")
    tangent, _ = T.terrain(conditioning.filled, "tangent", 30.0)
    assert_same_bytes({"tangent": chain.tangent}, tangent, "the kept tangent")
    ours = chain.stats["WetnessIndex"]
    assert ours == {**stage.stats, "ms_total": ours["ms_total"]}
    # the device form hands its rasters to the caller
    with DeviceRaster.from_host(z) as zd:
        twi = chain.apply_device(zd)
        kept = [twi, chain.filled, chain.codes, chain.accumulation, chain.tangent]
        assert all(isinstance(r, DeviceRaster) and r.ptr for r in kept)
        assert_same_bytes({"twi": twi.to_host(), "tangent": chain.tangent.to_host()},
                          {"twi": want, "tangent": tangent["tangent"]}, "DemToWetness.apply_device")
        for raster in kept:
            raster.free()
        plain = hd.DemToWetness(cellsize=30.0, slope=slope)
        with plain.apply_device(zd) as twi:
            assert_same_bytes({"twi": twi.to_host()}, {"twi": want}, "without partial results")
        assert plain.filled is plain.codes is plain.accumulation is plain.tangent is None


def test_zonal_statistics_over_the_tangent_stay_on_the_device():
    z = hdem_synth.synth_dem(130, 197)
    with DeviceRaster.from_host(z) as zd, contextlib.ExitStack() as stack:
        conditioning = hd.HydroConditioning(epsilon=1e-3)
        codes = stack.enter_context(conditioning.apply_device(zd))
        labels = stack.enter_context(hd.Watersheds(labels="compact").apply_device(codes))
        tangent = stack.enter_context(hd.Slope("tangent", cellsize=30.0).apply_device(zd))
        table = hd.ZonalStatistics(values=tangent, columns=("count", "valid", "max", "min")) \
            .apply_device(labels)
        lab, tan = labels.to_host(), tangent.to_host()
    want_max = np.full(int(lab.max()), -np.inf, F32)
    np.maximum.at(want_max, lab.ravel().astype(np.int64) - 1, tan.ravel())
    want_min = np.full(int(lab.max()), np.inf, F32)
    np.minimum.at(want_min, lab.ravel().astype(np.int64) - 1, tan.ravel())
    assert table["count"].sum() == z.size and np.array_equal(table["valid"], table["count"])
    assert np.array_equal(table["max"], want_max) and np.array_equal(table["min"], want_min)
    assert np.array_equal(tan, gradient_f32(z, 30.0, 30.0)[3])


# ---------------------------------------------------------------------------
# poison: the method of tests/test_gpu_scribble.py
# ---------------------------------------------------------------------------
def poison_case(name, want, slope):
    def run(call, inp):
        dem = call.up(inp["dem"])
        out = {n: call.out(dem.shape, F32) for n in want} if call.own else None
        outs, stats = T.terrain_dev(dem, want, (DY, DX), ZF, call.up(inp["codes"]),
                                    call.up(inp["acc"]), MIN_SLOPE, slope, out=out)
        return {n: (r.to_host() if call.own else call.host(r)) for n, r in outs.items()}, stats
    return Case(name, ((33, 257), (131, 157)), None, run, None, True, frozenset())


POISON_CASES = [poison_case("terrain-all", ALL, "horn"),
                poison_case("terrain-acc-codes", ("d8_slope", "twi", "spi"), "d8")]
_BASELINE = {}


def poison_baseline(entry, shape):
    key = (entry.name, shape)
    if key not in _BASELINE:
        _BASELINE[key] = execute(entry, inputs("synth", shape), None, False)
    return _BASELINE[key]


@pytest.mark.parametrize("byte", POISON, ids=lambda b: f"poison{b:02X}")
@pytest.mark.parametrize("entry,shape", [(e, s) for e in POISON_CASES for s in e.shapes],
                         ids=lambda v: v.name if isinstance(v, Case) else f"{v[0]}x{v[1]}")
def test_poisoned_workspace_and_outputs_change_no_byte(entry, shape, byte):
    want, want_stats = poison_baseline(entry, shape)
    whole, _ = device("synth", shape, "d8" if "codes" in entry.name else "horn")
    assert_same_bytes(want, {n: whole[n] for n in want}, f"{entry.name} {shape} without poison")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} {shape} under 0x{byte:02X}, out= {whose}"
        got, stats = execute(entry, inputs("synth", shape), byte, own)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
