"""
The terrain attributes of a float32 catchment area (``hdem_terrain_area_f32[_dev]``,
``AreaWetnessIndex``) on the MI355X, against the reference of tests/test_terrain_attributes.py
as tests/test_dinfsum.py applies it to an area.

Shapes, rasters and bars are those of tests/test_gpu_terrain_attributes.py, with its anisotropic
cells: ``dzdx``, ``dzdy`` and ``d8_slope`` are the reference's bits, ``tangent`` within 1 ulp,
``spi`` within 2, ``twi`` within ``6 * spacing(float32(max(|want|, 1)))`` of the float64 logarithm
of the reference's own float32 operands -- that file's derivation, which applies unchanged: the
new path makes the same roundings, ``area * cell`` where the other has ``float32(acc) * cell``.
The largest twi error seen is printed (``-s``) and recorded in DESIGN 3.25.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend as B
from hydrodem_amd import terrain as T
from hydrodem_amd.backend import DeviceRaster
from test_dinfsum import area_reference
from test_gpu_scribble import Case, assert_same_bytes, execute
from test_gpu_terrain_attributes import (ALL, DX, DY, MIN_SLOPE, N_ULP, SHAPES, ZF, inputs,
                                         reference, same_bits, ulps_f32, usable, worst)

pytestmark = pytest.mark.gpu

F32 = np.float32
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


@functools.lru_cache(maxsize=None)
def area_inputs(shape):
    """The dem and codes of the other file with a float32 area that is no integer, holds zeros,
    negatives, NaN and 2^40 cells, and a given slope with zeros, negatives, NaN and
    values on both sides of the floor."""
    inp = dict(inputs("synth", shape))
    rng = np.random.default_rng([11, *shape])
    area = (rng.random(shape) * 5000 + 1).astype(F32)
    flat = area.ravel()
    flat[::17] = 0.0
    flat[3::19] = -2.5
    flat[5::23] = np.nan
    flat[7::29] = F32(2.0 ** 40)
    given = (rng.random(shape) * 0.7).astype(F32)
    g = given.ravel()
    g[::13] = 0.0
    g[2::17] = -0.25
    g[4::19] = np.nan
    g[6::23] = F32(5e-4)
    g[8::29] = F32(MIN_SLOPE)                            # the floor itself is not below it
    for a in (area, given):
        a.setflags(write=False)
    inp.update(area=area, given=given)
    return inp


@functools.lru_cache(maxsize=None)
def area_ref(shape, slope):
    inp = area_inputs(shape)
    return area_reference(inp["dem"], inp["area"], DX, DY, ZF, MIN_SLOPE,
                          inp["given"] if slope == "given" else None)


def run_dev(inp, want, slope="horn", out=None, area="area", ctx=None):
    ctx = ctx or B.context()
    with contextlib.ExitStack() as stack:
        def up(a):
            return stack.enter_context(DeviceRaster.from_host(a, dtype=a.dtype, ctx=ctx))
        needs_codes = slope == "d8" or "d8_slope" in want
        needs_area = "twi" in want or "spi" in want
        outs, stats = T.terrain_area_dev(
            up(inp["dem"]), want, (DY, DX), ZF, up(inp[area]) if needs_area else None,
            up(inp["given"]) if slope == "given" else None,
            up(inp["codes"]) if needs_codes else None, MIN_SLOPE, slope, out=out)
        for raster in outs.values():
            stack.enter_context(raster)
        return {name: raster.to_host() for name, raster in outs.items()}, stats


@functools.lru_cache(maxsize=None)
def device(shape, slope="horn"):
    return run_dev(area_inputs(shape), ALL, slope)


def assert_twi(got, ref, keep, what):
    """twi inside the bar over the cells ``keep`` where the reference is a number; NaN where it
    is NaN.  Returns the largest error seen."""
    number = keep & ~np.isnan(ref)
    assert np.isnan(got[keep & np.isnan(ref)]).all(), what
    seen = worst("twi", got, ref, number)
    assert seen <= N_ULP["twi"], (what, seen)
    return seen


@pytest.mark.parametrize("slope", T.AREA_SLOPES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_output_against_the_reference(shape, slope):
    base, ref = reference("synth", shape), area_ref(shape, slope)
    got, stats = device(shape, slope)
    assert same_bits(got["dzdx"], base["dzdx"]) and same_bits(got["dzdy"], base["dzdy"])
    assert same_bits(got["d8_slope"], base["d8_slope"])
    assert ulps_f32(got["tangent"], base["tangent"]) <= 1
    spi_ulp = ulps_f32(got["spi"], ref["spi"])
    fin, left_out = usable(base)
    assert not left_out.any()
    hole = np.isnan(area_inputs(shape)["dem"])
    assert np.isnan(got["twi"][hole]).all() and np.isnan(got["spi"][hole]).all()
    seen = assert_twi(got["twi"], ref["twi"], fin, (shape, slope))
    print(f"\nterrain area ulp {shape} {slope}: spi {spi_ulp:.3f} twi {seen:.3f}")
    assert spi_ulp <= 2
    assert {k: v for k, v in stats.items() if k != "ms_total"} == ref["stats"]
    if min(shape) > 30:
        assert ref["stats"]["nonpositive_area"] > 50 and ref["stats"]["floored_cells"] > 50
        assert np.isnan(ref["twi"][~hole]).any() and np.isinf(ref["twi"]).any()


@pytest.mark.parametrize("shape", [(33, 257), (131, 157)], ids=IDS)
def test_the_given_slope_is_taken_as_it_is(shape):
    inp, ref = area_inputs(shape), area_ref(shape, "given")
    got, stats = device(shape, "given")
    horn, _ = device(shape)
    for name in ("dzdx", "dzdy", "tangent", "degrees", "aspect", "d8_slope"):
        assert_same_bytes({name: got[name]}, {name: horn[name]}, name)
    ok = ~np.isnan(inp["dem"])
    with np.errstate(invalid="ignore"):
        low = (inp["given"] < F32(MIN_SLOPE)) & ok
    assert stats["floored_cells"] == int(low.sum()) > 0
    # spi is one float32 product of the area and the slope as given: zeros, negatives and all
    cell = F32(np.sqrt(DX * DY))
    with np.errstate(all="ignore"):
        want = (inp["area"] * cell) * inp["given"]
    assert ulps_f32(got["spi"][ok], want[ok]) <= 2
    assert np.isnan(got["twi"][np.isnan(inp["given"])]).all()          # a NaN t stays NaN
    assert np.isnan(got["twi"][~ok]).all() and np.isnan(got["spi"][~ok]).all()
    # a floored cell holds what the floor itself would give
    floor_only = dict(inp, given=np.where(low, F32(MIN_SLOPE), inp["given"]).astype(F32))
    again, again_stats = run_dev(floor_only, ("twi",), "given")
    assert_same_bytes({"twi": again["twi"]}, {"twi": got["twi"]}, "floored")
    assert again_stats["floored_cells"] == 0
    assert_twi(got["twi"], ref["twi"], ok, "given")


@pytest.mark.parametrize("slope", T.SLOPES)
@pytest.mark.parametrize("shape", [(1, 9), (33, 257), (131, 157), (70, 515)], ids=IDS)
def test_an_integer_valued_area_gives_the_bytes_of_the_accumulation(shape, slope):
    inp = dict(inputs("synth", shape))
    acc = (inp["acc"] % np.uint32(1 << 24)).astype(np.uint32)
    acc.ravel()[1::7] = (1 << 24) - 1
    inp["acc"], inp["whole"] = acc, acc.astype(F32)
    assert np.array_equal(inp["whole"].astype(np.uint32), acc)
    got, stats = run_dev(inp, ALL, slope, area="whole")
    with DeviceRaster.from_host(inp["dem"], dtype=F32) as dz, \
            DeviceRaster.from_host(inp["codes"], dtype=np.uint8) as dc, \
            DeviceRaster.from_host(acc, dtype=np.uint32) as da:
        outs, want_stats = T.terrain_dev(dz, ALL, (DY, DX), ZF, dc, da, MIN_SLOPE, slope)
        want = {}
        for name, raster in outs.items():
            with raster:
                want[name] = raster.to_host()
    assert_same_bytes(got, want, f"area = float(acc) {shape} {slope}")
    assert {k: v for k, v in stats.items() if k not in ("ms_total", "nonpositive_area")} == \
        {k: v for k, v in want_stats.items() if k != "ms_total"}
    assert stats["nonpositive_area"] == int((acc == 0).sum())


SUBSETS = [("twi",), ("spi",), ("tangent",), ("dzdx", "aspect"), ("tangent", "twi", "spi"),
           ("degrees", "d8_slope", "twi")]


@pytest.mark.parametrize("slope", T.AREA_SLOPES + ("d8",))
@pytest.mark.parametrize("want", SUBSETS, ids="+".join)
def test_a_subset_returns_the_bytes_of_the_call_for_all(want, slope):
    for shape in ((33, 257), (131, 157)):
        whole, _ = device(shape, slope)
        got, _ = run_dev(area_inputs(shape), want, slope)
        assert_same_bytes(got, {name: whole[name] for name in want}, f"{want} {slope} {shape}")


@pytest.mark.parametrize("shape", [(1, 9), (33, 257), (131, 157)], ids=IDS)
def test_the_host_form_and_the_filter_return_the_bytes_of_the_device_form(shape):
    inp = area_inputs(shape)
    for slope in T.AREA_SLOPES:
        want, want_stats = device(shape, slope)
        given = inp["given"] if slope == "given" else None
        got, stats = T.terrain_area(inp["dem"], ALL, (DY, DX), ZF, inp["area"], given,
                                    inp["codes"], MIN_SLOPE, slope)
        assert_same_bytes(got, want, f"host form {shape} {slope}")
        assert {k: v for k, v in stats.items() if k != "ms_total"} == \
            {k: v for k, v in want_stats.items() if k != "ms_total"}
        f = hd.AreaWetnessIndex(inp["area"], given, (DY, DX), ZF, MIN_SLOPE, ("twi", "spi"), True)
        assert_same_bytes({"twi": f.apply(inp["dem"]), "spi": f.spi},
                          {"twi": want["twi"], "spi": want["spi"]}, "AreaWetnessIndex")
        assert f.twi is None and f.stats["nonpositive_area"] == want_stats["nonpositive_area"]


def test_the_library_refuses_before_any_launch():
    ctx = B.context()
    z = np.zeros((4, 4), F32)
    area, given = np.ones((4, 4), F32), np.ones((4, 4), F32)
    codes, out = np.ones((4, 4), np.uint8), np.empty((4, 4), F32)
    null = ctypes.c_void_p()
    ptr = lambda a: null if a is None else a.ctypes.data  # noqa: E731

    def call(a=None, g=None, c=None, outs=(None,) * 8, flags=0, ms=1e-3):
        rc = ctx.lib.hdem_terrain_area_f32(ctx.handle, ptr(z), 4, 4, ptr(a), ptr(g), ptr(c), 1.0,
                                           1.0, 1.0, ms, *[ptr(o) for o in outs], flags, None)
        return rc, ctx.lib.hdem_last_error().decode()
    only = lambda k, o=out: tuple(o if j == k else None for j in range(8))  # noqa: E731
    assert call(outs=only(3))[0] == B.OK
    assert call(a=area, outs=only(6))[0] == B.OK
    assert call(a=area, g=given, outs=only(6), flags=2)[0] == B.OK
    assert call(a=area, g=given, outs=only(3), flags=2)[0] == B.OK        # given, not read
    for kw, text in (
            (dict(), "no output wanted"),
            (dict(outs=only(6)), "twi and spi need the float32 area raster"),
            (dict(outs=only(7), c=codes), "twi and spi need the float32 area raster"),
            (dict(a=area, outs=only(6), flags=2), "HDEM_TERRAIN_TWI_GIVEN needs the float32"),
            (dict(a=area, g=given, outs=only(6)), "goes with HDEM_TERRAIN_TWI_GIVEN"),
            (dict(a=area, g=given, c=codes, outs=only(6), flags=3), "exclude each other"),
            (dict(a=area, outs=only(6), flags=1), "HDEM_TERRAIN_TWI_D8 needs the uint8 D8 codes"),
            (dict(a=area, outs=only(5)), "d8_slope needs the uint8 D8 codes"),
            (dict(a=area, outs=only(6), flags=4), "unknown flags 0x4"),
            (dict(a=area, outs=only(6), ms=0.0), "min_slope must be finite and positive"),
            (dict(a=area, outs=only(6, area)), "twi overlaps area"),
            (dict(a=area, g=given, outs=only(7, given), flags=2), "spi overlaps given_slope"),
            (dict(a=area, outs=(out, out) + (None,) * 6), "dzdy overlaps dzdx")):
        rc, said = call(**kw)
        assert rc == B.BAD_ARG and text in said, (kw, said)
    st = B._TerrainAreaStats()                            # pylint: disable=protected-access
    st.struct_size = 40                                   # the fields of the other struct only
    st.nonpositive_area = -3
    area[0, 0] = 0
    rc = ctx.lib.hdem_terrain_area_f32(ctx.handle, ptr(z), 4, 4, ptr(area), null, null, 1.0, 1.0,
                                       1.0, 1e-3, *[null] * 6, ptr(out), null, 0, ctypes.byref(st))
    assert rc == B.OK and st.flat_cells == 16 and st.floored_cells == 16
    assert st.nonpositive_area == -3 and out[0, 0] == -np.inf


# ---------------------------------------------------------------------------
# poison: the method of tests/test_gpu_scribble.py
# ---------------------------------------------------------------------------
def poison_case(name, want, slope):
    def run(call, inp):
        dem = call.up(inp["dem"])
        out = {n: call.out(dem.shape, F32) for n in want} if call.own else None
        outs, stats = T.terrain_area_dev(
            dem, want, (DY, DX), ZF, call.up(inp["area"]),
            call.up(inp["given"]) if slope == "given" else None, call.up(inp["codes"]),
            MIN_SLOPE, slope, out=out)
        return {n: (r.to_host() if call.own else call.host(r)) for n, r in outs.items()}, stats
    return Case(name, ((33, 257), (131, 157)), None, run, None, True, frozenset())


POISON_CASES = [poison_case("area-all", ALL, "horn"),
                poison_case("area-given", ("d8_slope", "twi", "spi"), "given")]


@pytest.mark.parametrize("byte", (0x00, 0xFF), ids=lambda b: f"poison{b:02X}")
@pytest.mark.parametrize("entry,shape", [(e, s) for e in POISON_CASES for s in e.shapes],
                         ids=lambda v: v.name if isinstance(v, Case) else f"{v[0]}x{v[1]}")
def test_poisoned_workspace_and_outputs_change_no_byte(entry, shape, byte):
    want, want_stats = execute(entry, area_inputs(shape), None, False)
    whole, _ = device(shape, "given" if "given" in entry.name else "horn")
    assert_same_bytes(want, {n: whole[n] for n in want}, f"{entry.name} {shape} without poison")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} {shape} under 0x{byte:02X}, out= {whose}"
        got, stats = execute(entry, area_inputs(shape), byte, own)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
