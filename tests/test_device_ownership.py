"""
Who frees a device raster (the rule: ``backend.result_raster``), operator by operator, with
no GPU: the library is a stand-in that hands out fake addresses and can fail one entry point.

``ROWS`` is the one table of calls, shared with tests/test_gpu_device_ownership.py: every
public operator that allocates device memory, in the forms it has.  Each row is run twice
here -- as it is, and with the entry point it names made to fail -- while a list holds a
strong reference to every raster ``DeviceRaster.empty`` made, so that nothing but an explicit
``free()`` can have released one.  Afterwards every such raster is freed or is one the call
returned or left on the operator for the caller; after a failure none is left; a raster the
test passed in (an operand, an ``out=``) is never freed; and the stand-in's own set of live
addresses says the same.

A row with ``rejected=True`` fails by itself on the real library (an even window, a byte
that is no D8 code ...): here its entry point is made to fail like any other, and the GPU
module runs it as it is.
"""
import collections
import ctypes
import functools
import types

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import assembly, backend
from hydrodem_amd.filters import ComposedFilter, ComposedFilterResults, LazyResults
from test_flowacc import random_acyclic_codes

SHAPE = (70, 90)            # crosses a 64-cell tile seam both ways, with partial tiles
DESTRIPE = (150, 168)       # the smallest raster whose quadrants take the destripe's window
E, W_ = 1, 16


@functools.lru_cache(maxsize=None)
def operands():
    """The host operands of the table (read-only: rows that write take a copy)."""
    dem = hdem_synth.synth_dem(*SHAPE)
    hs = hdem_synth.synth_hsheds(*SHAPE)
    groves = hdem_synth.synth_groves(*SHAPE)
    codes = random_acyclic_codes(*SHAPE, seed=5, ramp=True)
    bad = codes.copy()
    bad[40, 70] = 3                                     # SE | E: no D8 code
    seeds = np.zeros(SHAPE, np.uint32)
    seeds[::9, ::11] = np.arange(1, 8 * 9 + 1, dtype=np.uint32).reshape(8, 9)
    mask = (np.asarray(groves) != 0).astype(np.uint8)
    rivers = np.zeros(SHAPE, np.uint8)
    rivers[35] = 1
    o = types.SimpleNamespace(
        dem=dem, hs=hs, groves=groves, codes=codes, bad_codes=bad, seeds=seeds, mask=mask,
        rivers=rivers, cycle=np.array([[E, W_]], np.uint8),
        striped=hdem_synth.synth_striped_dem(*DESTRIPE),
        spectrum=np.abs(np.fft.fft2(dem)).astype(np.float32),
        streams=(mask & 1).astype(bool))
    for a in vars(o).values():
        a.setflags(write=False)
    return o


Row = collections.namedtuple("Row", "name fail call rejected", defaults=(False,))
# call(o, up) -> (result, operator or None); ``up(array)`` uploads an operand that is the
# test's (never to be freed by the call), ``up.empty(shape, dtype)`` makes an ``out=`` raster


def _op(operator, method, *args):
    return getattr(operator, method)(*args), operator


def _chain(cls, *members):
    chain = cls()
    chain.filters = list(members)
    return chain


def _three(cls, second):
    return _chain(cls, hd.PostProcessingFinal(), second, hd.D8FlowDirection())


def _copy_rate():
    try:
        return backend.copy_rate(nbytes=1 << 20, reps=1)
    finally:
        backend.context().profile(False)        # (copy_rate leaves the timers on)


B = backend
ROWS = [
    # ---- host forms: NumPy in, NumPy out
    Row("LagoonsDetection.apply", "hdem_lagoons_detection_f32_dev",
        lambda o, up: _op(hd.LagoonsDetection(), "apply", o.hs.copy())),
    Row("LagoonsDetection.apply[float64]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.LagoonsDetection(), "apply", o.hs.astype(np.float64))),
    Row("MajorityFilter.apply", "hdem_majority_f32_dev",
        lambda o, up: _op(hd.MajorityFilter(window_size=11), "apply", o.hs)),
    Row("TidyingLagoons.apply", "hdem_tidying_lagoons_f32_dev",
        lambda o, up: _op(hd.TidyingLagoons(), "apply", o.hs)),
    Row("ExpandFilter.apply", "hdem_expand_u8_dev",
        lambda o, up: _op(hd.ExpandFilter(window_size=7), "apply", o.mask.astype(np.float64))),
    Row("BlanksFourier.apply", "hdem_blanks_fourier_f32_dev",
        lambda o, up: _op(hd.BlanksFourier(window_size=55), "apply", o.spectrum)),
    Row("IsolatedPoints.apply", "hdem_isolated_points_u8_dev",
        lambda o, up: _op(hd.IsolatedPoints(window_size=3), "apply", o.mask.astype(np.float64))),
    Row("BinaryErosion.apply", "hdem_binary_erosion_u8_dev",
        lambda o, up: _op(hd.BinaryErosion(iterations=2), "apply", o.mask)),
    Row("BinaryClosing.apply", "hdem_binary_closing_u8_dev",
        lambda o, up: _op(hd.BinaryClosing(), "apply", o.mask)),
    Row("GreyDilation.apply", "hdem_grey_dilation_f32_dev",
        lambda o, up: _op(hd.GreyDilation(size=(7, 7)), "apply", o.hs)),
    Row("GreyDilation.apply[download]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.GreyDilation(size=(7, 7)), "apply", o.hs)),
    Row("CorrectNANValues.apply", "hdem_correct_nan_f32_dev",
        lambda o, up: _op(hd.CorrectNANValues(), "apply", o.hs.copy())),
    Row("CorrectNANValues.apply[float64]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.CorrectNANValues(), "apply", o.hs.astype(np.float64))),
    Row("CorrectNANValues.apply[even window]", "hdem_correct_nan_f32_dev",
        lambda o, up: _op(hd.CorrectNANValues(window_size=4), "apply", o.hs.copy()), True),
    Row("MajorityFilter.apply[window too high]", "hdem_majority_f32_dev",
        lambda o, up: _op(hd.MajorityFilter(window_size=71), "apply", o.hs), True),
    Row("FourierTransform.apply", "hdem_fft2_c2c_f32_dev",
        lambda o, up: _op(hd.FourierTransform(), "apply", o.dem)),
    Row("FourierITransform.apply", "hdem_fft2_c2c_f64_dev",
        lambda o, up: _op(hd.FourierITransform(), "apply", o.dem.astype(np.complex128))),
    Row("HydroConditioning.apply", "hdem_sinkfill_d8_f32_dev",
        lambda o, up: _op(hd.HydroConditioning(), "apply", o.dem)),
    Row("HydroConditioning.apply[resolve]", "hdem_resolve_flats_u8_dev",
        lambda o, up: _op(hd.HydroConditioning(flats="resolve"), "apply", o.dem)),
    Row("DemToHAND.apply", "hdem_flowtrace_u8_dev",
        lambda o, up: _op(hd.DemToHAND(threshold=20), "apply", o.dem)),
    Row("DemToHAND.apply[keep]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.DemToHAND(threshold=20, keep_partial_results=True), "apply",
                          o.dem)),
    Row("ComposedFilter.apply", "hdem_boxmean3_f32_dev",
        lambda o, up: _op(_chain(ComposedFilter, hd.QuadraticFilter(window_size=15),
                                 hd.PostProcessingFinal()), "apply", o.dem)),
    Row("assembly.final_dem", "hdem_boxmean3_f64_dev",
        lambda o, up: (assembly.final_dem(o.dem, o.mask, o.hs, o.hs * o.mask, o.rivers,
                                          keep_terms=True), None)),
    Row("assembly.final_dem[sum]", "hdem_elementwise_dev",
        lambda o, up: (assembly.final_dem(o.dem, o.mask, o.hs, o.hs * o.mask, o.rivers), None)),
    Row("backend.blanks_fourier", "hdem_memcpy_d2h",
        lambda o, up: (B.blanks_fourier(o.spectrum), None)),
    Row("backend.isolated_points", "hdem_isolated_points_u8_dev",
        lambda o, up: (B.isolated_points(o.mask), None)),
    Row("backend.expand", "hdem_elementwise_dev",
        lambda o, up: (B.expand(o.dem, 13, np.float64), None)),
    Row("backend.fft2", "hdem_fft2_c2c_f32_dev", lambda o, up: (B.fft2(o.dem, True), None)),
    Row("backend.widened_to_host", "hdem_memcpy_d2h",
        lambda o, up: (B.widened_to_host(up(o.mask), np.int64), None)),
    Row("backend.copy_rate", "hdem_copy_rate_dev", lambda o, up: (_copy_rate(), None)),
    # ---- device forms of the operators
    Row("DemToHAND.apply_device", "hdem_flowacc_u8_dev",
        lambda o, up: _op(hd.DemToHAND(threshold=20), "apply_device", up(o.dem))),
    Row("DemToHAND.apply_device[keep]", "hdem_flowtrace_u8_dev",
        lambda o, up: _op(hd.DemToHAND(threshold=20, keep_partial_results=True),
                          "apply_device", up(o.dem))),
    Row("DemToHAND.apply_device[keep, resolve]", "hdem_resolve_flats_u8_dev",
        lambda o, up: _op(hd.DemToHAND(threshold=20, keep_partial_results=True, epsilon=0.0,
                                       flats="resolve"), "apply_device", up(o.dem))),
    Row("HeightAboveDrainage.apply_device[keep]", "hdem_flowtrace_u8_dev",
        lambda o, up: _op(hd.HeightAboveDrainage(dem=o.dem, streams=o.streams,
                                                 keep_partial_results=True),
                          "apply_device", up(o.codes))),
    Row("FlowDistance.apply_device", "hdem_flowtrace_u8_dev",
        lambda o, up: _op(hd.FlowDistance(o.streams), "apply_device", up(o.codes))),
    Row("ResolveFlats.apply_device[keep]", "hdem_resolve_flats_u8_dev",
        lambda o, up: _op(hd.ResolveFlats(dem=o.dem, keep_partial_results=True),
                          "apply_device", up(o.codes))),
    Row("Watersheds.apply_device[pour points]", "hdem_watershed_u8_dev",
        lambda o, up: _op(hd.Watersheds(pour_points=o.seeds), "apply_device", up(o.codes))),
    Row("Watersheds.apply_device[compact]", "hdem_memcpy_d2h",
        lambda o, up: _op(hd.Watersheds(labels="compact"), "apply_device", up(o.codes))),
    Row("FlowAccumulation.apply_device", "hdem_flowacc_u8_dev",
        lambda o, up: _op(hd.FlowAccumulation(), "apply_device", up(o.codes))),
    Row("GrovesCorrection.apply_device", "hdem_groves_f32_dev",
        lambda o, up: _op(hd.GrovesCorrection(o.groves), "apply_device", up(o.dem))),
    Row("GrovesCorrectionsIter.apply_device", "hdem_groves_f32_dev",
        lambda o, up: _op(hd.GrovesCorrectionsIter(o.groves, 3), "apply_device", up(o.dem))),
    Row("ProductFilter.apply_device[host factor]", "hdem_elementwise_dev",
        lambda o, up: _op(hd.ProductFilter(factor=o.dem), "apply_device", up(o.mask))),
    Row("DetectApplyFourier.apply_device", "hdem_fourier_destripe_f32_dev",
        lambda o, up: _op(hd.DetectApplyFourier(), "apply_device", up(o.striped))),
    Row("DetectApplyFourier.apply_device[window too high]", "hdem_fourier_destripe_f32_dev",
        lambda o, up: _op(hd.DetectApplyFourier(), "apply_device", up(o.dem)), True),
    Row("ComposedFilter.apply_device", "hdem_d8_f32_dev",
        lambda o, up: _op(_three(ComposedFilter, hd.QuadraticFilter(window_size=15)),
                          "apply_device", up(o.dem))),
    Row("ComposedFilter.apply_device[the second member raises]", "hdem_quadratic_f32_dev",
        lambda o, up: _op(_three(ComposedFilter, hd.QuadraticFilter(window_size=4)),
                          "apply_device", up(o.dem)), True),
    Row("ComposedFilterResults.apply_device", "hdem_d8_f32_dev",
        lambda o, up: _op(_three(ComposedFilterResults, hd.QuadraticFilter(window_size=15)),
                          "apply_device", up(o.dem))),
    Row("ComposedFilterResults.apply_device[the second member raises]",
        "hdem_quadratic_f32_dev",
        lambda o, up: _op(_three(ComposedFilterResults, hd.QuadraticFilter(window_size=4)),
                          "apply_device", up(o.dem)), True),
    # ---- backend.*_dev
    Row("d8_dev", "hdem_d8_f32_dev", lambda o, up: (B.d8_dev(up(o.dem)), None)),
    Row("d8_dev[out]", "hdem_d8_f32_dev",
        lambda o, up: (B.d8_dev(up(o.dem), out=up.empty(SHAPE, np.uint8)), None)),
    Row("flowacc_dev", "hdem_flowacc_u8_dev", lambda o, up: (B.flowacc_dev(up(o.codes)), None)),
    Row("flowacc_dev[no D8 code]", "hdem_flowacc_u8_dev",
        lambda o, up: (B.flowacc_dev(up(o.bad_codes)), None), True),
    Row("flowacc_dev[cycle]", "hdem_flowacc_u8_dev",
        lambda o, up: (B.flowacc_dev(up(o.cycle)), None), True),
    Row("watershed_dev", "hdem_watershed_u8_dev",
        lambda o, up: (B.watershed_dev(up(o.codes), up(o.seeds)), None)),
    Row("watershed_dev[compact]", "hdem_watershed_u8_dev",
        lambda o, up: (B.watershed_dev(up(o.codes), compact=True), None)),
    Row("watershed_dev[compact, out]", "hdem_memcpy_d2h",
        lambda o, up: (B.watershed_dev(up(o.codes), compact=True,
                                       out=up.empty(SHAPE, np.uint32)), None)),
    Row("watershed_dev[compact, no D8 code]", "hdem_watershed_u8_dev",
        lambda o, up: (B.watershed_dev(up(o.bad_codes), compact=True), None), True),
    Row("watershed_dev[cycle]", "hdem_watershed_u8_dev",
        lambda o, up: (B.watershed_dev(up(o.cycle)), None), True),
    Row("watershed_dev[seeds of another shape]", None,      # (refused before any C call)
        lambda o, up: (B.watershed_dev(up(o.codes), up(o.seeds[:, :-1])), None), True),
    Row("flowtrace_dev", "hdem_flowtrace_u8_dev",
        lambda o, up: (B.flowtrace_dev(up(o.codes), up(o.mask), dem=up(o.dem),
                                       want=[n for n, _ in B.FT_OUTPUTS]), None)),
    Row("flowtrace_dev[no D8 code]", "hdem_flowtrace_u8_dev",
        lambda o, up: (B.flowtrace_dev(up(o.bad_codes), want=("stop", "distance")), None),
        True),
    Row("flowtrace_dev[cycle]", "hdem_flowtrace_u8_dev",
        lambda o, up: (B.flowtrace_dev(up(o.cycle), want=("stop", "distance")), None), True),
    Row("resolve_flats_dev", "hdem_resolve_flats_u8_dev",
        lambda o, up: (B.resolve_flats_dev(up(o.codes), up(o.dem), want_distance=True), None)),
    Row("resolve_flats_dev[out]", "hdem_resolve_flats_u8_dev",
        lambda o, up: (B.resolve_flats_dev(up(o.codes), up(o.dem), want_distance=True,
                                           out=up.empty(SHAPE, np.uint8)), None)),
    Row("resolve_flats_dev[no D8 code]", "hdem_resolve_flats_u8_dev",
        lambda o, up: (B.resolve_flats_dev(up(o.bad_codes), up(o.dem), True), None), True),
    Row("sinkfill_dev", "hdem_sinkfill_f32_dev",
        lambda o, up: (B.sinkfill_dev(up(o.dem)), None)),
    Row("sinkfill_d8_dev", "hdem_sinkfill_d8_f32_dev",
        lambda o, up: (B.sinkfill_d8_dev(up(o.dem)), None)),
    Row("sinkfill_d8_dev[codes]", "hdem_sinkfill_d8_f32_dev",
        lambda o, up: (B.sinkfill_d8_dev(up(o.dem), codes=up.empty(SHAPE, np.uint8)), None)),
    Row("blockmax_dev", "hdem_blockmax_f32_dev",
        lambda o, up: (B.blockmax_dev(up(o.dem), 8), None)),
    Row("elementwise_dev", "hdem_elementwise_dev",
        lambda o, up: (B.elementwise_dev(B.EW_ADD, up(o.dem), up(o.hs)), None)),
    Row("fourier_destripe_dev", "hdem_fourier_destripe_f32_dev",
        lambda o, up: (B.fourier_destripe_dev(up(o.striped),
                                              mask=up.empty(DESTRIPE, np.uint8)), None)),
    Row("blanks_fourier_dev", "hdem_blanks_fourier_f32_dev",
        lambda o, up: (B.blanks_fourier_dev(up(o.spectrum)), None)),
    Row("isolated_points_dev", "hdem_isolated_points_u8_dev",
        lambda o, up: (B.isolated_points_dev(up(o.mask)), None)),
    Row("expand_dev", "hdem_expand_u8_dev", lambda o, up: (B.expand_dev(up(o.mask)), None)),
    Row("correct_nan_dev", "hdem_correct_nan_f32_dev",
        lambda o, up: (B.correct_nan_dev(up(o.hs)), None)),
    Row("majority_dev", "hdem_majority_f32_dev",
        lambda o, up: (B.majority_dev(up(o.hs)), None)),
    Row("majority_dev[even window]", "hdem_majority_f32_dev",
        lambda o, up: (B.majority_dev(up(o.hs), 4), None), True),
    Row("binary_erosion_dev", "hdem_binary_erosion_u8_dev",
        lambda o, up: (B.binary_erosion_dev(up(o.mask), 2), None)),
    Row("binary_erosion_dev[synchronize]", "hdem_synchronize",
        lambda o, up: (B.binary_erosion_dev(up(o.mask), 2), None)),
    Row("binary_closing_dev", "hdem_binary_closing_u8_dev",
        lambda o, up: (B.binary_closing_dev(up(o.mask)), None)),
    Row("grey_dilation_dev", "hdem_grey_dilation_f32_dev",
        lambda o, up: (B.grey_dilation_dev(up(o.hs), 7), None)),
    Row("tidying_lagoons_dev", "hdem_tidying_lagoons_f32_dev",
        lambda o, up: (B.tidying_lagoons_dev(up(o.hs)), None)),
    Row("lagoons_detection_dev", "hdem_lagoons_detection_f32_dev",
        lambda o, up: (B.lagoons_detection_dev(up(o.hs)), None)),
    Row("boxmean3_dev", "hdem_boxmean3_f32_dev",
        lambda o, up: (B.boxmean3_dev(up(o.dem)), None)),
    Row("quadratic_dev", "hdem_quadratic_f32_dev",
        lambda o, up: (B.quadratic_dev(up(o.dem)), None)),
    Row("quadratic_dev[even window]", "hdem_quadratic_f32_dev",
        lambda o, up: (B.quadratic_dev(up(o.dem), 4), None), True),
    Row("groves_dev", "hdem_groves_f32_dev",
        lambda o, up: (B.groves_dev(up(o.dem), up(o.mask), iterations=3), None)),
    Row("groves_dev[out, scratch]", "hdem_groves_f32_dev",
        lambda o, up: (B.groves_dev(up(o.dem), up(o.mask), iterations=3,
                                    out=up.empty(SHAPE, np.float32),
                                    scratch=up.empty(SHAPE, np.float32)), None)),
]
ROW_IDS = [row.name for row in ROWS]
assert len(set(ROW_IDS)) == len(ROWS)


# ---------------------------------------------------------------------------
# the bookkeeping, shared with the GPU module
# ---------------------------------------------------------------------------
class Tracker:
    """``made``: every raster ``DeviceRaster.empty`` made since the last ``up`` of a call,
    held strongly; ``given``: the rasters that are the test's."""

    def __init__(self, monkeypatch):
        self.made, self.given = [], []
        real = backend.DeviceRaster.empty.__func__

        def empty(cls, shape, dtype, ctx=None):
            raster = real(cls, shape, dtype, ctx)
            self.made.append(raster)
            return raster
        monkeypatch.setattr(backend.DeviceRaster, "empty", classmethod(empty))

    def empty(self, shape, dtype):
        raster = backend.DeviceRaster.empty(shape, dtype)
        self.given.append(self.made.pop())
        return raster

    def __call__(self, array):
        raster = backend.DeviceRaster.from_host(array)
        self.given.append(self.made.pop())
        return raster

    def live(self):
        return [r for r in self.made if r.ptr is not None]


def handed_over(result, operator):
    """The device rasters a call returned or left on its operator for the caller."""
    found = []

    def walk(x):
        if isinstance(x, backend.DeviceRaster):
            found.append(x)
        elif isinstance(x, LazyResults):                # (without downloading its stages)
            walk(list(x.device.values()))
        elif isinstance(x, dict):
            walk(list(x.values()))
        elif isinstance(x, (tuple, list)):
            for v in x:
                walk(v)
    walk(result)
    for name in ("filled", "codes", "accumulation", "distance", "drainage", "results"):
        walk(getattr(operator, name, None))
    return found


def run_row(row, tracker, fails, live_addresses=None, raises=Exception):
    """One call of ``row`` under ``tracker``; the asserts of the module docstring."""
    try:
        result, operator = row.call(operands(), tracker)
    except raises:
        assert fails, f"{row.name} raised"
        # (in the handler: the traceback still holds every frame of the call)
        assert not tracker.live(), f"{row.name}: rasters left after the failure"
        kept = []
    else:
        assert not fails, f"{row.name} did not fail"
        kept = handed_over(result, operator)
        stray = [r for r in tracker.live() if not any(r is k for k in kept)]
        assert not stray, f"{row.name}: {len(stray)} rasters neither freed nor handed over"
    assert all(r.ptr is not None for r in tracker.given), f"{row.name} freed an operand"
    if live_addresses is not None:
        assert live_addresses() == {r.ptr for r in tracker.live() + tracker.given}
    for raster in kept + tracker.given:
        raster.free()


# ---------------------------------------------------------------------------
# the stand-in library
# ---------------------------------------------------------------------------
class StandIn:
    """An object whose attributes are the C entry points: ``hdem_malloc`` hands out fake
    addresses, ``hdem_free`` forgets them, ``hdem_host_alloc`` fails, ``fail`` returns
    BAD_ARG and everything else OK without touching its arguments."""

    def __init__(self, fail=None):
        self.fail, self.live, self.log, self.next = fail, set(), [], 0x10000

    def __getattr__(self, name):
        if not name.startswith("hdem_"):
            raise AttributeError(name)

        def entry(*args):
            self.log.append(name)
            if name == "hdem_last_error":
                return b"made to fail"
            if name == self.fail:
                return backend.BAD_ARG
            if name == "hdem_malloc":
                self.next += 0x10000
                self.live.add(self.next)
                args[2]._obj.value = self.next
            elif name == "hdem_free":
                self.live.remove(args[1])
            elif name == "hdem_host_alloc":
                return backend.OOM
            return backend.OK
        return entry


@pytest.fixture
def stand_in(monkeypatch):
    lib = StandIn()
    ctx = backend.Context.__new__(backend.Context)
    ctx.lib, ctx.handle, ctx.device = lib, ctypes.c_void_p(1), 0
    monkeypatch.setattr(backend, "context", lambda device=None: ctx)
    return lib, Tracker(monkeypatch)


@pytest.mark.parametrize("row", [r for r in ROWS if not r.rejected],
                         ids=[r.name for r in ROWS if not r.rejected])
def test_a_call_frees_what_it_does_not_hand_over(row, stand_in):
    lib, tracker = stand_in
    run_row(row, tracker, False, lambda: lib.live)
    assert not lib.live


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_a_failing_call_frees_everything_it_made(row, stand_in):
    lib, tracker = stand_in
    lib.fail = row.fail
    run_row(row, tracker, True, lambda: lib.live)
    assert (row.fail is None or row.fail in lib.log) and not lib.live


def test_to_host_writes_into_a_given_array(stand_in):
    _, tracker = stand_in
    with tracker.empty((3, 5), np.float32) as raster:
        out = np.zeros((3, 5), np.float32)
        assert raster.to_host(out) is out
        for wrong in (np.zeros((3, 5), np.float64), np.zeros((3, 4), np.float32),
                      np.zeros((5, 6), np.float32)[:3, :5]):
            with pytest.raises(ValueError):
                raster.to_host(wrong)
