"""
What the Python binding of the terrain operators (flow accumulation, watersheds, flow trace,
flat resolution, depressions and their table; the chains built on them) asks of the C
library, and what it refuses, with no GPU.

Three tables of literals, recorded before the host and device forms were given one body:

``CALLS`` / ``EXPECTED_CALLS``: every form and mode at 70 x 90 on the stand-in library of
tests/test_device_ownership.py, each C call logged as (entry point, arguments) with an
address reduced to ``"ptr"``, a missing one to ``"null"`` and a stats struct to ``"stats"``.
The operator entry points are compared in order, the allocations and copies as sorted sizes.
The stand-in reports 3 basins and 3 depressions, so that the outlets and the table are
fetched.

``REFUSALS`` / ``EXPECTED_REFUSALS``: bad calls with the exception class and the whole
message, raised while ``backend.context`` fails: no row touches the device.

``NAMES``: ``backend.__all__``.
"""
import ctypes
import functools
import types

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend
from test_device_ownership import SHAPE, StandIn, operands

B = backend
MEMORY = ("hdem_malloc", "hdem_memcpy_h2d", "hdem_memcpy_d2h")


def _reduced(a):
    if a is None:
        return "null"
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if type(a).__name__ == "CArgObject":                # byref(...)
        return "stats"
    if isinstance(a, (int, np.integer)) and not isinstance(a, bool) and a >= 0x10000:
        return "ptr"
    return a


class Recorder(StandIn):
    """The stand-in with every call logged in ``calls``, the context handle left out."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __getattr__(self, name):
        entry = super().__getattr__(name)

        def logged(*args):
            self.calls.append((name,) + tuple(_reduced(a) for a in args[1:]))
            status = entry(*args)
            if name.startswith("hdem_watershed_u8"):
                args[-1]._obj.basins = 3
            if name.startswith("hdem_depressions_f32"):
                args[-1]._obj.depressions = 3
            return status
        return logged

    def record(self):
        """The operator calls in order, and the sizes of the allocations and copies."""
        ops = [c for c in self.calls if c[0] not in MEMORY + ("hdem_free",)]
        sizes = {m: sorted(c[1] if m == "hdem_malloc" else c[3]
                           for c in self.calls if c[0] == m) for m in MEMORY}
        return ops, {m: s for m, s in sizes.items() if s}


def stand_in_context(lib):
    ctx = backend.Context.__new__(backend.Context)
    ctx.lib, ctx.handle, ctx.device = lib, ctypes.c_void_p(1), 0
    return ctx


def device_form(ctx):
    """``dev(array)``: the array's device form, a wrapped raster that owns nothing."""
    def dev(a):
        dtype = np.uint8 if a.dtype == np.bool_ else a.dtype
        return backend.DeviceRaster.wrap(0x10000, a.shape, dtype, ctx=ctx)
    return dev


@functools.lru_cache(maxsize=None)
def call_operands():
    """The operands of the ownership table, and three it has no use for."""
    o = operands()
    return types.SimpleNamespace(**vars(o), acc=np.full(SHAPE, 7, np.uint32),
                                 filled=o.dem + np.float32(1),
                                 labels=np.ones(SHAPE, np.uint32))


def both(name, make, operand):
    """A class through ``apply`` and through ``apply_device``."""
    return [(f"{name}.apply", lambda o, dev: make(o, dev).apply(operand(o))),
            (f"{name}.apply_device", lambda o, dev: make(o, dev).apply_device(dev(operand(o))))]


_codes, _dem, _filled = (lambda o: o.codes), (lambda o: o.dem), (lambda o: o.filled)
ALL = tuple(n for n, _ in B.FT_OUTPUTS)
CALLS = [
    *both("FlowAccumulation", lambda o, dev: hd.FlowAccumulation(), _codes),
    *both("Watersheds", lambda o, dev: hd.Watersheds(), _codes),
    *both("Watersheds[compact]", lambda o, dev: hd.Watersheds(labels="compact"), _codes),
    *both("Watersheds[raster]", lambda o, dev: hd.Watersheds(o.seeds.astype(np.int64)), _codes),
    *both("Watersheds[points]", lambda o, dev: hd.Watersheds([(3, 4), (50, 60, 9)]), _codes),
    *both("Watersheds[device raster]", lambda o, dev: hd.Watersheds(dev(o.seeds)), _codes),
    *both("FlowDistance", lambda o, dev: hd.FlowDistance(), _codes),
    *both("FlowDistance[mask]", lambda o, dev: hd.FlowDistance(o.streams, cellsize=30), _codes),
    *both("FlowDistance[uint32]", lambda o, dev: hd.FlowDistance(o.acc, threshold=20), _codes),
    *both("FlowDistance[device mask]", lambda o, dev: hd.FlowDistance(dev(o.mask)), _codes),
    *both("FlowDistance[device uint32]",
          lambda o, dev: hd.FlowDistance(dev(o.acc), threshold=20.0), _codes),
    *both("HeightAboveDrainage",
          lambda o, dev: hd.HeightAboveDrainage(dem=o.dem, streams=o.streams), _codes),
    *both("HeightAboveDrainage[keep]",
          lambda o, dev: hd.HeightAboveDrainage(dem=o.dem, streams=o.streams, cellsize=30.0,
                                                keep_partial_results=True), _codes),
    *both("HeightAboveDrainage[device operands]",
          lambda o, dev: hd.HeightAboveDrainage(dem=dev(o.dem), streams=dev(o.acc),
                                                threshold=5), _codes),
    *both("ResolveFlats", lambda o, dev: hd.ResolveFlats(dem=o.dem), _codes),
    *both("ResolveFlats[keep]",
          lambda o, dev: hd.ResolveFlats(dem=o.dem, keep_partial_results=True), _codes),
    *both("ResolveFlats[device dem]", lambda o, dev: hd.ResolveFlats(dem=dev(o.dem)), _codes),
    *both("Depressions", lambda o, dev: hd.Depressions(dem=o.dem), _filled),
    *both("Depressions[first]", lambda o, dev: hd.Depressions(dem=o.dem, labels="first"),
          _filled),
    *both("Depressions[table]",
          lambda o, dev: hd.Depressions(dem=o.dem, table=True, cellsize=30.0), _filled),
    *both("Depressions[table, device dem]",
          lambda o, dev: hd.Depressions(dem=dev(o.dem), table=True), _filled),
    *both("DepressionInventory", lambda o, dev: hd.DepressionInventory(cellsize=30.0), _dem),
    *both("DemToHAND", lambda o, dev: hd.DemToHAND(threshold=20), _dem),
    *both("DemToHAND[keep]",
          lambda o, dev: hd.DemToHAND(threshold=20, cellsize=30.0, keep_partial_results=True),
          _dem),
    *both("DemToHAND[resolve]",
          lambda o, dev: hd.DemToHAND(threshold=20, epsilon=0.0, flats="resolve"), _dem),
    *both("DemToHAND[keep, resolve]",
          lambda o, dev: hd.DemToHAND(threshold=20, epsilon=0.0, flats="resolve",
                                      keep_partial_results=True), _dem),
    *both("HydroConditioning", lambda o, dev: hd.HydroConditioning(), _dem),
    *both("HydroConditioning[resolve]",
          lambda o, dev: hd.HydroConditioning(epsilon=0.5, flats="resolve"), _dem),
    # ---- the twelve backend functions
    ("flowacc", lambda o, dev: B.flowacc(o.codes)),
    ("flowacc[stats]", lambda o, dev: B.flowacc(o.codes, return_stats=True)),
    ("flowacc_dev", lambda o, dev: B.flowacc_dev(dev(o.codes))),
    ("flowacc_dev[out]", lambda o, dev: B.flowacc_dev(dev(o.codes), out=dev(o.acc))),
    ("watershed", lambda o, dev: B.watershed(o.codes)),
    ("watershed[seeds]", lambda o, dev: B.watershed(o.codes, o.seeds)),
    ("watershed[compact]", lambda o, dev: B.watershed(o.codes, compact=True)),
    ("watershed_dev", lambda o, dev: B.watershed_dev(dev(o.codes))),
    ("watershed_dev[seeds]", lambda o, dev: B.watershed_dev(dev(o.codes), dev(o.seeds))),
    ("watershed_dev[compact]", lambda o, dev: B.watershed_dev(dev(o.codes), compact=True)),
    ("watershed_dev[compact, out]",
     lambda o, dev: B.watershed_dev(dev(o.codes), compact=True, out=dev(o.acc))),
    ("flowtrace", lambda o, dev: B.flowtrace(o.codes)),
    ("flowtrace[mask, all]",
     lambda o, dev: B.flowtrace(o.codes, o.streams, dem=o.dem, cellsize=30, want=ALL)),
    ("flowtrace[uint32]",
     lambda o, dev: B.flowtrace(o.codes, o.acc, 20, want=("stop", "ndiag"))),
    ("flowtrace[hand]", lambda o, dev: B.flowtrace(o.codes, o.mask, dem=o.dem, want="hand")),
    ("flowtrace_dev", lambda o, dev: B.flowtrace_dev(dev(o.codes))),
    ("flowtrace_dev[mask, all]",
     lambda o, dev: B.flowtrace_dev(dev(o.codes), dev(o.streams), dem=dev(o.dem), cellsize=30,
                                    want=ALL)),
    ("flowtrace_dev[uint32]",
     lambda o, dev: B.flowtrace_dev(dev(o.codes), dev(o.acc), 20, want=("stop", "ndiag"))),
    ("flowtrace_dev[hand]",
     lambda o, dev: B.flowtrace_dev(dev(o.codes), dev(o.mask), dem=dev(o.dem), want="hand")),
    ("resolve_flats", lambda o, dev: B.resolve_flats(o.codes, o.dem)),
    ("resolve_flats[distance]", lambda o, dev: B.resolve_flats(o.codes, o.dem, True)),
    ("resolve_flats_dev", lambda o, dev: B.resolve_flats_dev(dev(o.codes), dev(o.dem))),
    ("resolve_flats_dev[distance]",
     lambda o, dev: B.resolve_flats_dev(dev(o.codes), dev(o.dem), want_distance=True)),
    ("resolve_flats_dev[in place]",
     lambda o, dev: (lambda codes: B.resolve_flats_dev(codes, dev(o.dem), out=codes))(
         dev(o.codes))),
    ("depressions", lambda o, dev: B.depressions(o.dem, o.filled)),
    ("depressions[first]", lambda o, dev: B.depressions(o.dem, o.filled, compact=False)),
    ("depressions_dev", lambda o, dev: B.depressions_dev(dev(o.dem), dev(o.filled))),
    ("depressions_dev[first, out]",
     lambda o, dev: B.depressions_dev(dev(o.dem), dev(o.filled), False, out=dev(o.labels))),
    ("depression_table[3]",
     lambda o, dev: B.depression_table(o.dem, o.filled, o.labels, 3, cellsize=30.0)),
    ("depression_table[0]", lambda o, dev: B.depression_table(o.dem, o.filled, o.labels, 0)),
    ("depression_table_dev[3]",
     lambda o, dev: B.depression_table_dev(dev(o.dem), dev(o.filled), dev(o.labels), 3,
                                           cellsize=30.0)),
    ("depression_table_dev[0]",
     lambda o, dev: B.depression_table_dev(dev(o.dem), dev(o.filled), dev(o.labels), 0)),
]
CALL_IDS = [name for name, _ in CALLS]
assert len(set(CALL_IDS)) == len(CALLS)


def recorded(call):
    lib = Recorder()
    ctx = stand_in_context(lib)
    real, backend.context = backend.context, lambda device=None: ctx
    try:
        call(call_operands(), device_form(ctx))
    finally:
        backend.context = real
    return lib.record()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
S = (4, 4)
_c = np.ones(S, np.uint8)
_m = np.zeros(S, np.uint8)
_a = np.ones(S, np.uint32)
_z = np.zeros(S, np.float32)
_l = np.ones(S, np.uint32)
_c3 = np.ones((2, 4, 4), np.uint8)
_z3 = np.zeros((2, 4, 4), np.float32)
_wide = (4, 5)


def _trace_rows(form, fn, x):
    """The refusals of ``flowtrace_args`` through ``fn``; ``x`` makes an operand of the form."""
    rows = [
        ("codes dtype", lambda: fn(x(_c.astype(np.int32)))),
        ("codes 3-D", lambda: fn(x(_c3))),
        ("unknown output", lambda: fn(x(_c), want=("length", "stop"))),
        ("no output", lambda: fn(x(_c), want=())),
        ("threshold alone", lambda: fn(x(_c), threshold=3)),
        ("streams shape", lambda: fn(x(_c), x(np.zeros(_wide, np.uint8)))),
        ("mask with threshold", lambda: fn(x(_c), x(_m), 3)),
        ("uint32 without threshold", lambda: fn(x(_c), x(_a))),
        ("threshold 0", lambda: fn(x(_c), x(_a), 0)),
        ("threshold 2^32", lambda: fn(x(_c), x(_a), 2 ** 32)),
        ("threshold 1.5", lambda: fn(x(_c), x(_a), 1.5)),
        ("threshold True", lambda: fn(x(_c), x(_a), True)),
        ("streams dtype", lambda: fn(x(_c), x(_z), 3)),
        ("dem dtype", lambda: fn(x(_c), dem=x(_z.astype(np.float64)))),
        ("dem shape", lambda: fn(x(_c), dem=x(np.zeros(_wide, np.float32)))),
        ("hand without dem", lambda: fn(x(_c), x(_m), want=("hand",))),
        ("cellsize no number", lambda: fn(x(_c), cellsize="wide")),
        ("cellsize None", lambda: fn(x(_c), cellsize=None)),
        ("cellsize 0", lambda: fn(x(_c), cellsize=0)),
        ("cellsize nan", lambda: fn(x(_c), cellsize=float("nan"))),
        ("cellsize inf", lambda: fn(x(_c), cellsize=float("inf"))),
    ]
    return [(f"{form}[{name}]", call) for name, call in rows]


def _flats_rows(form, fn, x):
    rows = [
        ("codes dtype", lambda: fn(x(_c.astype(np.int8)), x(_z))),
        ("codes 3-D", lambda: fn(x(_c3), x(_z3))),
        ("no dem", lambda: fn(x(_c), None)),
        ("dem dtype", lambda: fn(x(_c), x(_z.astype(np.float64)))),
        ("dem shape", lambda: fn(x(_c), x(np.zeros(_wide, np.float32)))),
    ]
    return [(f"{form}[{name}]", call) for name, call in rows]


def _depression_rows(form, fn, table, x):
    rows = [
        ("filled dtype", lambda: fn(x(_z), x(_z.astype(np.float64)))),
        ("filled 3-D", lambda: fn(x(_z3), x(_z3))),
        ("no dem", lambda: fn(None, x(_z))),
        ("dem dtype", lambda: fn(x(_a), x(_z))),
        ("dem shape", lambda: fn(x(np.zeros(_wide, np.float32)), x(_z))),
        ("table: filled dtype", lambda: table(x(_z), x(_a), x(_l), 3)),
        ("table: filled 3-D", lambda: table(x(_z3), x(_z3), x(_l), 3)),
        ("table: dem dtype", lambda: table(x(_c), x(_z), x(_l), 3)),
        ("table: dem shape", lambda: table(x(np.zeros(_wide, np.float32)), x(_z), x(_l), 3)),
        ("table: labels dtype", lambda: table(x(_z), x(_z), x(_l.astype(np.int32)), 3)),
        ("table: labels shape", lambda: table(x(_z), x(_z), x(np.ones(_wide, np.uint32)), 3)),
        ("table: count -1", lambda: table(x(_z), x(_z), x(_l), -1)),
        ("table: count 1.5", lambda: table(x(_z), x(_z), x(_l), 1.5)),
        ("table: count True", lambda: table(x(_z), x(_z), x(_l), True)),
    ]
    return [(f"{form}[{name}]", call) for name, call in rows]


def _host(a):
    return a


def _dev(a):
    return a if a is None else backend.DeviceRaster.wrap(0x10000, a.shape, a.dtype,
                                                         ctx=stand_in_context(StandIn()))


def _class_rows(form, x):
    """The refusals of the classes at ``apply`` (``form``) time."""
    run = lambda f, a: getattr(f, form)(x(a))            # noqa: E731
    hand = lambda **k: hd.HeightAboveDrainage(streams=_m, **k)   # noqa: E731
    rows = [
        ("FlowAccumulation: dtype", lambda: run(hd.FlowAccumulation(), _z)),
        ("FlowAccumulation: 3-D", lambda: run(hd.FlowAccumulation(), _c3)),
        ("Watersheds: dtype", lambda: run(hd.Watersheds(), _z)),
        ("Watersheds: 3-D", lambda: run(hd.Watersheds(), _c3)),
        ("Watersheds: point outside", lambda: run(hd.Watersheds([(1, 1), (4, 0)]), _c)),
        ("Watersheds: seeds shape", lambda: run(hd.Watersheds(np.ones(_wide, np.int16)), _c)),
        ("Watersheds: device seeds shape",
         lambda: run(hd.Watersheds(_dev(np.ones(_wide, np.uint32))), _c)),
        ("FlowDistance: dtype", lambda: run(hd.FlowDistance(), _z)),
        ("FlowDistance: 3-D", lambda: run(hd.FlowDistance(_m), _c3)),
        ("FlowDistance: streams shape",
         lambda: run(hd.FlowDistance(np.zeros((3, 4), bool)), _c)),
        ("FlowDistance: device streams shape",
         lambda: run(hd.FlowDistance(_dev(np.ones((3, 4), np.uint32)), threshold=1), _c)),
        ("HeightAboveDrainage: dtype", lambda: run(hand(dem=_z), _a)),
        ("HeightAboveDrainage: 3-D", lambda: run(hand(dem=_z), _c3)),
        ("HeightAboveDrainage: dem shape",
         lambda: run(hand(dem=np.zeros(_wide, np.float32)), _c)),
        ("HeightAboveDrainage: device dem shape",
         lambda: run(hand(dem=_dev(np.zeros(_wide, np.float32))), _c)),
        ("ResolveFlats: dtype", lambda: run(hd.ResolveFlats(dem=_z), _a)),
        ("ResolveFlats: 3-D", lambda: run(hd.ResolveFlats(dem=_z), _c3)),
        ("ResolveFlats: dem shape",
         lambda: run(hd.ResolveFlats(dem=np.zeros(_wide, np.float32)), _c)),
        ("ResolveFlats: device dem shape",
         lambda: run(hd.ResolveFlats(dem=_dev(np.zeros(_wide, np.float32))), _c)),
        ("Depressions: dtype", lambda: run(hd.Depressions(dem=_z), _z.astype(np.float64))),
        ("Depressions: 3-D", lambda: run(hd.Depressions(dem=_z), _z3)),
        ("Depressions: dem shape",
         lambda: run(hd.Depressions(dem=np.zeros(_wide, np.float32)), _z)),
        ("Depressions: device dem shape",
         lambda: run(hd.Depressions(dem=_dev(np.zeros(_wide, np.float32)), table=True), _z)),
        ("DepressionInventory: dtype", lambda: run(hd.DepressionInventory(), _c)),
        ("DepressionInventory: 3-D", lambda: run(hd.DepressionInventory(), _z3)),
        ("DemToHAND: dtype", lambda: run(hd.DemToHAND(threshold=5), _z.astype(np.float64))),
        ("DemToHAND: 3-D", lambda: run(hd.DemToHAND(threshold=5), _z3)),
    ]
    return [(f"{form}[{name}]", call) for name, call in rows]


REFUSALS = [
    # ---- backend: flow accumulation and watersheds
    ("flowacc[dtype]", lambda: B.flowacc(_z)),
    ("flowacc[a list]", lambda: B.flowacc([[1, 2], [4, 8]])),
    ("flowacc[3-D]", lambda: B.flowacc(_c3)),                                   # (new)
    ("flowacc_dev[dtype]", lambda: B.flowacc_dev(_dev(_z))),                    # (new words)
    ("flowacc_dev[3-D]", lambda: B.flowacc_dev(_dev(_c3))),                     # (new)
    ("watershed[dtype]", lambda: B.watershed(_a)),
    ("watershed[3-D]", lambda: B.watershed(_c3)),
    ("watershed[seeds dtype]", lambda: B.watershed(_c, _a.astype(np.int32))),
    ("watershed[seeds shape]", lambda: B.watershed(_c, np.ones(_wide, np.uint32))),
    ("watershed[seeds, compact]", lambda: B.watershed(_c, _a, compact=True)),
    ("watershed_dev[dtype]", lambda: B.watershed_dev(_dev(_a))),                # (new words)
    ("watershed_dev[3-D]", lambda: B.watershed_dev(_dev(_c3))),                 # (new)
    ("watershed_dev[seeds dtype]",                                              # (new words)
     lambda: B.watershed_dev(_dev(_c), _dev(_a.astype(np.int32)))),
    ("watershed_dev[seeds shape]",
     lambda: B.watershed_dev(_dev(_c), _dev(np.ones(_wide, np.uint32)))),
    ("watershed_dev[seeds, compact]", lambda: B.watershed_dev(_dev(_c), _dev(_a), True)),
    # ---- backend: flow trace
    ("flowtrace[codes a list]", lambda: B.flowtrace([[1]])),
    ("flowtrace[streams a list]", lambda: B.flowtrace(_c, [[1]])),
    ("flowtrace[dem a device raster]", lambda: B.flowtrace(_c, dem=_dev(_z))),
    *_trace_rows("flowtrace", B.flowtrace, _host),
    *_trace_rows("flowtrace_dev", B.flowtrace_dev, _dev),
    # ---- backend: flat resolution
    ("resolve_flats[codes a list]", lambda: B.resolve_flats([[1]], _z)),
    ("resolve_flats[dem a device raster]", lambda: B.resolve_flats(_c, _dev(_z))),
    *_flats_rows("resolve_flats", B.resolve_flats, _host),
    *_flats_rows("resolve_flats_dev", B.resolve_flats_dev, _dev),
    # ---- backend: depressions and their table
    ("depressions[dem a list]", lambda: B.depressions([[1.0]], _z)),
    ("depressions[filled a device raster]", lambda: B.depressions(_z, _dev(_z))),
    ("depression_table[dem a list]", lambda: B.depression_table([[1.0]], _z, _l, 3)),
    ("depression_table[filled a list]", lambda: B.depression_table(_z, [[1.0]], _l, 3)),
    ("depression_table[labels missing]", lambda: B.depression_table(_z, _z, None, 3)),
    *_depression_rows("depressions", B.depressions, B.depression_table, _host),
    *_depression_rows("depressions_dev", B.depressions_dev, B.depression_table_dev, _dev),
    # ---- the classes: construction
    ("Watersheds(labels)", lambda: hd.Watersheds(labels="dense")),
    ("Watersheds(compact, points)", lambda: hd.Watersheds([(1, 1)], labels="compact")),
    ("Watersheds(device seeds dtype)", lambda: hd.Watersheds(_dev(_a.astype(np.int64)))),
    ("Watersheds(device seeds 3-D)",
     lambda: hd.Watersheds(_dev(np.ones((2, 4, 4), np.uint32)))),
    ("Watersheds(seeds 1-D)", lambda: hd.Watersheds(np.ones(4, np.uint32))),
    ("Watersheds(seeds float)", lambda: hd.Watersheds(_z)),
    ("Watersheds(seeds negative)", lambda: hd.Watersheds(-_a.astype(np.int32))),
    ("Watersheds(seeds too large)", lambda: hd.Watersheds(_a.astype(np.int64) << 32)),
    ("Watersheds(point of four)", lambda: hd.Watersheds([(1, 1), (1, 2, 3, 4)])),
    ("Watersheds(label 0)", lambda: hd.Watersheds([(1, 1, 0)])),
    ("FlowDistance(streams a list)", lambda: hd.FlowDistance([[0, 1], [1, 0]])),
    ("FlowDistance(streams 1-D)", lambda: hd.FlowDistance(np.zeros(4, np.uint8))),
    ("FlowDistance(streams dtype)", lambda: hd.FlowDistance(np.zeros(S, np.int32))),
    ("FlowDistance(device streams dtype)", lambda: hd.FlowDistance(_dev(_z), threshold=1)),
    ("FlowDistance(uint32 without threshold)", lambda: hd.FlowDistance(_a)),
    ("FlowDistance(mask with threshold)", lambda: hd.FlowDistance(_m != 0, threshold=1)),
    ("FlowDistance(threshold alone)", lambda: hd.FlowDistance(threshold=1)),
    ("FlowDistance(threshold -1)", lambda: hd.FlowDistance(_a, threshold=-1)),
    ("FlowDistance(cellsize no number)", lambda: hd.FlowDistance(cellsize="wide")),
    ("FlowDistance(cellsize -30)", lambda: hd.FlowDistance(cellsize=-30.0)),
    ("HeightAboveDrainage(no dem)", lambda: hd.HeightAboveDrainage(dem=None, streams=_m)),
    ("HeightAboveDrainage(no streams)", lambda: hd.HeightAboveDrainage(dem=_z, streams=None)),
    ("HeightAboveDrainage(dem a list)",
     lambda: hd.HeightAboveDrainage(dem=[[0.0]], streams=_m)),
    ("HeightAboveDrainage(dem 3-D)", lambda: hd.HeightAboveDrainage(dem=_z3, streams=_m)),
    ("HeightAboveDrainage(dem dtype)",
     lambda: hd.HeightAboveDrainage(dem=_z.astype(np.float64), streams=_m)),
    ("HeightAboveDrainage(cellsize inf)",
     lambda: hd.HeightAboveDrainage(dem=_z, streams=_m, cellsize=float("inf"))),
    ("ResolveFlats(no dem)", lambda: hd.ResolveFlats(dem=None)),
    ("ResolveFlats(dem a list)", lambda: hd.ResolveFlats(dem=[[0.0]])),
    ("ResolveFlats(dem 3-D)", lambda: hd.ResolveFlats(dem=_z3)),
    ("ResolveFlats(dem dtype)", lambda: hd.ResolveFlats(dem=_z.astype(np.float64))),
    ("ResolveFlats(device dem dtype)", lambda: hd.ResolveFlats(dem=_dev(_a))),
    ("Depressions(no dem)", lambda: hd.Depressions(dem=None)),
    ("Depressions(dem a list)", lambda: hd.Depressions(dem=[[0.0]])),
    ("Depressions(dem 1-D)", lambda: hd.Depressions(dem=np.zeros(4, np.float32))),
    ("Depressions(dem dtype)", lambda: hd.Depressions(dem=_a)),
    ("Depressions(labels)", lambda: hd.Depressions(dem=_z, labels="outlet")),
    ("Depressions(table of first labels)",
     lambda: hd.Depressions(dem=_z, labels="first", table=True)),
    ("Depressions(cellsize no number)", lambda: hd.Depressions(dem=_z, cellsize=[30])),
    ("Depressions(cellsize 0)", lambda: hd.Depressions(dem=_z, cellsize=0)),
    ("DepressionInventory(epsilon no number)", lambda: hd.DepressionInventory(epsilon="small")),
    ("DepressionInventory(epsilon -1)", lambda: hd.DepressionInventory(epsilon=-1)),
    ("DepressionInventory(epsilon nan)", lambda: hd.DepressionInventory(epsilon=float("nan"))),
    ("DepressionInventory(cellsize nan)",
     lambda: hd.DepressionInventory(cellsize=float("nan"))),
    ("HydroConditioning(flats)", lambda: hd.HydroConditioning(flats="fill")),
    ("HydroConditioning[resolve].apply_batch",
     lambda: hd.HydroConditioning(flats="resolve").apply_batch([_z])),
    ("DemToHAND(flats)", lambda: hd.DemToHAND(threshold=5, flats=None)),
    ("DemToHAND(threshold 0)", lambda: hd.DemToHAND(threshold=0)),
    ("DemToHAND(no threshold)", lambda: hd.DemToHAND(threshold=None)),
    ("DemToHAND(cellsize no number)", lambda: hd.DemToHAND(threshold=5, cellsize="wide")),
    # ---- the classes: the raster they are applied to
    *_class_rows("apply", _host),
    *_class_rows("apply_device", _dev),
]
REFUSAL_IDS = [name for name, _ in REFUSALS]
assert len(set(REFUSAL_IDS)) == len(REFUSALS)


def refused(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    try:
        call()
    except Exception as exc:  # pylint: disable=broad-except
        return type(exc).__name__, str(exc)
    return None


# ---- the recorded tables
EXPECTED_CALLS = {
    'FlowAccumulation.apply': (
        [('hdem_flowacc_u8', 'ptr', 70, 90, 'ptr', 'stats')],
        {}),
    'FlowAccumulation.apply_device': (
        [('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats')],
        {'hdem_malloc': [25200]}),
    'Watersheds.apply': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'null', 0, 'ptr', 'null', 'stats')],
        {}),
    'Watersheds.apply_device': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'null', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200]}),
    'Watersheds[compact].apply': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'null', 1, 'ptr', 'ptr', 'stats')],
        {}),
    'Watersheds[compact].apply_device': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'null', 1, 'ptr', 'ptr', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_d2h': [12]}),
    'Watersheds[raster].apply': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {}),
    'Watersheds[raster].apply_device': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'Watersheds[points].apply': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {}),
    'Watersheds[points].apply_device': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'Watersheds[device raster].apply': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {'hdem_memcpy_d2h': [25200]}),
    'Watersheds[device raster].apply_device': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200]}),
    'FlowDistance.apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'null', 0, 0, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {}),
    'FlowDistance.apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'null', 0, 0, 'null', 1.0, 'null', 'null',
          'null', 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'FlowDistance[mask].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'null', 30.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {}),
    'FlowDistance[mask].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'null', 30.0, 'null', 'null',
          'null', 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [6300, 25200], 'hdem_memcpy_h2d': [6300]}),
    'FlowDistance[uint32].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {}),
    'FlowDistance[uint32].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'null', 'null',
          'null', 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'FlowDistance[device mask].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {'hdem_memcpy_d2h': [6300]}),
    'FlowDistance[device mask].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'FlowDistance[device uint32].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {'hdem_memcpy_d2h': [25200]}),
    'FlowDistance[device uint32].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'null', 'null',
          'null', 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'HeightAboveDrainage.apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {}),
    'HeightAboveDrainage.apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200], 'hdem_memcpy_h2d': [6300, 25200]}),
    'HeightAboveDrainage[keep].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 30.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {}),
    'HeightAboveDrainage[keep].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 30.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200], 'hdem_memcpy_h2d': [6300, 25200]}),
    'HeightAboveDrainage[device operands].apply': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 2, 5, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_memcpy_d2h': [25200, 25200]}),
    'HeightAboveDrainage[device operands].apply_device': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 5, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'ResolveFlats.apply': (
        [('hdem_resolve_flats_u8', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {}),
    'ResolveFlats.apply_device': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [6300, 25200], 'hdem_memcpy_h2d': [25200]}),
    'ResolveFlats[keep].apply': (
        [('hdem_resolve_flats_u8', 'ptr', 'ptr', 70, 90, 'ptr', 'ptr', 0, 'stats')],
        {}),
    'ResolveFlats[keep].apply_device': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'ResolveFlats[device dem].apply': (
        [('hdem_resolve_flats_u8', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {'hdem_memcpy_d2h': [25200]}),
    'ResolveFlats[device dem].apply_device': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [6300]}),
    'Depressions.apply': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats')],
        {}),
    'Depressions.apply_device': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'Depressions[first].apply': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 0, 'ptr', 'stats')],
        {}),
    'Depressions[first].apply_device': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 0, 'ptr', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_h2d': [25200]}),
    'Depressions[table].apply': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr', 'ptr',
          'ptr')],
        {}),
    'Depressions[table].apply_device': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32_dev', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr')],
        {'hdem_malloc': [72, 25200, 25200], 'hdem_memcpy_h2d': [25200], 'hdem_memcpy_d2h': [72]}),
    'Depressions[table, device dem].apply': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr', 'ptr',
          'ptr')],
        {'hdem_memcpy_d2h': [25200]}),
    'Depressions[table, device dem].apply_device': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32_dev', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr')],
        {'hdem_malloc': [72, 25200], 'hdem_memcpy_d2h': [72]}),
    'DepressionInventory.apply': (
        [('hdem_sinkfill_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'stats'),
         ('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32_dev', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr')],
        {'hdem_malloc': [72, 25200, 25200, 25200], 'hdem_memcpy_h2d': [25200], 'hdem_memcpy_d2h':
         [72, 25200, 25200]}),
    'DepressionInventory.apply_device': (
        [('hdem_sinkfill_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'stats'),
         ('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats'),
         ('hdem_depression_table_f32_dev', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr')],
        {'hdem_malloc': [72, 25200, 25200], 'hdem_memcpy_d2h': [72]}),
    'DemToHAND.apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.001, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200], 'hdem_memcpy_h2d': [25200],
         'hdem_memcpy_d2h': [25200]}),
    'DemToHAND.apply_device': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.001, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200]}),
    'DemToHAND[keep].apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.001, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 30.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200, 25200, 25200], 'hdem_memcpy_h2d':
         [25200], 'hdem_memcpy_d2h': [6300, 25200, 25200, 25200, 25200]}),
    'DemToHAND[keep].apply_device': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.001, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 30.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200, 25200]}),
    'DemToHAND[resolve].apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200], 'hdem_memcpy_h2d': [25200],
         'hdem_memcpy_d2h': [25200]}),
    'DemToHAND[resolve].apply_device': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200]}),
    'DemToHAND[keep, resolve].apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200, 25200, 25200], 'hdem_memcpy_h2d':
         [25200], 'hdem_memcpy_d2h': [6300, 25200, 25200, 25200, 25200]}),
    'DemToHAND[keep, resolve].apply_device': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats'),
         ('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats'),
         ('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'ptr', 1.0, 'ptr', 'null', 'null',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200, 25200, 25200, 25200]}),
    'HydroConditioning.apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'ptr', 'stats')],
        {'hdem_malloc': [6300, 25200, 25200], 'hdem_memcpy_h2d': [25200], 'hdem_memcpy_d2h': [6300,
         25200]}),
    'HydroConditioning.apply_device': (
        [('hdem_sinkfill_f32_dev', 'ptr', 70, 90, 0.0, 0, 0, 'ptr', 'stats'),
         ('hdem_d8_f32_dev', 'ptr', 70, 90, 'ptr')],
        {'hdem_malloc': [6300, 25200]}),
    'HydroConditioning[resolve].apply': (
        [('hdem_sinkfill_d8_f32_dev', 'ptr', 70, 90, 0.5, 0, 0, 'ptr', 'ptr', 'stats'),
         ('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [6300, 25200, 25200], 'hdem_memcpy_h2d': [25200], 'hdem_memcpy_d2h': [6300,
         25200]}),
    'HydroConditioning[resolve].apply_device': (
        [('hdem_sinkfill_f32_dev', 'ptr', 70, 90, 0.5, 0, 0, 'ptr', 'stats'),
         ('hdem_d8_f32_dev', 'ptr', 70, 90, 'ptr')],
        {'hdem_malloc': [6300, 25200]}),
    'flowacc': (
        [('hdem_flowacc_u8', 'ptr', 70, 90, 'ptr', 'stats')],
        {}),
    'flowacc[stats]': (
        [('hdem_flowacc_u8', 'ptr', 70, 90, 'ptr', 'stats')],
        {}),
    'flowacc_dev': (
        [('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats')],
        {'hdem_malloc': [25200]}),
    'flowacc_dev[out]': (
        [('hdem_flowacc_u8_dev', 'ptr', 70, 90, 'ptr', 'stats')],
        {}),
    'watershed': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'null', 0, 'ptr', 'null', 'stats')],
        {}),
    'watershed[seeds]': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {}),
    'watershed[compact]': (
        [('hdem_watershed_u8', 'ptr', 70, 90, 'null', 1, 'ptr', 'ptr', 'stats')],
        {}),
    'watershed_dev': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'null', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200]}),
    'watershed_dev[seeds]': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'ptr', 0, 'ptr', 'null', 'stats')],
        {'hdem_malloc': [25200]}),
    'watershed_dev[compact]': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'null', 1, 'ptr', 'ptr', 'stats')],
        {'hdem_malloc': [25200, 25200], 'hdem_memcpy_d2h': [12]}),
    'watershed_dev[compact, out]': (
        [('hdem_watershed_u8_dev', 'ptr', 70, 90, 'null', 1, 'ptr', 'ptr', 'stats')],
        {'hdem_malloc': [25200], 'hdem_memcpy_d2h': [12]}),
    'flowtrace': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'null', 0, 0, 'null', 1.0, 'null', 'null', 'null',
          'ptr', 'null', 0, 'stats')],
        {}),
    'flowtrace[mask, all]': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 30.0, 'ptr', 'ptr', 'ptr', 'ptr',
          'ptr', 0, 'stats')],
        {}),
    'flowtrace[uint32]': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'ptr', 'null', 'ptr',
          'null', 'null', 0, 'stats')],
        {}),
    'flowtrace[hand]': (
        [('hdem_flowtrace_u8', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {}),
    'flowtrace_dev': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'null', 0, 0, 'null', 1.0, 'null', 'null',
          'null', 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'flowtrace_dev[mask, all]': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 30.0, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [25200, 25200, 25200, 25200, 25200]}),
    'flowtrace_dev[uint32]': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 2, 20, 'null', 1.0, 'ptr', 'null', 'ptr',
          'null', 'null', 0, 'stats')],
        {'hdem_malloc': [25200, 25200]}),
    'flowtrace_dev[hand]': (
        [('hdem_flowtrace_u8_dev', 'ptr', 70, 90, 'ptr', 1, 0, 'ptr', 1.0, 'null', 'null', 'null',
          'null', 'ptr', 0, 'stats')],
        {'hdem_malloc': [25200]}),
    'resolve_flats': (
        [('hdem_resolve_flats_u8', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {}),
    'resolve_flats[distance]': (
        [('hdem_resolve_flats_u8', 'ptr', 'ptr', 70, 90, 'ptr', 'ptr', 0, 'stats')],
        {}),
    'resolve_flats_dev': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {'hdem_malloc': [6300]}),
    'resolve_flats_dev[distance]': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'ptr', 0, 'stats')],
        {'hdem_malloc': [6300, 25200]}),
    'resolve_flats_dev[in place]': (
        [('hdem_resolve_flats_u8_dev', 'ptr', 'ptr', 70, 90, 'ptr', 'null', 0, 'stats')],
        {}),
    'depressions': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats')],
        {}),
    'depressions[first]': (
        [('hdem_depressions_f32', 'ptr', 'ptr', 70, 90, 0, 'ptr', 'stats')],
        {}),
    'depressions_dev': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 1, 'ptr', 'stats')],
        {'hdem_malloc': [25200]}),
    'depressions_dev[first, out]': (
        [('hdem_depressions_f32_dev', 'ptr', 'ptr', 70, 90, 0, 'ptr', 'stats')],
        {}),
    'depression_table[3]': (
        [('hdem_depression_table_f32', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr', 'ptr',
          'ptr')],
        {}),
    'depression_table[0]': (
        [],
        {}),
    'depression_table_dev[3]': (
        [('hdem_depression_table_f32_dev', 'ptr', 'ptr', 'ptr', 70, 90, 3, 'ptr', 'ptr', 'ptr',
          'ptr', 'ptr')],
        {'hdem_malloc': [72], 'hdem_memcpy_d2h': [72]}),
    'depression_table_dev[0]': (
        [],
        {}),
}

EXPECTED_REFUSALS = {
    'flowacc[dtype]': ('ValueError', 'flow accumulation takes uint8 D8 codes, got float32'),
    'flowacc[a list]': ('ValueError', 'flow accumulation takes uint8 D8 codes, got int64'),
    # (refused only after the device was touched, before the two forms had one body)
    'flowacc[3-D]': ('ValueError', 'expected a 2-D raster, got shape (2, 4, 4)'),
    # (was 'expected a uint8 raster, got float32')
    'flowacc_dev[dtype]': ('ValueError', 'flow accumulation takes uint8 D8 codes, got float32'),
    # (was left to the library)
    'flowacc_dev[3-D]': ('ValueError', 'expected a 2-D raster, got shape (2, 4, 4)'),
    'watershed[dtype]': ('ValueError', 'watershed labelling takes uint8 D8 codes, got uint32'),
    'watershed[3-D]': ('ValueError', 'expected a 2-D raster, got shape (2, 4, 4)'),
    'watershed[seeds dtype]': ('ValueError', 'seeds are uint32, got int32'),
    'watershed[seeds shape]': ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'watershed[seeds, compact]':
        ('ValueError', 'compact labels number the outlets: no pour points with them'),
    # (was 'expected a uint8 raster, got uint32')
    'watershed_dev[dtype]': ('ValueError', 'watershed labelling takes uint8 D8 codes, got uint32'),
    # (was left to the library)
    'watershed_dev[3-D]': ('ValueError', 'expected a 2-D raster, got shape (2, 4, 4)'),
    # (was 'expected a uint32 raster, got int32')
    'watershed_dev[seeds dtype]': ('ValueError', 'seeds are uint32, got int32'),
    'watershed_dev[seeds shape]': ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'watershed_dev[seeds, compact]':
        ('ValueError', 'compact labels number the outlets: no pour points with them'),
    'flowtrace[codes a list]': ('ValueError', "codes is a NumPy array, got <class 'list'>"),
    'flowtrace[streams a list]': ('ValueError', "streams is a NumPy array, got <class 'list'>"),
    'flowtrace[dem a device raster]':
        ('ValueError', "dem is a NumPy array, got <class 'hydrodem_amd.backend.DeviceRaster'>"),
    'flowtrace[codes dtype]': ('ValueError', 'the flow trace takes uint8 D8 codes, got int32'),
    'flowtrace[codes 3-D]': ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'flowtrace[unknown output]':
        ('ValueError',
         "unknown flow trace outputs ['length']: choose among ['stop', 'ncard', 'ndiag', "
         "'distance', 'hand']"),
    'flowtrace[no output]':
        ('ValueError',
         "no output wanted: choose among ['stop', 'ncard', 'ndiag', 'distance', 'hand']"),
    'flowtrace[threshold alone]':
        ('ValueError', 'a threshold needs the uint32 raster it applies to'),
    'flowtrace[streams shape]': ('ValueError', 'streams are (4, 5), the codes (4, 4)'),
    'flowtrace[mask with threshold]': ('ValueError', 'a uint8 stream mask takes no threshold'),
    'flowtrace[uint32 without threshold]':
        ('ValueError', 'a uint32 stream raster needs a threshold'),
    'flowtrace[threshold 0]': ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 0'),
    'flowtrace[threshold 2^32]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 4294967296'),
    'flowtrace[threshold 1.5]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 1.5'),
    'flowtrace[threshold True]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got True'),
    'flowtrace[streams dtype]':
        ('ValueError',
         'streams are a uint8 mask or a uint32 raster with a threshold, got float32'),
    'flowtrace[dem dtype]': ('ValueError', 'the dem is float32, got float64'),
    'flowtrace[dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'flowtrace[hand without dem]': ('ValueError', 'hand needs the dem it is measured on'),
    'flowtrace[cellsize no number]': ('ValueError', "cellsize is a number, got 'wide'"),
    'flowtrace[cellsize None]': ('ValueError', 'cellsize is a number, got None'),
    'flowtrace[cellsize 0]': ('ValueError', 'cellsize must be finite and positive, got 0.0'),
    'flowtrace[cellsize nan]': ('ValueError', 'cellsize must be finite and positive, got nan'),
    'flowtrace[cellsize inf]': ('ValueError', 'cellsize must be finite and positive, got inf'),
    'flowtrace_dev[codes dtype]': ('ValueError', 'the flow trace takes uint8 D8 codes, got int32'),
    'flowtrace_dev[codes 3-D]':
        ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'flowtrace_dev[unknown output]':
        ('ValueError',
         "unknown flow trace outputs ['length']: choose among ['stop', 'ncard', 'ndiag', "
         "'distance', 'hand']"),
    'flowtrace_dev[no output]':
        ('ValueError',
         "no output wanted: choose among ['stop', 'ncard', 'ndiag', 'distance', 'hand']"),
    'flowtrace_dev[threshold alone]':
        ('ValueError', 'a threshold needs the uint32 raster it applies to'),
    'flowtrace_dev[streams shape]': ('ValueError', 'streams are (4, 5), the codes (4, 4)'),
    'flowtrace_dev[mask with threshold]': ('ValueError', 'a uint8 stream mask takes no threshold'),
    'flowtrace_dev[uint32 without threshold]':
        ('ValueError', 'a uint32 stream raster needs a threshold'),
    'flowtrace_dev[threshold 0]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 0'),
    'flowtrace_dev[threshold 2^32]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 4294967296'),
    'flowtrace_dev[threshold 1.5]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 1.5'),
    'flowtrace_dev[threshold True]':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got True'),
    'flowtrace_dev[streams dtype]':
        ('ValueError',
         'streams are a uint8 mask or a uint32 raster with a threshold, got float32'),
    'flowtrace_dev[dem dtype]': ('ValueError', 'the dem is float32, got float64'),
    'flowtrace_dev[dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'flowtrace_dev[hand without dem]': ('ValueError', 'hand needs the dem it is measured on'),
    'flowtrace_dev[cellsize no number]': ('ValueError', "cellsize is a number, got 'wide'"),
    'flowtrace_dev[cellsize None]': ('ValueError', 'cellsize is a number, got None'),
    'flowtrace_dev[cellsize 0]': ('ValueError', 'cellsize must be finite and positive, got 0.0'),
    'flowtrace_dev[cellsize nan]': ('ValueError', 'cellsize must be finite and positive, got nan'),
    'flowtrace_dev[cellsize inf]': ('ValueError', 'cellsize must be finite and positive, got inf'),
    'resolve_flats[codes a list]': ('ValueError', "codes is a NumPy array, got <class 'list'>"),
    'resolve_flats[dem a device raster]':
        ('ValueError', "dem is a NumPy array, got <class 'hydrodem_amd.backend.DeviceRaster'>"),
    'resolve_flats[codes dtype]': ('ValueError', 'flat resolution takes uint8 D8 codes, got int8'),
    'resolve_flats[codes 3-D]':
        ('ValueError', 'flat resolution takes a 2-D raster, got 3 dimensions'),
    'resolve_flats[no dem]':
        ('ValueError', 'flat resolution needs the dem the codes were made on'),
    'resolve_flats[dem dtype]': ('ValueError', 'the dem is float32, got float64'),
    'resolve_flats[dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'resolve_flats_dev[codes dtype]':
        ('ValueError', 'flat resolution takes uint8 D8 codes, got int8'),
    'resolve_flats_dev[codes 3-D]':
        ('ValueError', 'flat resolution takes a 2-D raster, got 3 dimensions'),
    'resolve_flats_dev[no dem]':
        ('ValueError', 'flat resolution needs the dem the codes were made on'),
    'resolve_flats_dev[dem dtype]': ('ValueError', 'the dem is float32, got float64'),
    'resolve_flats_dev[dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'depressions[dem a list]': ('ValueError', "dem is a NumPy array, got <class 'list'>"),
    'depressions[filled a device raster]':
        ('ValueError', "filled is a NumPy array, got <class 'hydrodem_amd.backend.DeviceRaster'>"),
    'depression_table[dem a list]': ('ValueError', "dem is a NumPy array, got <class 'list'>"),
    'depression_table[filled a list]':
        ('ValueError', "filled is a NumPy array, got <class 'list'>"),
    'depression_table[labels missing]':
        ('ValueError', "labels is a NumPy array, got <class 'NoneType'>"),
    'depressions[filled dtype]': ('ValueError', 'the filled raster is float32, got float64'),
    'depressions[filled 3-D]': ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'depressions[no dem]': ('ValueError', "dem is a NumPy array, got <class 'NoneType'>"),
    'depressions[dem dtype]': ('ValueError', 'the dem is float32, got uint32'),
    'depressions[dem shape]': ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'depressions[table: filled dtype]': ('ValueError', 'the filled raster is float32, got uint32'),
    'depressions[table: filled 3-D]':
        ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'depressions[table: dem dtype]': ('ValueError', 'the dem is float32, got uint8'),
    'depressions[table: dem shape]': ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'depressions[table: labels dtype]': ('ValueError', 'the labels are uint32, got int32'),
    'depressions[table: labels shape]':
        ('ValueError', 'the labels are (4, 5), the filled raster (4, 4)'),
    'depressions[table: count -1]': ('ValueError', 'count is the number of depressions, got -1'),
    'depressions[table: count 1.5]': ('ValueError', 'count is the number of depressions, got 1.5'),
    'depressions[table: count True]':
        ('ValueError', 'count is the number of depressions, got True'),
    'depressions_dev[filled dtype]': ('ValueError', 'the filled raster is float32, got float64'),
    'depressions_dev[filled 3-D]':
        ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'depressions_dev[no dem]':
        ('ValueError', 'depressions need the dem the filled raster is compared with'),
    'depressions_dev[dem dtype]': ('ValueError', 'the dem is float32, got uint32'),
    'depressions_dev[dem shape]': ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'depressions_dev[table: filled dtype]':
        ('ValueError', 'the filled raster is float32, got uint32'),
    'depressions_dev[table: filled 3-D]':
        ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'depressions_dev[table: dem dtype]': ('ValueError', 'the dem is float32, got uint8'),
    'depressions_dev[table: dem shape]':
        ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'depressions_dev[table: labels dtype]': ('ValueError', 'the labels are uint32, got int32'),
    'depressions_dev[table: labels shape]':
        ('ValueError', 'the labels are (4, 5), the filled raster (4, 4)'),
    'depressions_dev[table: count -1]':
        ('ValueError', 'count is the number of depressions, got -1'),
    'depressions_dev[table: count 1.5]':
        ('ValueError', 'count is the number of depressions, got 1.5'),
    'depressions_dev[table: count True]':
        ('ValueError', 'count is the number of depressions, got True'),
    'Watersheds(labels)': ('ValueError', "labels is 'outlet' or 'compact', got 'dense'"),
    'Watersheds(compact, points)':
        ('ValueError',
         'compact labels number the outlets: they cannot be combined with pour points'),
    'Watersheds(device seeds dtype)':
        ('ValueError', 'a device seeds raster is 2-D uint32, got int64 (4, 4)'),
    'Watersheds(device seeds 3-D)':
        ('ValueError', 'a device seeds raster is 2-D uint32, got uint32 (2, 4, 4)'),
    'Watersheds(seeds 1-D)': ('ValueError', 'a seeds raster is 2-D, got 1 dimensions'),
    'Watersheds(seeds float)': ('ValueError', 'a seeds raster has an integer dtype, got float32'),
    'Watersheds(seeds negative)': ('ValueError', 'seed labels must fit uint32'),
    'Watersheds(seeds too large)': ('ValueError', 'seed labels must fit uint32'),
    'Watersheds(point of four)':
        ('ValueError', 'pour point 1 is (row, col) or (row, col, label), got (1, 2, 3, 4)'),
    'Watersheds(label 0)':
        ('ValueError', 'pour point 0: label 0 is not in 1 ... 2^32 - 1 (0 means no pour point)'),
    'FlowDistance(streams a list)':
        ('ValueError', "streams is a NumPy array or a DeviceRaster, got <class 'list'>"),
    'FlowDistance(streams 1-D)': ('ValueError', 'streams is a 2-D raster, got 1 dimensions'),
    'FlowDistance(streams dtype)':
        ('ValueError', 'streams has dtype bool or uint8 or uint32, got int32'),
    'FlowDistance(device streams dtype)':
        ('ValueError', 'streams has dtype bool or uint8 or uint32, got float32'),
    'FlowDistance(uint32 without threshold)':
        ('ValueError', 'a uint32 stream raster needs a threshold'),
    'FlowDistance(mask with threshold)': ('ValueError', 'a uint8 stream mask takes no threshold'),
    'FlowDistance(threshold alone)':
        ('ValueError', 'a threshold needs the uint32 raster it applies to'),
    'FlowDistance(threshold -1)':
        ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got -1'),
    'FlowDistance(cellsize no number)': ('ValueError', "cellsize is a number, got 'wide'"),
    'FlowDistance(cellsize -30)':
        ('ValueError', 'cellsize must be finite and positive, got -30.0'),
    'HeightAboveDrainage(no dem)':
        ('ValueError', 'HeightAboveDrainage needs the dem it is measured on'),
    'HeightAboveDrainage(no streams)':
        ('ValueError',
         'HeightAboveDrainage needs streams (a mask, or a uint32 raster with a threshold)'),
    'HeightAboveDrainage(dem a list)':
        ('ValueError', "dem is a NumPy array or a DeviceRaster, got <class 'list'>"),
    'HeightAboveDrainage(dem 3-D)': ('ValueError', 'dem is a 2-D raster, got 3 dimensions'),
    'HeightAboveDrainage(dem dtype)': ('ValueError', 'dem has dtype float32, got float64'),
    'HeightAboveDrainage(cellsize inf)':
        ('ValueError', 'cellsize must be finite and positive, got inf'),
    'ResolveFlats(no dem)': ('ValueError', 'ResolveFlats needs the dem the codes were made on'),
    'ResolveFlats(dem a list)':
        ('ValueError', "dem is a NumPy array or a DeviceRaster, got <class 'list'>"),
    'ResolveFlats(dem 3-D)': ('ValueError', 'dem is a 2-D raster, got 3 dimensions'),
    'ResolveFlats(dem dtype)': ('ValueError', 'dem has dtype float32, got float64'),
    'ResolveFlats(device dem dtype)': ('ValueError', 'dem has dtype float32, got uint32'),
    'Depressions(no dem)':
        ('ValueError', 'Depressions needs the dem the filled raster is compared with'),
    'Depressions(dem a list)':
        ('ValueError', "dem is a NumPy array or a DeviceRaster, got <class 'list'>"),
    'Depressions(dem 1-D)': ('ValueError', 'dem is a 2-D raster, got 1 dimensions'),
    'Depressions(dem dtype)': ('ValueError', 'dem has dtype float32, got uint32'),
    'Depressions(labels)': ('ValueError', "labels is 'first' or 'compact', got 'outlet'"),
    'Depressions(table of first labels)':
        ('ValueError',
         "the table has one row per compact label: table=True needs labels='compact'"),
    'Depressions(cellsize no number)': ('ValueError', 'cellsize is a number, got [30]'),
    'Depressions(cellsize 0)': ('ValueError', 'cellsize must be finite and positive, got 0.0'),
    'DepressionInventory(epsilon no number)': ('ValueError', "epsilon is a number, got 'small'"),
    'DepressionInventory(epsilon -1)':
        ('ValueError', 'epsilon must be finite and not negative, got -1'),
    'DepressionInventory(epsilon nan)':
        ('ValueError', 'epsilon must be finite and not negative, got nan'),
    'DepressionInventory(cellsize nan)':
        ('ValueError', 'cellsize must be finite and positive, got nan'),
    'HydroConditioning(flats)': ('ValueError', "flats is 'keep' or 'resolve', got 'fill'"),
    'HydroConditioning[resolve].apply_batch':
        ('ValueError',
         "apply_batch does not resolve flats: use apply raster by raster with flats='resolve'"),
    'DemToHAND(flats)': ('ValueError', "flats is 'keep' or 'resolve', got None"),
    'DemToHAND(threshold 0)': ('ValueError', 'threshold is an integer in 1 ... 2^32 - 1, got 0'),
    'DemToHAND(no threshold)': ('ValueError', 'a uint32 stream raster needs a threshold'),
    'DemToHAND(cellsize no number)': ('ValueError', "cellsize is a number, got 'wide'"),
    'apply[FlowAccumulation: dtype]':
        ('ValueError', 'FlowAccumulation takes uint8 D8 codes, got float32'),
    'apply[FlowAccumulation: 3-D]':
        ('ValueError', 'FlowAccumulation takes a 2-D raster, got 3 dimensions'),
    'apply[Watersheds: dtype]': ('ValueError', 'Watersheds takes uint8 D8 codes, got float32'),
    'apply[Watersheds: 3-D]': ('ValueError', 'Watersheds takes a 2-D raster, got 3 dimensions'),
    'apply[Watersheds: point outside]':
        ('ValueError', 'pour point 1 at (4, 0) is outside the 4 x 4 raster'),
    'apply[Watersheds: seeds shape]': ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'apply[Watersheds: device seeds shape]': ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'apply[FlowDistance: dtype]':
        ('ValueError', 'the flow trace takes uint8 D8 codes, got float32'),
    'apply[FlowDistance: 3-D]':
        ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'apply[FlowDistance: streams shape]': ('ValueError', 'streams are (3, 4), the codes (4, 4)'),
    'apply[FlowDistance: device streams shape]':
        ('ValueError', 'streams are (3, 4), the codes (4, 4)'),
    'apply[HeightAboveDrainage: dtype]':
        ('ValueError', 'the flow trace takes uint8 D8 codes, got uint32'),
    'apply[HeightAboveDrainage: 3-D]':
        ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'apply[HeightAboveDrainage: dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply[HeightAboveDrainage: device dem shape]':
        ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply[ResolveFlats: dtype]':
        ('ValueError', 'flat resolution takes uint8 D8 codes, got uint32'),
    'apply[ResolveFlats: 3-D]':
        ('ValueError', 'flat resolution takes a 2-D raster, got 3 dimensions'),
    'apply[ResolveFlats: dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply[ResolveFlats: device dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply[Depressions: dtype]': ('ValueError', 'the filled raster is float32, got float64'),
    'apply[Depressions: 3-D]': ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'apply[Depressions: dem shape]': ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'apply[Depressions: device dem shape]':
        ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'apply[DepressionInventory: dtype]':
        ('ValueError', 'DepressionInventory takes a float32 DEM, got uint8'),
    'apply[DepressionInventory: 3-D]':
        ('ValueError', 'DepressionInventory takes a 2-D raster, got 3 dimensions'),
    'apply[DemToHAND: dtype]': ('ValueError', 'DemToHAND takes a float32 DEM, got float64'),
    'apply[DemToHAND: 3-D]': ('ValueError', 'DemToHAND takes a 2-D raster, got 3 dimensions'),
    'apply_device[FlowAccumulation: dtype]':
        ('ValueError', 'FlowAccumulation takes uint8 D8 codes, got float32'),
    'apply_device[FlowAccumulation: 3-D]':
        ('ValueError', 'FlowAccumulation takes a 2-D raster, got 3 dimensions'),
    'apply_device[Watersheds: dtype]':
        ('ValueError', 'Watersheds takes uint8 D8 codes, got float32'),
    'apply_device[Watersheds: 3-D]':
        ('ValueError', 'Watersheds takes a 2-D raster, got 3 dimensions'),
    'apply_device[Watersheds: point outside]':
        ('ValueError', 'pour point 1 at (4, 0) is outside the 4 x 4 raster'),
    'apply_device[Watersheds: seeds shape]': ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'apply_device[Watersheds: device seeds shape]':
        ('ValueError', 'seeds are (4, 5), the codes (4, 4)'),
    'apply_device[FlowDistance: dtype]':
        ('ValueError', 'the flow trace takes uint8 D8 codes, got float32'),
    'apply_device[FlowDistance: 3-D]':
        ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'apply_device[FlowDistance: streams shape]':
        ('ValueError', 'streams are (3, 4), the codes (4, 4)'),
    'apply_device[FlowDistance: device streams shape]':
        ('ValueError', 'streams are (3, 4), the codes (4, 4)'),
    'apply_device[HeightAboveDrainage: dtype]':
        ('ValueError', 'the flow trace takes uint8 D8 codes, got uint32'),
    'apply_device[HeightAboveDrainage: 3-D]':
        ('ValueError', 'the flow trace takes a 2-D raster, got 3 dimensions'),
    'apply_device[HeightAboveDrainage: dem shape]':
        ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply_device[HeightAboveDrainage: device dem shape]':
        ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply_device[ResolveFlats: dtype]':
        ('ValueError', 'flat resolution takes uint8 D8 codes, got uint32'),
    'apply_device[ResolveFlats: 3-D]':
        ('ValueError', 'flat resolution takes a 2-D raster, got 3 dimensions'),
    'apply_device[ResolveFlats: dem shape]': ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply_device[ResolveFlats: device dem shape]':
        ('ValueError', 'the dem is (4, 5), the codes (4, 4)'),
    'apply_device[Depressions: dtype]':
        ('ValueError', 'the filled raster is float32, got float64'),
    'apply_device[Depressions: 3-D]':
        ('ValueError', 'depressions take a 2-D raster, got 3 dimensions'),
    'apply_device[Depressions: dem shape]':
        ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'apply_device[Depressions: device dem shape]':
        ('ValueError', 'the dem is (4, 5), the filled raster (4, 4)'),
    'apply_device[DepressionInventory: dtype]':
        ('ValueError', 'DepressionInventory takes a float32 DEM, got uint8'),
    'apply_device[DepressionInventory: 3-D]':
        ('ValueError', 'DepressionInventory takes a 2-D raster, got 3 dimensions'),
    'apply_device[DemToHAND: dtype]': ('ValueError', 'DemToHAND takes a float32 DEM, got float64'),
    'apply_device[DemToHAND: 3-D]':
        ('ValueError', 'DemToHAND takes a 2-D raster, got 3 dimensions'),
}

NAMES = ['BAD_ARG', 'BackendError', 'Context', 'DEPR_COLUMNS', 'DEPR_COMPACT', 'DepressionsStats',
 'DeviceRaster', 'EW_ADD', 'EW_GT', 'EW_LT', 'EW_MUL', 'EW_NONZERO', 'EW_RSUB', 'FILL_ACT_BOTTOM',
 'FILL_ACT_TOP', 'FILL_DEFER', 'FILL_GHOST_BOTTOM', 'FILL_GHOST_GIVEN', 'FILL_GHOST_TOP',
 'FILL_INIT', 'FILL_NO_COARSE', 'FILL_NO_VERIFY', 'FILL_RESUME', 'FILL_SYNC_ONLY', 'FILL_WARM',
 'FT_OUTPUTS', 'FT_STREAMS_ACC_U32', 'FT_STREAMS_MASK_U8', 'FT_STREAMS_NONE', 'FillStats',
 'FlowAccStats', 'FlowTraceStats', 'HIP_ERR', 'HydroDEMException', 'K_BLOCKMAX', 'K_BOXMEAN',
 'K_CONVOLVE', 'K_COPY', 'K_D8', 'K_ELEMENTWISE', 'K_FFT', 'K_FILL_COARSE', 'K_FILL_FLAT',
 'K_FILL_HUB', 'K_FILL_INIT', 'K_FILL_ROUND', 'K_FILL_TILE', 'K_FLOWACC', 'K_FOURIER_DETECT',
 'K_FOURIER_MASK', 'K_FOURIER_POINT', 'K_FOURIER_ROWSUM', 'K_GROVES', 'K_LAGOON', 'K_MAJORITY',
 'KernelStat', 'LIB_PATH', 'NOT_CONVERGED', 'NO_DEVICE', 'NotConvergedError', 'OK', 'OOM',
 'OTHER_SYMBOLS', 'ResolveFlatsStats', 'SIGNATURES', 'WINDOW_EVEN', 'WINDOW_HIGH', 'WS_COMPACT',
 'WatershedStats', 'WindowSizeEvenError', 'WindowSizeHighError', 'around', 'binary_closing_dev',
 'binary_erosion_dev', 'blanks_fourier', 'blanks_fourier_dev', 'blockmax_dev', 'boxmean3',
 'boxmean3_dev', 'context', 'contextlib', 'convolve', 'copy_rate', 'correct_nan_dev', 'ctypes',
 'd8', 'd8_dev', 'depression_table', 'depression_table_dev', 'depression_table_of', 'depressions',
 'depressions_args', 'depressions_dev', 'device_count', 'elementwise_dev',
 'elementwise_work_type', 'expand', 'expand_dev', 'fft2', 'fft2_dev', 'flowacc', 'flowacc_dev',
 'flowtrace', 'flowtrace_args', 'flowtrace_dev', 'fourier_destripe', 'fourier_destripe_dev',
 'grey_dilation_dev', 'groves', 'groves_dev', 'host_empty', 'importlib', 'is_device_raster',
 'isolated_points', 'isolated_points_dev', 'lagoons_detection_dev', 'load_library',
 'logical_type', 'majority_dev', 'mask_bytes', 'np', 'on_device', 'os', 'quadratic',
 'quadratic_dev', 'resolve_flats', 'resolve_flats_args', 'resolve_flats_dev', 'result_raster',
 'sinkfill', 'sinkfill_d8_dev', 'sinkfill_dev', 'sys', 'threading', 'tidying_lagoons_dev',
 'watershed', 'watershed_dev', 'weakref', 'widened_to_host']
# ---- end of the recorded tables


@pytest.mark.parametrize("name,call", CALLS, ids=CALL_IDS)
def test_a_form_makes_the_recorded_c_calls(name, call):
    ops, sizes = recorded(call)
    want_ops, want_sizes = EXPECTED_CALLS[name]
    assert ops == want_ops
    assert sizes == want_sizes


@pytest.mark.parametrize("name,call", REFUSALS, ids=REFUSAL_IDS)
def test_a_bad_call_is_refused_in_the_recorded_words_without_a_device(name, call, monkeypatch):
    assert refused(call, monkeypatch) == EXPECTED_REFUSALS[name]


def test_the_public_names_of_the_backend():
    assert sorted(backend.__all__) == NAMES
