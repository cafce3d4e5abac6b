"""
The proximity kernels (``hdem_proximity[_dev]``, ``EuclideanDistance``, ``EuclideanAllocation``,
``BurnStreams``) on the MI355X against the references of tests/test_proximity.py.

Shapes: strips and tiny rasters, one exact tile of ``PX_TILE`` = 64 cells and one cell past it
both ways, several tiles with partial last ones, and one cell past every other boundary inside
hdem_proximity.hip: (2, 257) is one column past the four 64-column chunks a workgroup of the
bits kernel takes; (257, 2) one row past the ``NT`` = 256 rows of a workgroup of the carry
kernel and past the 256 nodes from which a thread of the column kernel owns a node; (700, 3) has
levels with more nodes than the workgroup has threads; (16384, 2) is the longest column kept in
LDS (``PX_LDS_LINE`` = 16384 rows) and (16385, 2) the first that the column kernel reads from
global memory; (2, 16385) has 257 chunks to carry a source column across.

Bars: ``d2``, ``nearest`` and ``label`` equal the reference (``brute`` where cells x sources
allows it, ``separable`` otherwise); ``distance``, ``rise`` and ``burned`` are the bits of the
NumPy formulas, a NaN being a NaN whatever its sign and payload.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend as B
from hydrodem_amd import proximity as P
from hydrodem_amd.backend import DeviceRaster
from oracle import c_oracle
from test_gpu_scribble import POISON, Case, assert_same_bytes, execute
from test_proximity import (UNREACHED, brute, burned_of, checkerboard, full_column, full_row,
                            mirrored_pair, random_sources, reference, separable)

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (64, 64), (65, 63), (130, 197), (3, 700), (700, 3),
          (2, 257), (257, 2)]
LONG = [(16384, 2), (16385, 2), (2, 16385)]
CELL, BUFFER, SMOOTH, SHARP = 30.0, 6.5, 5.0, 2.0
ALL = tuple(n for n, _ in P.PROXIMITY_OUTPUTS)
TYPES = dict(P.PROXIMITY_OUTPUTS)
BRUTE_LIMIT = 1 << 26                                    # cells x sources


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


# ---------------------------------------------------------------------------
# inputs and their reference, made once
# ---------------------------------------------------------------------------
def corner(k):
    def layout(shape):
        s = np.zeros(shape, bool)
        s[-(k // 2), -(k % 2)] = True                    # (0, 0), (0, -1), (-1, 0), (-1, -1)
        return s
    return layout


def centre(shape):
    s = np.zeros(shape, bool)
    s[shape[0] // 2, shape[1] // 2] = True
    return s


LAYOUTS = {"none": lambda shape: np.zeros(shape, bool), "all": lambda shape: np.ones(shape, bool),
           "corner0": corner(0), "corner1": corner(1), "corner2": corner(2), "corner3": corner(3),
           "centre": centre,
           "random0.001": lambda shape: random_sources(shape, 0.001),
           "random0.05": lambda shape: random_sources(shape, 0.05),
           "random0.5": lambda shape: random_sources(shape, 0.5),
           "row": full_row, "column": full_column, "checkerboard": checkerboard,
           "mirrored": mirrored_pair}
SPARSE = ("none", "corner0", "corner1", "corner2", "corner3", "centre", "random0.001",
          "random0.05", "mirrored")
CASES = [(shape, name) for shape in SHAPES for name in LAYOUTS] + \
        [(shape, name) for shape in LONG for name in SPARSE]
IDS = [f"{s[0]}x{s[1]}-{name}" for s, name in CASES]


@functools.lru_cache(maxsize=None)
def inputs(shape, layout):
    h, w = shape
    s = LAYOUTS[layout](shape)
    dem = hdem_synth.synth_dem(h, w).copy()
    if h * w >= 9:
        dem.ravel()[[0, h * w // 2, h * w - 2]] = np.nan
    flat = np.arange(h * w, dtype=np.uint32).reshape(shape)
    labels = np.where(s, flat % np.uint32(1000) + np.uint32(1), np.uint32(0)).astype(np.uint32)
    for a in (s, dem, labels):
        a.setflags(write=False)
    return {"sources": s, "mask": s.view(np.uint8), "labels": labels, "dem": dem}


def how_for(sources):
    return brute if sources.size * max(1, int(sources.sum())) <= BRUTE_LIMIT else separable


@functools.lru_cache(maxsize=None)
def expected(shape, layout, max_distance=None):
    inp = inputs(shape, layout)
    return reference(inp["sources"], max_distance, inp["dem"], inp["labels"], CELL, BUFFER,
                     SMOOTH, SHARP, how_for(inp["sources"]))


def run_dev(inp, want=ALL, kind="labels", threshold=None, max_distance=None, ctx=None, out=None):
    """One device call on host inputs: ``{name: host array}`` and the stats."""
    ctx = ctx or B.context()
    with contextlib.ExitStack() as stack:
        def up(a):
            return stack.enter_context(DeviceRaster.from_host(a, dtype=a.dtype, ctx=ctx))
        needs_dem = "rise" in want or "burned" in want
        outs, stats = P.proximity_dev(up(inp[kind]), threshold, want,
                                      up(inp["dem"]) if needs_dem else None, CELL, max_distance,
                                      BUFFER, SMOOTH, SHARP, out=out)
        for raster in outs.values():
            if out is None or not any(raster is r for r in out.values()):
                stack.enter_context(raster)
        return {name: raster.to_host() for name, raster in outs.items()}, stats


@functools.lru_cache(maxsize=None)
def device(shape, layout, max_distance=None):
    return run_dev(inputs(shape, layout), max_distance=max_distance)


def assert_matches(got, ref, what):
    """Integers equal; floats bit-equal where the reference is a number, NaN where it is NaN."""
    for name, want in ref.items():
        if name not in got:
            continue
        g = got[name]
        assert (g.dtype, g.shape) == (want.dtype, want.shape), f"{what}: {name}"
        if want.dtype.kind == "f":
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(g), nan), f"{what}: {name} NaN cells"
            g, want = g.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
        if not np.array_equal(g, want):
            bad = np.flatnonzero(g.ravel() != want.ravel())
            raise AssertionError(f"{what}: {name} differs in {bad.size} cells, the first at "
                                 f"{bad[0]}: {g.ravel()[bad[0]]} for {want.ravel()[bad[0]]}")


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_every_output_against_the_reference(shape, layout):
    ref = expected(shape, layout)
    got, stats = device(shape, layout)
    assert set(got) == set(ALL)
    assert_matches(got, ref, f"{shape} {layout}")
    assert stats["sources"] == int(inputs(shape, layout)["sources"].sum())
    assert stats["unreached"] == int((ref["d2"] == UNREACHED).sum())


@pytest.mark.parametrize("gap", [63, 64, 65, 300])
def test_a_step_of_the_argmin_gives_deep_nodes_a_long_range(gap):
    """Two sources ``gap`` rows apart in a column of 700: at the levels where a thread owns a
    node, the nodes that straddle the step of the argmin search ``gap + 1`` rows, as long as a
    wave and longer, while their neighbours search one."""
    s = np.zeros((700, 3), bool)
    s[300, 1] = s[300 + gap, 2] = True
    dem = hdem_synth.synth_dem(700, 3)
    inp = {"sources": s, "labels": s.astype(np.uint32) * np.uint32(9), "dem": dem}
    got, _ = run_dev(inp)
    assert_matches(got, reference(s, None, dem, inp["labels"], CELL, BUFFER, SMOOTH, SHARP),
                   f"gap {gap}")


@pytest.mark.parametrize("max_distance", [1, 5, 100000])
@pytest.mark.parametrize("shape,layout", [((65, 63), "random0.05"), ((130, 197), "mirrored"),
                                          ((130, 197), "random0.001"), ((3, 700), "corner3"),
                                          ((16385, 2), "centre")], ids=str)
def test_max_distance_puts_cells_out_of_reach(shape, layout, max_distance):
    ref = expected(shape, layout, max_distance)
    got, stats = device(shape, layout, max_distance)
    assert_matches(got, ref, f"{shape} {layout} within {max_distance}")
    assert stats["unreached"] == int((ref["d2"] == UNREACHED).sum())
    if max_distance < 100:
        assert 0 < stats["unreached"] < ref["d2"].size
    else:
        assert_same_bytes(got, device(shape, layout)[0], "a bound larger than the raster")


# ---------------------------------------------------------------------------
# the real chain: fill -> D8 -> accumulation >= 10, as a mask, an accumulation and labels
# ---------------------------------------------------------------------------
THRESHOLD = 10


@functools.lru_cache(maxsize=None)
def chain_inputs(shape=(130, 197)):
    z = hdem_synth.synth_dem(*shape)
    codes = hd.HydroConditioning(epsilon=1e-3).apply(z)
    acc = hd.FlowAccumulation().apply(codes)
    basins = hd.Watersheds(labels="compact").apply(codes)
    s = acc >= THRESHOLD
    inp = {"sources": s, "mask": s.view(np.uint8), "acc": acc,
           "labels": np.where(s, basins, 0).astype(np.uint32), "dem": z}
    for a in inp.values():
        a.setflags(write=False)
    return inp


def test_streams_as_a_mask_an_accumulation_and_labels():
    inp = chain_inputs()
    assert 100 < inp["sources"].sum() < inp["sources"].size // 2
    ref = reference(inp["sources"], None, inp["dem"], inp["labels"], CELL, BUFFER, SMOOTH, SHARP,
                    separable)
    by_labels, stats = run_dev(inp)
    assert_matches(by_labels, ref, "streams as labels")
    assert stats["sources"] == int(inp["sources"].sum()) and stats["unreached"] == 0
    rest = tuple(n for n in ALL if n != "label")
    by_mask, _ = run_dev(inp, rest, "mask")
    by_acc, _ = run_dev(inp, rest, "acc", THRESHOLD)
    want = {n: by_labels[n] for n in rest}
    assert_same_bytes(by_mask, want, "streams as a mask")
    assert_same_bytes(by_acc, want, "streams as an accumulation")
    # a bool mask on the host side, and the filters
    host, _ = P.proximity(inp["sources"], want=("d2", "distance"), cellsize=CELL)
    assert_same_bytes(host, {n: by_labels[n] for n in host}, "a bool mask")
    distance = hd.EuclideanDistance(threshold=THRESHOLD, cellsize=CELL)
    assert_same_bytes({"distance": distance.apply(inp["acc"])}, {"distance": ref["distance"]},
                      "EuclideanDistance")
    assert distance.stats["sources"] == stats["sources"]
    assert np.array_equal(hd.EuclideanAllocation().apply(inp["labels"]), ref["label"])
    assert np.array_equal(hd.EuclideanAllocation().apply(inp["sources"]), ref["nearest"])
    given = hd.EuclideanAllocation(inp["acc"], threshold=THRESHOLD, max_distance=3)
    near3 = reference(inp["sources"], 3, how=separable)["nearest"]
    assert np.array_equal(given.apply(inp["dem"]), near3)
    with DeviceRaster.from_host(inp["labels"]) as labels, \
            hd.EuclideanAllocation().apply_device(labels) as got:
        assert np.array_equal(got.to_host(), ref["label"])


# ---------------------------------------------------------------------------
# host and device forms, out=, subsets, repeats
# ---------------------------------------------------------------------------
FORMS = [((1, 9), "centre"), ((65, 63), "random0.05"), ((130, 197), "checkerboard"),
         ((16385, 2), "random0.001")]


@pytest.mark.parametrize("shape,layout", FORMS, ids=str)
def test_the_host_form_returns_the_bytes_of_the_device_form(shape, layout):
    inp = inputs(shape, layout)
    want, want_stats = device(shape, layout)
    got, stats = P.proximity(inp["labels"], None, ALL, inp["dem"], CELL, None, BUFFER, SMOOTH,
                             SHARP)
    assert_same_bytes(got, want, f"host form {shape} {layout}")
    counts = lambda st: {k: v for k, v in st.items() if not k.startswith("ms_")}  # noqa: E731
    assert counts(stats) == counts(want_stats)


@pytest.mark.parametrize("shape,layout", FORMS[1:3], ids=str)
def test_out_rasters_are_written_in_place(shape, layout):
    want, _ = device(shape, layout)
    ctx = B.context()
    with contextlib.ExitStack() as stack:
        out = {n: stack.enter_context(DeviceRaster.empty(shape, TYPES[n], ctx))
               for n in ("nearest", "burned")}
        for raster in out.values():
            ctx.check(ctx.lib.hdem_memset_dev(ctx.handle, raster.ptr, 0x5A, raster.nbytes))
        inp = inputs(shape, layout)
        with DeviceRaster.from_host(inp["labels"]) as src, DeviceRaster.from_host(inp["dem"]) as dem:
            outs, _ = P.proximity_dev(src, None, ("d2", "nearest", "burned"), dem, CELL, None,
                                      BUFFER, SMOOTH, SHARP, out=out)
        assert outs["nearest"] is out["nearest"] and outs["burned"] is out["burned"]
        with outs["d2"] as fresh:
            got = {"d2": fresh.to_host(), "nearest": out["nearest"].to_host(),
                   "burned": out["burned"].to_host()}
        with pytest.raises(ValueError, match="not wanted"):
            P.proximity_dev(out["nearest"], None, ("d2",), out={"nearest": out["nearest"]})
    assert_same_bytes(got, {n: want[n] for n in got}, f"out= {shape} {layout}")


# the final kernel branches on every output pointer by itself
SUBSETS = [(name,) for name in ALL] + [("d2", "nearest"), ("label", "rise"),
                                       ("distance", "burned"), ("nearest", "distance", "rise")]


@pytest.mark.parametrize("want", SUBSETS, ids="+".join)
def test_a_subset_returns_the_bytes_of_the_call_for_all(want):
    for shape, layout in (((65, 63), "random0.05"), ((130, 197), "mirrored")):
        whole, _ = device(shape, layout)
        got, _ = run_dev(inputs(shape, layout), want)
        assert_same_bytes(got, {name: whole[name] for name in want}, f"{want} {shape}")


@pytest.mark.parametrize("shape,layout", FORMS + [((700, 3), "random0.5")], ids=str)
def test_three_calls_return_the_same_bytes(shape, layout):
    want, want_stats = device(shape, layout)
    for k in range(3):
        got, stats = run_dev(inputs(shape, layout))
        assert_same_bytes(got, want, f"call {k} {shape} {layout}")
        assert stats["sources"] == want_stats["sources"]
        assert stats["unreached"] == want_stats["unreached"]


# ---------------------------------------------------------------------------
# refusals of the library
# ---------------------------------------------------------------------------
def test_the_library_refuses_before_any_launch():
    ctx = B.context()
    mask = np.ones((4, 4), np.uint8)
    acc = np.ones((4, 4), np.uint32)
    z = np.zeros((4, 4), F32)
    u32, f32 = np.empty((4, 4), np.uint32), np.empty((4, 4), F32)
    null = ctypes.c_void_p()
    ptr = lambda a: null if a is None else a.ctypes.data  # noqa: E731

    def call(src=mask, kind=P.SOURCES_MASK_U8, threshold=0, shape=(4, 4), dem=None, cell=1.0,
             reach=0, buffer=2.0, smooth=1.0, sharp=0.0, outs=(None,) * 6):
        rc = ctx.lib.hdem_proximity(ctx.handle, ptr(src), kind, threshold, *shape, ptr(dem), cell,
                                    reach, buffer, smooth, sharp, *[ptr(o) for o in outs], None)
        if rc != B.OK:
            assert rc == B.BAD_ARG and ctx.lib.hdem_last_error()
        return rc
    only = lambda k, o: tuple(o if j == k else None for j in range(6))  # noqa: E731
    assert call(outs=only(0, u32)) == B.OK
    assert call(outs=only(5, f32), dem=z) == B.OK
    assert call() == B.BAD_ARG                                           # no output
    assert call(src=None, outs=only(0, u32)) == B.BAD_ARG                # no sources
    assert call(kind=0, outs=only(0, u32)) == B.BAD_ARG                  # "every cell" is no kind
    assert call(kind=4, outs=only(0, u32)) == B.BAD_ARG
    assert call(threshold=3, outs=only(0, u32)) == B.BAD_ARG             # a mask with a threshold
    assert call(src=acc, kind=P.SOURCES_ACC_U32, outs=only(0, u32)) == B.BAD_ARG   # threshold 0
    assert call(src=acc, kind=P.SOURCES_LABELS_U32, threshold=1, outs=only(0, u32)) == B.BAD_ARG
    assert call(outs=only(2, u32)) == B.BAD_ARG                          # label without labels
    assert call(src=acc, kind=P.SOURCES_ACC_U32, threshold=1, outs=only(2, u32)) == B.BAD_ARG
    assert call(src=acc, kind=P.SOURCES_LABELS_U32, outs=only(2, u32)) == B.OK
    assert call(outs=only(4, f32)) == B.BAD_ARG                          # rise without dem
    assert call(outs=only(5, f32)) == B.BAD_ARG                          # burned without dem
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(outs=only(3, f32), cell=bad) == B.BAD_ARG
        assert call(outs=only(5, f32), dem=z, buffer=bad) == B.BAD_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(outs=only(5, f32), dem=z, smooth=bad) == B.BAD_ARG
        assert call(outs=only(5, f32), dem=z, sharp=bad) == B.BAD_ARG
    assert call(outs=only(4, z), dem=z) == B.BAD_ARG                     # an output over the dem
    assert call(src=acc, kind=P.SOURCES_LABELS_U32, outs=only(0, acc)) == B.BAD_ARG
    assert call(outs=(u32, u32) + (None,) * 4) == B.BAD_ARG              # two outputs, one place
    # the size limits: nothing is allocated, nothing is read
    for shape in ((1, 65537), (65537, 1), (1, 65536), (65536, 1), (65535, 65535), (3, 1 << 30)):
        assert call(shape=shape, outs=only(0, u32)) == B.BAD_ARG, shape
    assert b"2^32 - 2" in ctx.lib.hdem_last_error() or b"cells" in ctx.lib.hdem_last_error()
    with pytest.raises(ValueError, match="squared diagonal"):
        P.proximity(np.zeros((1, 65537), np.uint8))


# ---------------------------------------------------------------------------
# stream burning in front of the fill
# ---------------------------------------------------------------------------
def test_burn_fill_and_d8_as_one_device_chain():
    inp = chain_inputs()
    z, acc = inp["dem"], inp["acc"]
    streams = inp["sources"]
    burn = hd.BurnStreams(acc, threshold=THRESHOLD, buffer=4, smooth=3.0, sharp=1.5)
    want_burned = burned_of(z, separable(streams)[0], 4, 3.0, 1.5)
    want_filled = c_oracle.sinkfill_pflood(want_burned, eps=1e-3)
    chain, front = hd.ComposedFilter(), hd.ComposedFilter()
    front.filters = [burn, hd.SinkFill(epsilon=1e-3)]
    chain.filters = front.filters + [hd.D8FlowDirection()]
    with DeviceRaster.from_host(z) as zd:
        with burn.apply_device(zd) as burned:
            assert_matches({"burned": burned.to_host()}, {"burned": want_burned}, "BurnStreams")
        with front.apply_device(zd) as filled:
            assert np.array_equal(filled.to_host(), want_filled)
        with chain.apply_device(zd) as codes:
            assert codes.dtype == np.uint8
            assert np.array_equal(codes.to_host(), c_oracle.d8(want_filled))
    assert np.array_equal(chain.apply(z), c_oracle.d8(want_filled))       # the same on the host
    assert_matches({"burned": burn.apply(z)}, {"burned": want_burned}, "BurnStreams.apply")
    assert streams.sum() > 100 and (want_burned[streams] < z[streams]).all()
    assert burn.stats["sources"] == int(streams.sum())


# ---------------------------------------------------------------------------
# poison: the method of tests/test_gpu_scribble.py
# ---------------------------------------------------------------------------
def poison_case(name, want, shape, layout):
    def run(call, inp):
        src, dem = call.up(inp["labels"]), call.up(inp["dem"])
        out = {n: call.out(src.shape, TYPES[n]) for n in want} if call.own else None
        outs, stats = P.proximity_dev(src, None, want, dem, CELL, None, BUFFER, SMOOTH, SHARP,
                                      out=out)
        return {n: (r.to_host() if call.own else call.host(r)) for n, r in outs.items()}, stats
    return Case(name, ((shape, layout),), None, run, None, True, frozenset())


POISON_CASES = [poison_case("proximity-all", ALL, (130, 197), "random0.05"),
                poison_case("proximity-d2", ("d2",), (65, 63), "checkerboard"),
                poison_case("proximity-global-line", ("nearest", "burned"), (16385, 2),
                            "random0.001")]
_BASELINE = {}


def poison_baseline(entry):
    if entry.name not in _BASELINE:
        _BASELINE[entry.name] = execute(entry, inputs(*entry.shapes[0]), None, False)
    return _BASELINE[entry.name]


@pytest.mark.parametrize("byte", POISON, ids=lambda b: f"poison{b:02X}")
@pytest.mark.parametrize("entry", POISON_CASES, ids=lambda e: e.name)
def test_poisoned_workspace_and_outputs_change_no_byte(entry, byte):
    shape, layout = entry.shapes[0]
    want, want_stats = poison_baseline(entry)
    whole, _ = device(shape, layout)
    assert_same_bytes(want, {n: whole[n] for n in want}, f"{entry.name} without poison")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} under 0x{byte:02X}, out= {whose}"
        got, stats = execute(entry, inputs(shape, layout), byte, own)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
