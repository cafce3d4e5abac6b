"""
Every device operator on poisoned scratch and output memory (``hdem_set_scribble``,
``Context.scribble``).

The other GPU tests hold each operator to a CPU reference, but none of them controls what the
operator's workspace holds when the call begins: the arena of the multi-kernel chains is kept
between calls, ``hdem_malloc`` hands back cached blocks with their last owner's bytes, and a
fresh ``hipMalloc`` is usually zero pages.  An operator that reads what it never wrote passes
as long as the leftovers happen to be harmless.  Here every device entry point of
``backend.py`` runs on a fresh context with that memory filled with 0x00, 0xFF (NaN, -1, the
flats' "infinite"), 0x7F (the sink fill's "unset", a huge finite float) and 0x01 (the D8 code
E, a small index, a set mask byte), with ``out=`` left to the library and with a caller's
``out=`` raster under the same poison, and must return the bytes of the run without poison
(R0), which is held to the operator's CPU reference under the bar its own test module uses.

Stats are compared too, without the ``ms_*`` times and without the counters that depend on
the order in which workgroups happen to run, whatever the workspace holds (``Case.schedule``,
each with its reason); they are not results.

Then the hook itself, the host-pointer entry points and the composed chains under 0xFF on the
default context, and two sequences without the hook, shrinking and growing on one context,
for the buffers the hook leaves alone on reuse (the sink fill's workspace and hub buffers) and
for the arena.

Run with ``-k poison00`` first where a fault would cost more than a failed test: a scribbled
index that a kernel really reads is an address the kernel follows.
"""
import collections
import contextlib

import numpy as np
import pytest
from scipy import fftpack, ndimage

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend as B
from hydrodem_amd import streamorder as SO
from hydrodem_amd import upstream as UP
from hydrodem_amd.backend import DeviceRaster
from oracle import c_oracle, hdem_oracle_np
from oracle import hdem_oracle_fourier as OF
from oracle import hdem_oracle_lagoons as OL
from test_depressions import first_labels
from test_depressions import reference as depressions_reference
from test_elementwise_cases import same as same_as_numpy
from test_flats import random_flats, resolve_flats_bfs
from test_flowacc import acc_kahn, random_acyclic_codes, terminal_mask
from test_flowtrace import distance_of, hand_of, trace_walk
from test_gpu_f64 import FFT_RTOL as FFT64_RTOL
from test_gpu_f64 import IFFT_RTOL as IFFT64_RTOL
from test_gpu_fourier import FFT_RTOL
from test_gpu_fourier import TOL as FOURIER_TOL
from test_gpu_parity import TOL, _groves_compare, _groves_excused_limit
from test_streamorder import link_ends, order_kahn, stream_of
from test_upstream import length_of, upstream_kahn
from test_watersheds import labels_walk, random_seeds

pytestmark = pytest.mark.gpu

POISON = (0x00, 0xFF, 0x7F, 0x01)
SEED = 5
THRESHOLD = 10                  # stream where the accumulation reaches it
CELL = 30.0

# 64 x 64 tiles: 3 x 4 with a partial last row and column of tiles (2 and 5 cells), one exact
# tile, two strips
D8_SHAPES = [(130, 197), (64, 64), (1, 200), (65, 1)]
# 62 x 62 tiles over the interior: one tile of one cell, 2 x 4 and 4 x 6 tiles with a partial
# last row and column; beyond the issue's sizes (519, 508), 81 tiles, where the fill takes its
# hub start, whose buffers the library allocates for itself
FILL_SHAPES = [(3, 3), (126, 190), (200, 333), (519, 508)]
WINDOW_SHAPES = [(64, 33), (131, 157)]
FOURIER_SHAPES = [(141, 155), (150, 168), (256, 256)]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


# ---------------------------------------------------------------------------
# one call on one context
# ---------------------------------------------------------------------------
class Call:
    """The device rasters of one call: uploaded operands, the caller's ``out=`` rasters when
    the call is made with them (``own``), results to download; all freed with ``stack``."""

    def __init__(self, ctx, own):
        self.ctx, self.own, self.stack = ctx, own, contextlib.ExitStack()

    def up(self, array):
        return self.stack.enter_context(
            DeviceRaster.from_host(array, dtype=array.dtype, ctx=self.ctx))

    def empty(self, shape, dtype):
        return self.stack.enter_context(DeviceRaster.empty(shape, dtype, self.ctx))

    def out(self, shape, dtype):
        return self.empty(shape, dtype) if self.own else None

    def host(self, raster):
        self.stack.callback(raster.free)
        return raster.to_host()


Case = collections.namedtuple("Case", "name shapes build run check own schedule")
CASES = []


def case(name, shapes, build, check, own=True, schedule=()):
    """Register ``run(call, inputs) -> ({name: host array}, stats or None)``.  ``own``: the
    entry point takes ``out=``.  ``schedule``: stats that depend on the order of execution."""
    def register(run):
        CASES.append(Case(name, tuple(shapes), build, run, check, own, frozenset(schedule)))
        return run
    return register


def execute(entry, inputs, byte, own):
    """``entry.run`` on a fresh context, under ``byte`` when it is not ``None``."""
    ctx = B.Context()
    try:
        with contextlib.ExitStack() as stack:
            if byte is not None:
                stack.enter_context(ctx.scribble(byte))
            call = Call(ctx, own)
            stack.enter_context(call.stack)          # (freed before the mode goes off)
            arrays, stats = entry.run(call, inputs)
            ctx.synchronize()
        return ({k: np.ascontiguousarray(v) for k, v in arrays.items()},
                counters(stats, entry.schedule))
    except B.BackendError as exc:
        # a HIP call failed: a kernel may have followed a poisoned index, and whatever runs on
        # this device afterwards proves nothing
        pytest.exit(f"a HIP call failed in {entry.name} under {byte!r}: {exc}", returncode=3)
    finally:
        ctx.close()


def counters(stats, schedule=()):
    if stats is None:
        return None
    return {k: v for k, v in stats.items() if not k.startswith("ms_") and k not in schedule}


def assert_same_bytes(got, want, what):
    assert got.keys() == want.keys(), what
    for name, w in want.items():
        g = got[name]
        assert (g.dtype, g.shape) == (w.dtype, w.shape), f"{what}: {name}"
        gb, wb = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
        if not np.array_equal(gb, wb):
            cells = np.flatnonzero((gb != wb).reshape(g.size, -1).any(axis=1))
            first = np.unravel_index(cells[0], g.shape) if g.ndim else ()
            raise AssertionError(
                f"{what}: {name} differs in {cells.size} of {g.size} cells, the first at "
                f"{first}: {g.reshape(-1)[cells[0]]!r} for {w.reshape(-1)[cells[0]]!r}")


def equal(got, want):
    """Values and shape; NaN equal to NaN in the float rasters."""
    return np.array_equal(got, want, equal_nan=np.asarray(got).dtype.kind in "fc")


# ---------------------------------------------------------------------------
# the tiled D8 operators
# ---------------------------------------------------------------------------
def codes_of(shape, seed):
    codes = random_acyclic_codes(*shape, seed, ramp=True)
    acc = acc_kahn(codes).astype(np.uint32)
    rng = np.random.default_rng([seed, *shape])
    return {"codes": codes, "acc": acc, "mask": (acc >= THRESHOLD).astype(np.uint8),
            "dem": rng.random(shape, dtype=np.float32) * np.float32(100.0),
            "seeds": random_seeds(shape, seed)}


def check_flowacc(inp, got):
    assert got["acc"].dtype == np.uint32 and equal(got["acc"], inp["acc"])


# max_hops: the walk that goes on at a node is the one whose atomic arrives last
@case("flowacc", D8_SHAPES, codes_of, check_flowacc, schedule=("max_hops",))
def _(call, inp):
    out, stats = B.flowacc_dev(call.up(inp["codes"]), out=call.out(inp["codes"].shape, np.uint32))
    return {"acc": call.host(out)}, stats


def check_outlets(inp, got):
    assert equal(got["labels"], labels_walk(inp["codes"]))


def check_pour(inp, got):
    assert equal(got["labels"], labels_walk(inp["codes"], inp["seeds"]))


def check_compact(inp, got):
    labels, outlets = got["labels"], got["outlets"]
    assert outlets.size == int(terminal_mask(inp["codes"]).sum()) == np.unique(outlets).size
    assert labels.min() >= 1 and labels.max() == outlets.size
    assert equal(outlets[labels.ravel().astype(np.int64) - 1].astype(np.int64) + 1,
                 labels_walk(inp["codes"]).ravel())


# forest_rounds: the watershed forest jumps in place, a racing reader may see an ancestor
def watershed_case(name, check, **kw):
    @case(name, D8_SHAPES, codes_of, check, schedule=("forest_rounds",))
    def _(call, inp):
        seeds = call.up(inp["seeds"]) if kw.get("seeds") else None
        out, outlets, stats = B.watershed_dev(call.up(inp["codes"]), seeds, kw.get("compact", False),
                                              out=call.out(inp["codes"].shape, np.uint32))
        got = {"labels": call.host(out)}
        if outlets is not None:
            got["outlets"] = outlets
        return got, stats


watershed_case("watershed-outlet", check_outlets)
watershed_case("watershed-compact", check_compact, compact=True)
watershed_case("watershed-pour", check_pour, seeds=True)


def trace_case(name, streams, want, dem=False):
    def check(inp, got):
        s = None if streams is None else inp["mask"] if streams == "mask" else inp["acc"] >= THRESHOLD
        stop, nc, nd = trace_walk(inp["codes"], s)
        ref = {"stop": stop, "ncard": nc, "ndiag": nd, "distance": distance_of(stop, nc, nd, CELL),
               "hand": hand_of(stop, inp["dem"])}
        assert set(got) == set(want)
        for k in got:
            assert got[k].dtype == ref[k].dtype and equal(got[k], ref[k]), k

    @case(name, D8_SHAPES, codes_of, check, own=False)
    def _(call, inp):
        s = None if streams is None else call.up(inp[streams])
        outs, stats = B.flowtrace_dev(call.up(inp["codes"]), s,
                                      THRESHOLD if streams == "acc" else None,
                                      call.up(inp["dem"]) if dem else None, CELL, want)
        return {k: call.host(r) for k, r in outs.items()}, stats


trace_case("flowtrace-outlet", None, ("distance",))
trace_case("flowtrace-mask", "mask", ("stop", "distance"))
trace_case("flowtrace-acc", "acc", ("ncard", "ndiag", "distance"))
trace_case("flowtrace-hand", "acc", ("stop", "ncard", "ndiag", "distance", "hand"), dem=True)


def check_upstream(inp, got):
    nc, nd = upstream_kahn(inp["codes"])
    assert equal(got["ncard"], nc) and equal(got["ndiag"], nd)
    assert got["length"].dtype == np.float32 and equal(got["length"], length_of(nc, nd, CELL))


@case("upstream", D8_SHAPES, codes_of, check_upstream, own=False, schedule=("max_hops",))
def _(call, inp):
    outs, stats = UP.upstream_dev(call.up(inp["codes"]), CELL, ("ncard", "ndiag", "length"))
    return {k: call.host(r) for k, r in outs.items()}, stats


def order_case(name, streams, want):
    def check(inp, got):
        s = stream_of(inp["codes"], None if streams is None else inp[streams],
                      THRESHOLD if streams == "acc" else None)
        order, magnitude = order_kahn(inp["codes"], s)
        ref = {"order": order, "magnitude": magnitude, "link": link_ends(inp["codes"], s)}
        assert set(got) == set(want)
        for k in got:
            assert equal(got[k], ref[k]), k

    # with "link" the first stops live in the caller's raster, without it behind the flow
    # trace's bytes in the arena
    @case(name, D8_SHAPES, codes_of, check, own=False, schedule=("max_hops",))
    def _(call, inp):
        s = None if streams is None else call.up(inp[streams])
        outs, stats = SO.streamorder_dev(call.up(inp["codes"]), s,
                                         THRESHOLD if streams == "acc" else None, want)
        return {k: call.host(r) for k, r in outs.items()}, stats


order_case("streamorder-all", None, ("order", "magnitude", "link"))
order_case("streamorder-mask", "mask", ("order", "magnitude"))
order_case("streamorder-acc", "acc", ("order", "magnitude", "link"))
order_case("streamorder-acc-nolink", "acc", ("order",))


def flats_of(shape, seed):
    dem, codes = random_flats(shape, seed)
    return {"dem": dem, "codes": codes}


def check_flats(inp, got):
    out, dist = resolve_flats_bfs(inp["dem"], inp["codes"])
    assert equal(got["codes"], out) and equal(got["dist"], dist)


# rounds, tile_visits: a tile reads the halo its neighbours write in the same launch
@case("resolve_flats", D8_SHAPES, flats_of, check_flats, schedule=("rounds", "tile_visits"))
def _(call, inp):
    out, dist, stats = B.resolve_flats_dev(call.up(inp["codes"]), call.up(inp["dem"]), True,
                                           out=call.out(inp["codes"].shape, np.uint8))
    return {"codes": call.host(out), "dist": call.host(dist)}, stats


def filled_of(shape, seed):
    dem = hdem_synth.synth_dem(*shape, variant="rough")
    return {"dem": dem, "filled": c_oracle.sinkfill_pflood(dem)}


def check_depressions(inp, got):
    lab, count, table = depressions_reference(inp["dem"], inp["filled"], CELL)
    assert got["labels"].dtype == np.uint32 and equal(got["labels"], lab)
    for k, column in table.items():
        assert got[k].dtype == column.dtype and equal(got[k], column), k
    assert got["first"].size == count


def check_depressions_first(inp, got):
    lab, _, table = depressions_reference(inp["dem"], inp["filled"])
    assert equal(got["labels"], first_labels(lab, table["first"]))


@case("depressions-compact-table", D8_SHAPES, filled_of, check_depressions)
def _(call, inp):
    dem, filled = call.up(inp["dem"]), call.up(inp["filled"])
    labels, stats = B.depressions_dev(dem, filled, True, out=call.out(inp["dem"].shape, np.uint32))
    table = B.depression_table_dev(dem, filled, labels, stats["depressions"], CELL)
    return dict(table, labels=call.host(labels)), stats


@case("depressions-first", D8_SHAPES, filled_of, check_depressions_first)
def _(call, inp):
    labels, stats = B.depressions_dev(call.up(inp["dem"]), call.up(inp["filled"]), False,
                                      out=call.out(inp["dem"].shape, np.uint32))
    return {"labels": call.host(labels)}, stats


# ---------------------------------------------------------------------------
# sink fill, D8, coarsening
# ---------------------------------------------------------------------------
# The asynchronous phase takes tiles off a worklist in the order the workgroups get to them:
# how often a tile (a flat one too) is visited, found unchanged or queued again, and how many
# sweeps the visits make, is the schedule's -- two runs of one fill on fresh contexts without
# any poison differ in them -- and whether the whole launch was resident at once depends on
# what else the device runs.  What the fill converged to, in how many certifying rounds, what
# it left pending and the tile grid are compared.
FILL_SCHEDULE = ("tile_visits", "iterations", "visits_unchanged", "visits_requeued",
                 "visits_flat", "flat_unchanged", "partial_residency")


def dem_of(nodata):
    def build(shape, seed):
        z = hdem_synth.synth_dem(*shape)
        if nodata:
            z[shape[0] // 2, shape[1] // 2] = np.nan
            if shape[1] > 60:
                z[shape[0] // 3:shape[0] // 3 + 4, 30:50] = np.nan
        return {"z": z}
    return build


def fill_case(name, eps, nodata, d8=False):
    def check(inp, got):
        want = c_oracle.sinkfill_pflood(inp["z"], eps=eps)
        assert got["filled"].dtype == np.float32 and equal(got["filled"], want)
        assert equal(np.isnan(got["filled"]), np.isnan(inp["z"]))
        if d8:
            assert equal(got["codes"], c_oracle.d8(want))

    @case(name, FILL_SHAPES, dem_of(nodata), check, schedule=FILL_SCHEDULE)
    def _(call, inp):
        z = call.up(inp["z"])
        if not d8:
            out, stats = B.sinkfill_dev(z, eps, out=call.out(z.shape, np.float32))
            return {"filled": call.host(out)}, stats
        out, codes, stats = B.sinkfill_d8_dev(z, eps, out=call.out(z.shape, np.float32),
                                              codes=call.out(z.shape, np.uint8))
        return {"filled": call.host(out), "codes": call.host(codes)}, stats


for _nodata in (False, True):
    _tag = "-nodata" if _nodata else ""
    fill_case("sinkfill" + _tag, 0.0, _nodata)
    fill_case("sinkfill-eps" + _tag, 1e-3, _nodata)
    fill_case("sinkfill_d8" + _tag, 0.0, _nodata, d8=True)


def check_d8(inp, got):
    assert equal(got["codes"], c_oracle.d8(inp["z"]))
    assert equal(got["codes"], hdem_oracle_np.d8_flow_direction(inp["z"]))


@case("d8", WINDOW_SHAPES + [(3, 3), (1, 9)], dem_of(True), check_d8)
def _(call, inp):
    z = call.up(inp["z"])
    return {"codes": call.host(B.d8_dev(z, out=call.out(z.shape, np.uint8)))}, None


def blockmax_case(block):
    def check(inp, got):
        z = inp["z"]
        zn = np.where(np.isnan(z), np.finfo(np.float32).max, z)
        ch, cw = -(-z.shape[0] // block), -(-z.shape[1] // block)
        pad = np.full((ch * block, cw * block), -np.inf, dtype=np.float32)
        pad[:z.shape[0], :z.shape[1]] = zn
        assert equal(got["coarse"], pad.reshape(ch, block, cw, block).max(axis=(1, 3)))

    @case(f"blockmax-{block}", WINDOW_SHAPES, dem_of(True), check)
    def _(call, inp):
        z = call.up(inp["z"])
        shape = (-(-z.shape[0] // block), -(-z.shape[1] // block))
        return {"coarse": call.host(B.blockmax_dev(z, block, out=call.out(shape, np.float32)))}, None


blockmax_case(4)
blockmax_case(16)


# ---------------------------------------------------------------------------
# the windowed operators
# ---------------------------------------------------------------------------
def boxmean_case(dtype, do_round):
    def build(shape, seed):
        x = hdem_synth.synth_dem(*shape).astype(dtype)
        if dtype == np.float64:
            x = x + np.random.default_rng(seed).standard_normal(shape) * 1e-3
        return {"x": x}

    def check(inp, got):
        assert got["mean"].dtype == dtype and equal(got["mean"], c_oracle.boxmean3(inp["x"], do_round))

    @case(f"boxmean3-{np.dtype(dtype).name}-{'round' if do_round else 'plain'}",
          WINDOW_SHAPES + [(1, 5)], build, check)
    def _(call, inp):
        x = call.up(inp["x"])
        return {"mean": call.host(B.boxmean3_dev(x, do_round, out=call.out(x.shape, dtype)))}, None


for _dtype in (np.float32, np.float64):
    for _round in (True, False):
        boxmean_case(_dtype, _round)


def check_quadratic(inp, got):
    dem, q = inp["z"], got["smooth"]
    assert np.abs(q.astype(np.float64) - c_oracle.quadratic_ref(dem, 15)).max() <= TOL
    assert np.abs(q - hdem_oracle_np.quadratic_exact64(dem, 15)).max() <= TOL
    ring = np.ones(dem.shape, bool)
    ring[7:-7, 7:-7] = False
    assert equal(q[ring], dem[ring])                     # the border ring is the input's


@case("quadratic-15", WINDOW_SHAPES, dem_of(False), check_quadratic)
def _(call, inp):
    z = call.up(inp["z"])
    return {"smooth": call.host(B.quadratic_dev(z, 15, out=call.out(z.shape, np.float32)))}, None


def groves_of(shape, seed):
    rng = np.random.default_rng(seed)
    img = hdem_synth.synth_dem(*shape)
    img = (img + np.where(rng.random(shape) < 0.04, rng.uniform(1, 6, shape), 0)).astype(np.float32)
    return {"img": img, "groves": hdem_synth.synth_groves(*shape)}


def check_groves(inp, got):
    want = c_oracle.groves_ref(inp["img"], inp["groves"], 3)
    _, stages = hdem_oracle_np.groves_exact64(inp["img"], inp["groves"], 3)
    excused = _groves_compare(got["img"], want, [s[0] for s in stages])
    assert excused <= _groves_excused_limit(inp["img"])


@case("groves-3", WINDOW_SHAPES, groves_of, check_groves)
def _(call, inp):
    img, groves = call.up(inp["img"]), call.up(np.ascontiguousarray(inp["groves"], np.uint8))
    out = B.groves_dev(img, groves, 15, 1.5, 3, out=call.out(img.shape, np.float32),
                       scratch=call.empty(img.shape, np.float32))
    return {"img": call.host(out)}, None


def elementwise_case(name, op, dtype, operand, ufunc, image_first=True):
    """One operator of each kind; the reference is the NumPy ufunc on the logical types."""
    def build(shape, seed):
        rng = np.random.default_rng([seed, *shape])
        image = (rng.random(shape) * 9 - 3).astype(dtype) if np.dtype(dtype).kind == "f" else \
            rng.integers(0, 7, shape).astype(dtype)
        other = operand
        if operand == "raster":
            other = (rng.random(shape) * 5).astype(np.float32)
        return {"image": image, "other": other}

    def check(inp, got):
        image, other = inp["image"], inp["other"]
        image = image.astype(np.int64) if image.dtype == np.uint8 else image
        want = ufunc(image, other) if image_first else ufunc(other, image)
        assert same_as_numpy(got["result"], want)

    @case("elementwise-" + name, WINDOW_SHAPES, build, check)
    def _(call, inp):
        image, other = call.up(inp["image"]), inp["other"]
        if isinstance(other, np.ndarray):
            other = call.up(other)
        first = B.elementwise_dev(op, image, other)
        got = call.host(first)
        if not call.own:
            return {"result": got}, None
        out = B.elementwise_dev(op, image, other, out=call.empty(first.shape, first.dtype))
        return {"result": call.host(out)}, None


elementwise_case("mul-raster", B.EW_MUL, np.float32, "raster", np.multiply)
elementwise_case("add-scalar", B.EW_ADD, np.float32, 2.5, np.add)
elementwise_case("rsub-scalar", B.EW_RSUB, np.float64, 1.5, np.subtract, image_first=False)
elementwise_case("gt-scalar", B.EW_GT, np.float32, 0.1, np.greater)
elementwise_case("lt-scalar", B.EW_LT, np.int64, 4, np.less)
elementwise_case("nonzero", B.EW_NONZERO, np.uint8, 0, np.not_equal)


def hsheds_of(shape, seed):
    hs = hdem_synth.synth_hsheds(*shape, seed=seed)
    _, stages = OL.lagoons_detection(hs)
    rng = np.random.default_rng([seed, *shape])
    return {"hs": hs, "stages": stages, "major": stages["MajorityFilter"].astype(np.float32),
            "blobs": ndimage.binary_dilation(rng.random(shape) < 0.03, iterations=3).astype(np.uint8)}


def correct_nan_case(window):
    def check(inp, got):
        assert equal(got["fixed"], OL.correct_nan_values(inp["hs"], window))

    @case(f"correct_nan-{window}", WINDOW_SHAPES, hsheds_of, check)
    def _(call, inp):
        hs = call.up(inp["hs"])
        out = B.correct_nan_dev(hs, call.out(hs.shape, np.float32), window)
        return {"fixed": call.host(out)}, None


def majority_case(window):
    def check(inp, got):
        fixed = inp["stages"]["CorrectNANValues"]
        assert equal(got["major"], OL.majority_filter(fixed, window))

    @case(f"majority-{window}", WINDOW_SHAPES, hsheds_of, check)
    def _(call, inp):
        fixed = call.up(np.ascontiguousarray(inp["stages"]["CorrectNANValues"], np.float32))
        out = B.majority_dev(fixed, window, out=call.out(fixed.shape, np.float32))
        return {"major": call.host(out)}, None


for _window in (3, 5):
    correct_nan_case(_window)
for _window in (5, 11):
    majority_case(_window)

CROSS = ndimage.generate_binary_structure(2, 1)
ONES3 = np.ones((3, 3), bool)
# W % 4 == 0 takes erode_cross4_kernel with the cross, everything else morph_kernel
EROSION_SHAPES = WINDOW_SHAPES + [(131, 156)]


def erosion_case(iterations, name, structure):
    def check(inp, got):
        want = ndimage.binary_erosion(inp["blobs"] != 0, structure=structure, iterations=iterations)
        assert equal(got["mask"], want.astype(np.uint8))
        if structure is CROSS:
            assert equal(got["mask"], OL.binary_erosion(inp["blobs"] != 0, iterations))

    @case(f"erosion-{name}-{iterations}", EROSION_SHAPES, hsheds_of, check)
    def _(call, inp):
        mask = call.up(inp["blobs"])
        out = B.binary_erosion_dev(mask, iterations, None if structure is CROSS else structure,
                                   out=call.out(mask.shape, np.uint8))
        return {"mask": call.host(out)}, None


for _iterations in (1, 2):
    erosion_case(_iterations, "cross", CROSS)
    erosion_case(_iterations, "ones3", ONES3)


def check_closing(inp, got):
    assert equal(got["mask"], OL.binary_closing(inp["blobs"] != 0).astype(np.uint8))


@case("closing", WINDOW_SHAPES, hsheds_of, check_closing)
def _(call, inp):
    mask = call.up(inp["blobs"])
    return {"mask": call.host(B.binary_closing_dev(mask, out=call.out(mask.shape, np.uint8)))}, None


def dilation_case(size, dtype):
    def build(shape, seed):
        rng = np.random.default_rng([seed, *shape])
        return {"img": (rng.standard_normal(shape) * 100).astype(dtype)}

    def check(inp, got):
        assert got["img"].dtype == dtype and equal(got["img"], OL.grey_dilation(inp["img"], size))

    @case(f"grey_dilation-{size[0]}x{size[1]}-{np.dtype(dtype).name}", WINDOW_SHAPES, build, check)
    def _(call, inp):
        img = call.up(inp["img"])
        return {"img": call.host(B.grey_dilation_dev(img, size, out=call.out(img.shape, dtype)))}, None


for _size in ((7, 7), (3, 5)):
    for _dtype in (np.float32, np.float64):
        dilation_case(_size, _dtype)


def check_tidying(inp, got):
    assert equal(got["tidy"], OL.tidying_lagoons(inp["major"]))


@case("tidying_lagoons", WINDOW_SHAPES, hsheds_of, check_tidying)
def _(call, inp):
    img = call.up(inp["major"])
    return {"tidy": call.host(B.tidying_lagoons_dev(img, out=call.out(img.shape, np.float32)))}, None


def check_lagoons(inp, got):
    mask, stages = OL.lagoons_detection(inp["hs"])
    assert equal(got["mask"], mask)
    assert equal(got["fixed"], stages["CorrectNANValues"])
    assert equal(got["values"], stages["TidyingLagoons"])


@case("lagoons_detection", WINDOW_SHAPES, hsheds_of, check_lagoons, own=False)
def _(call, inp):
    mask, fixed, values = B.lagoons_detection_dev(call.up(inp["hs"]))
    return {"mask": call.host(mask), "fixed": call.host(fixed), "values": call.host(values)}, None


# ---------------------------------------------------------------------------
# the Fourier chain
# ---------------------------------------------------------------------------
def striped_of(shape, seed):
    dem = hdem_synth.synth_striped_dem(*shape, seed=seed)
    _, mag = OF.fourier_initial(dem)
    detected, _ = OF.detect_blanks_fourier(mag.astype(np.float32))
    return {"dem": dem, "mag": mag.astype(np.float32), "detected": (detected > 0).astype(np.uint8)}


def check_destripe(inp, got):
    want, want_mask, _ = OF.detect_apply_fourier(inp["dem"])
    assert equal(got["mask"], want_mask)
    assert got["dem"].dtype == np.float32 and np.abs(got["dem"] - want).max() <= FOURIER_TOL


@case("fourier_destripe", FOURIER_SHAPES, striped_of, check_destripe)
def _(call, inp):
    dem = call.up(inp["dem"])
    mask = call.empty(dem.shape, np.uint8)
    out = B.fourier_destripe_dev(dem, out=call.out(dem.shape, np.float32), mask=mask)
    return {"dem": call.host(out), "mask": call.host(mask)}, None


def check_blanks(inp, got):
    found, q_mod, _ = OF.blanks_fourier(inp["mag"])
    assert equal(got["found"], found) and equal(got["q"], q_mod)


@case("blanks_fourier", FOURIER_SHAPES, striped_of, check_blanks)
def _(call, inp):
    q = call.up(inp["mag"])
    found = B.blanks_fourier_dev(q, found=call.out(q.shape, np.uint8))
    return {"found": call.host(found), "q": call.host(q)}, None


def check_isolated(inp, got):
    assert equal(got["mask"], OF.isolated_points(inp["detected"]))


@case("isolated_points", FOURIER_SHAPES, striped_of, check_isolated)
def _(call, inp):
    m = call.up(inp["detected"])
    return {"mask": call.host(B.isolated_points_dev(m, 3, out=call.out(m.shape, np.uint8)))}, None


def check_expand(inp, got):
    assert equal(got["mask"], OF.expand(inp["detected"]))


@case("expand", FOURIER_SHAPES, striped_of, check_expand)
def _(call, inp):
    m = call.up(inp["detected"])
    return {"mask": call.host(B.expand_dev(m, 13, out=call.out(m.shape, np.uint8)))}, None


def fft_case(dtype, inverse):
    forward_bar, inverse_bar = (FFT_RTOL, FFT_RTOL) if dtype == np.complex64 else \
        (FFT64_RTOL, IFFT64_RTOL)

    def build(shape, seed):
        rng = np.random.default_rng([seed, *shape])
        x = rng.standard_normal(shape) * 10 + 100 + 1j * rng.standard_normal(shape)
        return {"x": x.astype(dtype)}

    def check(inp, got):
        x = inp["x"].astype(np.complex128)
        want = fftpack.ifft2(x) * x.size if inverse else fftpack.fft2(x)     # (unnormalised)
        assert got["x"].dtype == dtype
        assert np.abs(got["x"] - want).max() <= (inverse_bar if inverse else forward_bar) * \
            np.abs(want).max()

    # in place: no out= to give
    @case(f"fft2-{np.dtype(dtype).name}-{'inverse' if inverse else 'forward'}", FOURIER_SHAPES,
          build, check, own=False)
    def _(call, inp):
        return {"x": call.host(B.fft2_dev(call.up(inp["x"]), inverse))}, None


for _dtype in (np.complex64, np.complex128):
    for _inverse in (False, True):
        fft_case(_dtype, _inverse)


# ---------------------------------------------------------------------------
# b. every device entry point is independent of the poison
# ---------------------------------------------------------------------------
PARAMS = [(entry, shape) for entry in CASES for shape in entry.shapes]
IDS = [f"{entry.name}-{shape[0]}x{shape[1]}" for entry, shape in PARAMS]
_BASELINE = {}


def baseline(entry, shape):
    """(inputs, R0, its stats): the run without poison, made once."""
    key = (entry.name, shape)
    if key not in _BASELINE:
        inputs = entry.build(shape, SEED)
        _BASELINE[key] = (inputs, *execute(entry, inputs, None, False))
    return _BASELINE[key]


def test_the_table_names_every_device_entry_point_of_the_binding():
    assert len({entry.name for entry in CASES}) == len(CASES)
    named = {n for n in dir(B) if n.endswith("_dev") and not n.startswith("_")
             and callable(getattr(B, n))}
    named |= {"upstream_dev", "streamorder_dev"}
    source = open(__file__, encoding="utf-8").read()
    assert not [n for n in sorted(named) if f".{n}(" not in source]


@pytest.mark.parametrize("entry,shape", PARAMS, ids=IDS)
def test_the_run_without_poison_is_the_cpu_reference(entry, shape):
    inputs, got, _ = baseline(entry, shape)
    entry.check(inputs, got)


@pytest.mark.parametrize("byte", POISON, ids=lambda b: f"poison{b:02X}")
@pytest.mark.parametrize("entry,shape", PARAMS, ids=IDS)
def test_poisoned_workspace_and_outputs_change_no_byte(entry, shape, byte):
    inputs, want, want_stats = baseline(entry, shape)
    for own in (False, True) if entry.own else (False,):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} {shape} under 0x{byte:02X}, out= {whose}"
        got, stats = execute(entry, inputs, byte, own)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what


# ---------------------------------------------------------------------------
# a. the hook does what it says
# ---------------------------------------------------------------------------
def test_scribble_fills_fresh_and_cached_blocks_and_stops_when_told():
    ctx = B.Context()
    try:
        shape = (37, 53)
        ones = np.full(shape, 1.0, np.float32)
        with ctx.scribble(0xA5):
            first = DeviceRaster.empty(shape, np.float32, ctx)
            assert (first.to_host().view(np.uint8) == 0xA5).all()
            ctx.check(ctx.lib.hdem_memcpy_h2d(ctx.handle, first.ptr, ones.ctypes.data, ones.nbytes))
            address = first.ptr
            first.free()
            again = DeviceRaster.empty(shape, np.float32, ctx)       # the cached block
            assert again.ptr == address
            assert (again.to_host().view(np.uint8) == 0xA5).all()
            ctx.check(ctx.lib.hdem_memcpy_h2d(ctx.handle, again.ptr, ones.ctypes.data, ones.nbytes))
            again.free()
        kept = DeviceRaster.empty(shape, np.float32, ctx)             # the mode is off again
        assert kept.ptr == address
        assert np.array_equal(kept.to_host(), ones)
        kept.free()
        for bad in (-1, 256, 2.5, True):
            with pytest.raises(ValueError):
                with ctx.scribble(bad):
                    pass
        assert ctx.lib.hdem_set_scribble(ctx.handle, 256) == B.BAD_ARG
        assert ctx.lib.hdem_set_scribble(None, 1) == B.BAD_ARG
    finally:
        ctx.close()


def test_scribble_fills_exactly_the_arena_bytes_an_operator_asks_for():
    """The stream order keeps its views behind the flow trace's bytes and calls the trace,
    which asks for those bytes only: were the nested request poisoned any further, the stop
    mask and the node words would go (order-acc-nolink keeps the first stops there too)."""
    entry = next(e for e in CASES if e.name == "streamorder-acc-nolink")
    inputs, want, _ = baseline(entry, (130, 197))
    got, _ = execute(entry, inputs, 0xFF, False)
    assert_same_bytes(got, want, "the nested arena request")
    assert int(got["order"].max()) >= 3                          # there was something to lose


# ---------------------------------------------------------------------------
# c. the host-pointer entry points and the composed chains, on the default context
# ---------------------------------------------------------------------------
def _host_flowacc(i):
    return {"acc": hd.FlowAccumulation().apply(i["codes"])}


def _host_watersheds(i):
    f = hd.Watersheds(labels="compact")
    return {"compact": f.apply(i["codes"]),
            "pour": hd.Watersheds(pour_points=i["seeds"]).apply(i["codes"])}


def _host_hand(i):
    f = hd.HeightAboveDrainage(dem=i["dem"], streams=i["acc"], threshold=THRESHOLD, cellsize=CELL)
    return {"hand": f.apply(i["codes"])}


def _host_flats(i):
    return {"codes": hd.ResolveFlats(dem=i["flat_dem"]).apply(i["flat_codes"])}


def _host_depressions(i):
    f = hd.Depressions(dem=i["z"], table=True, cellsize=CELL)
    got = {"labels": f.apply(i["filled"])}
    got.update({"table_" + k: v for k, v in f.table.items()})
    g = hd.DepressionInventory(cellsize=CELL)
    got["inventory"] = g.apply(i["z"])
    got["inventory_filled"] = g.filled
    got.update({"inventory_" + k: v for k, v in g.table.items()})
    return got


def _host_upstream(i):
    return {"length": hd.UpstreamFlowLength(cellsize=CELL).apply(i["codes"])}


def _host_streamorder(i):
    return {"order": hd.StreamOrder(i["acc"], threshold=THRESHOLD).apply(i["codes"]),
            "magnitude": hd.StreamOrder(method="shreve").apply(i["codes"])}


def _host_sinkfill(i):
    return {"filled": hd.SinkFill().apply(i["z"]), "eps": hd.SinkFill(epsilon=1e-3).apply(i["z"])}


def _host_lagoons(i):
    f = hd.LagoonsDetection()
    mask = f.apply(i["hs"].copy())
    return {"mask": mask, "fixed": f.hsheds_nan_fixed, "values": f.lagoons_values}


def _host_fourier(i):
    f = hd.DetectApplyFourier(keep_mask=True)
    return {"dem": f.apply(i["striped"]), "mask": f.mask}


def _host_groves(i):
    return {"img": hd.GrovesCorrectionsIter(i["groves"], iterations=3).apply(i["img"])}


def _host_conditioning(i):
    f = hd.HydroConditioning()
    return {"codes": f.apply(i["z"]), "filled": f.filled}


def _host_dem_to_hand(i):
    return {"hand": hd.DemToHAND(threshold=THRESHOLD, cellsize=CELL).apply(i["z"])}


def _host_dem_to_order(i):
    return {"order": hd.DemToStreamOrder(threshold=THRESHOLD).apply(i["z"])}


HOST_CALLS = {"FlowAccumulation": _host_flowacc, "Watersheds": _host_watersheds,
              "HeightAboveDrainage": _host_hand, "ResolveFlats": _host_flats,
              "Depressions+DepressionInventory": _host_depressions,
              "UpstreamFlowLength": _host_upstream, "StreamOrder": _host_streamorder,
              "SinkFill": _host_sinkfill, "LagoonsDetection": _host_lagoons,
              "DetectApplyFourier": _host_fourier, "GrovesCorrectionsIter": _host_groves,
              "HydroConditioning": _host_conditioning, "DemToHAND": _host_dem_to_hand,
              "DemToStreamOrder": _host_dem_to_order}


@pytest.fixture(scope="module")
def host_inputs():
    inputs = dict(codes_of((130, 197), SEED))
    flats = flats_of((130, 197), SEED)
    inputs.update(flat_dem=flats["dem"], flat_codes=flats["codes"])
    inputs.update(filled_of((130, 197), SEED))
    inputs["z"] = inputs["dem"]
    inputs.update(groves_of((131, 157), SEED))
    inputs["hs"] = hdem_synth.synth_hsheds(131, 157, seed=SEED)
    inputs["striped"] = hdem_synth.synth_striped_dem(150, 168, seed=SEED)
    return inputs


@pytest.mark.parametrize("name", list(HOST_CALLS))
def test_the_host_entry_points_stage_through_poisoned_blocks(name, host_inputs):
    run = HOST_CALLS[name]
    want = {k: np.ascontiguousarray(v) for k, v in run(host_inputs).items()}
    ctx = B.context()
    try:
        with ctx.scribble(0xFF):
            got = {k: np.ascontiguousarray(v) for k, v in run(host_inputs).items()}
    finally:
        ctx.check(ctx.lib.hdem_set_scribble(ctx.handle, -1))
    assert_same_bytes(got, want, f"{name} under 0xFF")
    # and the mode is off: a written block comes back from the cache as it was left
    ones = np.full((41, 43), 1.0, np.float32)
    first = DeviceRaster.from_host(ones, ctx=ctx)
    address = first.ptr
    first.free()
    with DeviceRaster.empty(ones.shape, np.float32, ctx) as again:
        if again.ptr == address:
            assert np.array_equal(again.to_host(), ones)


# ---------------------------------------------------------------------------
# d. leftovers without the hook: one context, sizes going down and up
# ---------------------------------------------------------------------------
def _fill_on(ctx, z):
    with DeviceRaster.from_host(z, ctx=ctx) as zd:
        out, stats = B.sinkfill_dev(zd, flags=B.FILL_INIT)
        with out:
            return {"filled": out.to_host()}, counters(stats, FILL_SCHEDULE)


def _on_a_fresh_context(run, *args):
    ctx = B.Context()
    try:
        return run(ctx, *args)
    finally:
        ctx.close()


def test_sinkfill_workspace_left_by_other_sizes_changes_nothing():
    """fill_ws and the hub buffers are reused, not regrown, from the second call on; the hook
    leaves them alone by design (they carry resumable and prepared state)."""
    rasters = [hdem_synth.synth_dem(519, 508), hdem_synth.synth_dem(126, 190),
               hdem_synth.synth_dem(3, 3), hdem_synth.synth_dem(519, 508, variant="srtm")]
    ctx = B.Context()
    try:
        sequence = [_fill_on(ctx, z) for z in rasters]
    finally:
        ctx.close()
    for k, (z, (got, stats)) in enumerate(zip(rasters, sequence)):
        want, want_stats = _on_a_fresh_context(_fill_on, z)
        assert_same_bytes(got, want, f"fill {k} of the sequence, {z.shape}")
        assert stats == want_stats, k
    assert equal(sequence[-1][0]["filled"], c_oracle.sinkfill_pflood(rasters[-1]))


def _trace_on(ctx, inp):
    with DeviceRaster.from_host(inp["codes"], ctx=ctx) as codes, \
            DeviceRaster.from_host(inp["acc"], ctx=ctx) as acc:
        outs, stats = B.flowtrace_dev(codes, acc, THRESHOLD, None, CELL, ("stop", "distance"))
        with contextlib.ExitStack() as stack:
            for r in outs.values():
                stack.enter_context(r)
            return {k: r.to_host() for k, r in outs.items()}, counters(stats)


def _flowacc_on(ctx, inp):
    with DeviceRaster.from_host(inp["codes"], ctx=ctx) as codes:
        out, stats = B.flowacc_dev(codes)
        with out:
            return {"acc": out.to_host()}, counters(stats, ("max_hops",))


def _depressions_on(ctx, inp):
    with DeviceRaster.from_host(inp["dem"], ctx=ctx) as dem, \
            DeviceRaster.from_host(inp["filled"], ctx=ctx) as filled:
        out, stats = B.depressions_dev(dem, filled, True)
        with out:
            return {"labels": out.to_host()}, counters(stats)


def test_arena_left_by_a_larger_operator_changes_nothing():
    big = {"codes": random_acyclic_codes(700, 900, SEED, ramp=True)}
    big["acc"] = acc_kahn(big["codes"]).astype(np.uint32)
    steps = [(_trace_on, big), (_flowacc_on, codes_of((130, 197), SEED)),
             (_depressions_on, filled_of((65, 64), SEED))]
    ctx = B.Context()
    try:
        sequence = [run(ctx, inp) for run, inp in steps]
    finally:
        ctx.close()
    for (run, inp), (got, stats) in zip(steps, sequence):
        want, want_stats = _on_a_fresh_context(run, inp)
        assert_same_bytes(got, want, run.__name__)
        assert stats == want_stats, run.__name__
    assert equal(sequence[1][0]["acc"], steps[1][1]["acc"])
