"""
One table of every device entry point of the binding (a plain helper module, no tests).

The cases live where their references live: ``tests/test_gpu_scribble.py`` has the table of the
operators that existed when it was written, and the files of the newer operators each keep a
``Case`` (or a ``poison_case`` factory) of their own, through which their poison test runs.  Here
they are collected, ``ENTRIES``, and each is given the **one** shape at which it is run where the
subject is not the operator's sizes but something around it (the stream and the context, in
``tests/test_gpu_streams.py``): the smallest at which the operator has more than one tile and a
partial one,

    tiled D8, D-infinity, proximity, zonal, streamnet, depressions, flats    (130, 197)
    windowed and lagoon operators                                            (131, 157)
    terrain and the D-infinity direction (a second 256-column tile)          (33, 257)
    destripe (split inverse)                                                 (150, 168), (256, 256)
    FFTs and the other single steps of the Fourier chain                     (141, 155)
    fill and fill + D8 (the second takes the hub start)                      (200, 333), (519, 508)
    the fill's protocols: a caller's hub start, coarse start, seam rows      (519, 508), (200, 333),
                                                                             (130, 197)

A case is ``Case(name, shapes, build, run, check, own, schedule)`` of test_gpu_scribble:
``build(shape, seed)`` makes the host inputs, ``run(call, inputs)`` makes the device calls through
``call.up`` / ``call.out`` / ``call.empty`` / ``call.host`` and returns ``({name: host array},
stats or None)``, ``check(inputs, got)`` holds the run to the CPU reference under the bar of the
operator's own test file.

``symbols_reached`` says which C symbols of ``backend.SIGNATURES`` a case reaches, by a
source-text rule (``tests/test_device_cases.py`` holds the table to it): the names a case's
``run`` calls as attributes (``B.flowacc_dev(``) are followed through the functions of the package
by their plain names, a bare name in its caller's module first, and a symbol is reached where
it stands in such a function as a string or an attribute, docstrings apart, or where the
function hands its stem to ``side.call``, which appends ``_dev`` for the device side.  The rule
can claim too much through a name that several functions share, never too little.
"""
import ast
import collections
import inspect
import pathlib
import re

import numpy as np

import test_gpu_dinf as DI
import test_gpu_dinfsum as DS
import test_gpu_elevation_regimes as ER
import test_gpu_flowpath as FP
import test_gpu_flowsum as FS
import test_gpu_proximity as PX
import test_gpu_scribble as S
import test_gpu_streamnet as SN
import test_gpu_terrain_area as TR
import test_gpu_terrain_attributes as TA
import test_gpu_upextreme as UE
import test_gpu_zonal as ZO
from hydrodem_amd import backend as B
from oracle import c_oracle
from test_gpu_scribble import Case

D8_SHAPE, WINDOW_SHAPE, TERRAIN_SHAPE, FFT_SHAPE = (130, 197), (131, 157), (33, 257), (141, 155)
DESTRIPE_SHAPES, FILL_SHAPES = ((150, 168), (256, 256)), ((200, 333), (519, 508))

Entry = collections.namedtuple("Entry", "case shapes")


def _shapes_of(name):
    """The shapes of a case of test_gpu_scribble's table, by the operator's group."""
    if name.startswith("sinkfill"):
        return FILL_SHAPES
    if name == "fourier_destripe":
        return DESTRIPE_SHAPES
    if name.startswith("fft2-") or name in ("blanks_fourier", "isolated_points", "expand"):
        return (FFT_SHAPE,)
    if name.split("-")[0] in ("flowacc", "watershed", "flowtrace", "upstream", "streamorder",
                              "resolve_flats", "depressions"):
        return (D8_SHAPE,)
    return (WINDOW_SHAPE,)


# ---------------------------------------------------------------------------
# the factories of the proximity and terrain files, given their inputs and references
# ---------------------------------------------------------------------------
def _proximity(name, want, layout):
    made = PX.poison_case(name, want, D8_SHAPE, layout)

    def check(inp, got):
        assert set(got) == set(want)
        PX.assert_matches(got, PX.expected(D8_SHAPE, layout), name)
    return made._replace(shapes=(D8_SHAPE,), build=lambda shape, seed: PX.inputs(shape, layout),
                         check=check)


def _terrain_bars(got, ref, fin, hole, what):
    """The bars of test_every_output_against_the_reference, for the outputs that are there."""
    for name in ("dzdx", "dzdy", "d8_slope"):
        assert name not in got or TA.same_bits(got[name], ref[name]), (what, name)
    assert "tangent" not in got or TA.ulps_f32(got["tangent"], ref["tangent"]) <= 1, what
    assert "spi" not in got or TA.ulps_f32(got["spi"], ref["spi"]) <= 2, what
    for name in ("degrees", "aspect"):
        if name in got:
            assert np.isnan(got[name][hole]).all()
            assert TA.worst(name, got[name], ref[name], fin) <= TA.N_ULP[name], (what, name)


def _terrain(name, want, slope):
    made = TA.poison_case(name, want, slope)

    def check(inp, got):
        assert set(got) == set(want)
        ref = TA.reference("synth", TERRAIN_SHAPE, slope)
        fin, _ = TA.usable(TA.reference("synth", TERRAIN_SHAPE))
        hole = np.isnan(inp["dem"])
        _terrain_bars(got, ref, fin, hole, name)
        # (along the D8 slope the reference itself has NaN outside the holes: its bar is that of
        # test_wetness_along_the_d8_slope, over the cells where the reference is a number)
        keep = fin if slope == "horn" else ~np.isnan(ref["twi"])
        assert np.isnan(got["twi"][hole if slope == "horn" else ~keep]).all()
        assert TA.worst("twi", got["twi"], ref["twi"], keep) <= TA.N_ULP["twi"], name
    return made._replace(shapes=(TERRAIN_SHAPE,), build=lambda shape, seed: TA.inputs("synth", shape),
                         check=check)


def _terrain_area(name, want, slope):
    made = TR.poison_case(name, want, slope)

    def check(inp, got):
        assert set(got) == set(want)
        base, ref = TA.reference("synth", TERRAIN_SHAPE), TR.area_ref(TERRAIN_SHAPE, slope)
        fin, _ = TA.usable(base)
        hole = np.isnan(inp["dem"])
        _terrain_bars(got, {**base, "spi": ref["spi"]}, fin, hole, name)
        assert np.isnan(got["twi"][hole]).all() and np.isnan(got["spi"][hole]).all()
        TR.assert_twi(got["twi"], ref["twi"], fin, name)
    return made._replace(shapes=(TERRAIN_SHAPE,), build=lambda shape, seed: TR.area_inputs(shape),
                         check=check)


# ---------------------------------------------------------------------------
# the two entry points that move bytes and have no operator around them
# ---------------------------------------------------------------------------
def _bytes_of(shape, seed):
    rng = np.random.default_rng([seed, *shape])
    return {"x": rng.standard_normal(shape).astype(np.float32)}


def _run_copy(call, inp):
    src = call.up(inp["x"])
    dst = call.out(src.shape, np.float32) or call.empty(src.shape, np.float32)
    src.ctx.check(src.ctx.lib.hdem_copy_rate_dev(src.ctx.handle, src.ptr, dst.ptr, src.nbytes))
    return {"copy": call.host(dst)}, None


def _check_copy(inp, got):
    assert got["copy"].tobytes() == inp["x"].tobytes()


def _run_memset(call, inp):
    x = call.up(inp["x"])
    x.ctx.check(x.ctx.lib.hdem_memset_dev(x.ctx.handle, x.ptr + 16, 0xA5, x.nbytes - 48))
    return {"x": call.host(x)}, None


def _check_memset(inp, got):
    want = inp["x"].copy().reshape(-1).view(np.uint8)
    want[16:-32] = 0xA5
    assert got["x"].tobytes() == want.tobytes()


# ---------------------------------------------------------------------------
# the sink fill's protocols: what one call tells the context for a later one
# ---------------------------------------------------------------------------
FILL_TILE = 62                    # tile edge of the fill (hdem_fill_stats.tile_h)
HUB_WALL = 3.0e38                 # a wall of the hub raster (hdem_sinkfill.hip, partition.HUB_BIG)
COARSE_BLOCK = 16
# the rows of _seam_inputs a variant receives as (top, bottom); None: no such neighbour
SEAM_ROWS = {"both": ("top_zeros", "bot_same"), "top": ("top_same", None), "none": (None, None)}
SEAM_PENDING, SEAM_PRESET = (-1, 0, 3), (0, 1)


def hub_raster_shape(shape):
    """(2 ty + 1, 2 tx + 1) of include/hydrodem_hip.h."""
    return tuple(2 * -(-(n - 2) // FILL_TILE) + 1 for n in shape)


def _assert_fill_and_codes(inp, got):
    want = c_oracle.sinkfill_pflood(inp["z"])
    assert got["filled"].dtype == np.float32 and S.equal(got["filled"], want)
    assert got["codes"].dtype == np.uint8 and S.equal(got["codes"], c_oracle.d8(want))
    return want


def _run_hub_given(call, inp):
    """The hub start of a partition of one block, every step of partition.hub_start."""
    z = call.up(inp["z"])
    ctx, shape = z.ctx, hub_raster_shape(z.shape)
    w = call.empty(z.shape, np.float32)
    ctx.fill_hub_prepare(z.ptr, z.shape[0], z.shape[1], 0, w.ptr)
    d = w.to_host()                        # (the ring of w is nobody's yet: the raster's, below)
    raster = call.empty(shape, np.float32)
    ctx.fill_hub_raster(raster.ptr)
    levels, _ = B.sinkfill_dev(raster, out=call.empty(shape, np.float32),
                               flags=B.FILL_INIT | B.FILL_NO_VERIFY)
    ctx.set_fill_hub_levels(levels.ptr)
    out, codes, stats = B.sinkfill_d8_dev(z, out=w, codes=call.out(z.shape, np.uint8),
                                          flags=B.FILL_INIT)
    d[0], d[-1], d[:, 0], d[:, -1] = inp["z"][0], inp["z"][-1], inp["z"][:, 0], inp["z"][:, -1]
    return {"raster": call.host(raster), "levels": call.host(levels), "d": d,
            "filled": call.host(out), "codes": call.host(codes)}, stats


def _check_hub_given(inp, got):
    """The oracle's bits, and the start values the levels stand for -- max(d, level of the
    cell's tile), an outlet tile (NaN) keeping d -- as upper bounds of the fill."""
    z = inp["z"]
    want = _assert_fill_and_codes(inp, got)
    assert got["raster"].shape == got["levels"].shape == hub_raster_shape(z.shape)
    level = got["levels"][1::2, 1::2].copy()
    level[level >= HUB_WALL] = np.inf
    level = np.repeat(np.repeat(level, FILL_TILE, 0), FILL_TILE, 1)[:z.shape[0] - 2, :z.shape[1] - 2]
    u, d = got["d"].copy(), got["d"][1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        u[1:-1, 1:-1] = np.where(np.isnan(level) | np.isnan(d), d, np.maximum(d, level))
    ER.assert_bounds(u, want)
    assert np.isfinite(got["levels"][1::2, 1::2]).any()          # (there were levels to use)


def _run_coarse_given(call, inp):
    z = call.up(inp["z"])
    shape = tuple(-(-n // COARSE_BLOCK) for n in z.shape)
    coarse = B.blockmax_dev(z, COARSE_BLOCK, out=call.empty(shape, np.float32))
    cfill, _ = B.sinkfill_dev(coarse, out=call.empty(shape, np.float32))
    z.ctx.set_fill_coarse_start(cfill.ptr, shape[0], shape[1], COARSE_BLOCK, None)
    out, codes, stats = B.sinkfill_d8_dev(z, out=call.out(z.shape, np.float32),
                                          codes=call.out(z.shape, np.uint8))
    return {"coarse": call.host(cfill), "filled": call.host(out), "codes": call.host(codes)}, stats


def _check_coarse_given(inp, got):
    z = inp["z"]
    want = _assert_fill_and_codes(inp, got)
    level = np.repeat(np.repeat(got["coarse"], COARSE_BLOCK, 0), COARSE_BLOCK, 1)
    u = np.maximum(z, level[:z.shape[0], :z.shape[1]])
    u[0], u[-1], u[:, 0], u[:, -1] = z[0], z[-1], z[:, 0], z[:, -1]
    ER.assert_bounds(u, want)


def _seam_inputs(shape, seed):
    """A deferred block and the rows its neighbours send.  Rows 0 and H-1 hold a NaN, a -0.0 and
    a +0.0.  ``top_zeros`` is row 0 with the signs of its zeros swapped: equal values, other
    bits.  ``top_same`` / ``bot_same`` are the rows themselves: the NaN is no equal value, and
    the same bits."""
    rng = np.random.default_rng([seed, *shape])
    w = (rng.standard_normal(shape) * 100).astype(np.float32)
    for row in (0, shape[0] - 1):
        w[row, 5], w[row, 70], w[row, shape[1] - 3] = np.nan, -0.0, 0.0
    top_zeros = w[:1].copy()
    top_zeros[0, 70], top_zeros[0, shape[1] - 3] = 0.0, -0.0
    return {"w": w, "top_zeros": top_zeros, "top_same": w[:1].copy(), "bot_same": w[-1:].copy()}


def _run_seam_apply(call, inp):
    fresh = call.up(inp["w"])
    ctx, (H, W) = fresh.ctx, fresh.shape
    w = call.empty(fresh.shape, np.float32)
    sent = {name: call.up(inp[name]) for name in ("top_zeros", "top_same", "bot_same")}
    got = {}
    for rows, (top, bot) in SEAM_ROWS.items():
        for pending in SEAM_PENDING:
            for preset in SEAM_PRESET:
                ctx.check(ctx.lib.hdem_memcpy_d2d(ctx.handle, w.ptr, fresh.ptr, fresh.nbytes))
                words = call.up(np.full((1, 4), preset, np.uint32))
                ctx.fill_seam_apply(w.ptr, H, W, sent[top].ptr if top else 0,
                                    sent[bot].ptr if bot else 0, pending, words.ptr)
                got[f"w-{rows}-{pending}-{preset}"] = w.to_host()
                got[f"words-{rows}-{pending}-{preset}"] = call.host(words)
    return got, None


def _check_seam_apply(inp, got):
    """include/hydrodem_hip.h on hdem_fill_seam_apply_dev, in NumPy."""
    bits = lambda row: row.view(np.uint32)
    assert len(got) == 2 * len(SEAM_ROWS) * len(SEAM_PENDING) * len(SEAM_PRESET)
    for rows, names in SEAM_ROWS.items():
        top, bot = (None if name is None else inp[name] for name in names)
        want_w = inp["w"].copy()
        changed = [0, 0]
        for k, (row, sent) in enumerate(((0, top), (-1, bot))):
            if sent is not None:
                changed[k] = int((bits(sent[0]) != bits(want_w[row])).any())
                want_w[row] = sent[0]
        assert changed == {"both": [1, 0], "top": [0, 0], "none": [0, 0]}[rows]
        for pending in SEAM_PENDING:
            for preset in SEAM_PRESET:
                what = f"{rows}-{pending}-{preset}"
                queued = int(pending > 0) if pending >= 0 else int(preset != 0)
                want_words = [queued, *changed, int(bool(queued or any(changed)))]
                assert got["words-" + what].ravel().tolist() == want_words, what
                assert got["w-" + what].tobytes() == want_w.tobytes(), what


FILL_PROTOCOL_CASES = [
    Case("fill-hub-given", (FILL_SHAPES[1],), S.dem_of(False), _run_hub_given, _check_hub_given,
         True, frozenset(S.FILL_SCHEDULE)),
    Case("fill-coarse-given", (FILL_SHAPES[0],), S.dem_of(False), _run_coarse_given,
         _check_coarse_given, True, frozenset(S.FILL_SCHEDULE)),
    Case("fill-seam-apply", (D8_SHAPE,), _seam_inputs, _run_seam_apply, _check_seam_apply, False,
         frozenset()),
]


# (132 x 156 floats: the copy kernel moves 16 bytes a lane and takes whole lanes only)
BYTE_CASES = [Case("copy_rate", ((132, 156),), _bytes_of, _run_copy, _check_copy, True, frozenset()),
              Case("memset", ((132, 156),), _bytes_of, _run_memset, _check_memset, False,
                   frozenset())]

ENTRIES = [Entry(entry, _shapes_of(entry.name)) for entry in S.CASES] + [
    Entry(_proximity("proximity-all", PX.ALL, "random0.05"), (D8_SHAPE,)),
    Entry(_proximity("proximity-d2", ("d2",), "checkerboard"), (D8_SHAPE,)),
    Entry(_proximity("proximity-nearest-burned", ("nearest", "burned"), "random0.001"),
          (D8_SHAPE,)),
    Entry(_terrain("terrain-all", TA.ALL, "horn"), (TERRAIN_SHAPE,)),
    Entry(_terrain("terrain-acc-codes", ("d8_slope", "twi", "spi"), "d8"), (TERRAIN_SHAPE,)),
    Entry(_terrain_area("area-all", TR.ALL, "horn"), (TERRAIN_SHAPE,)),
    Entry(_terrain_area("area-given", ("d8_slope", "twi", "spi"), "given"), (TERRAIN_SHAPE,)),
    Entry(FS.POISON_CASE, (D8_SHAPE,)),
    Entry(UE.POISON_CASE, (D8_SHAPE,)),
    Entry(FP.POISON_CASE, (D8_SHAPE,)),
    Entry(DI.POISON_CASES[0], (D8_SHAPE,)),
    Entry(DI.POISON_CASES[1], (TERRAIN_SHAPE,)),
    Entry(DS.POISON_CASE, (D8_SHAPE,)),
    Entry(ZO.POISON_CASE, (D8_SHAPE,)),
    Entry(SN.POISON_CASE, (D8_SHAPE,)),
] + [Entry(entry, entry.shapes) for entry in FILL_PROTOCOL_CASES + BYTE_CASES]

PARAMS = [(e.case, shape) for e in ENTRIES for shape in e.shapes]
IDS = [f"{case.name}-{shape[0]}x{shape[1]}" for case, shape in PARAMS]

# Reached by no case, each with its reason.  Empty: the partition's seam exchange and its hub
# start, once excused here, are the fill's protocol cases above.
ALLOWED = {}


# ---------------------------------------------------------------------------
# which symbols a case reaches
# ---------------------------------------------------------------------------
def _package_functions():
    """{(module, plain name): [(names it calls, hdem_ words in it, whether it hands a stem to
    side.call)]} of every function and method of the package, docstrings left out.  A called
    name is kept with how it was called: bare (looked up in the caller's module first) or as an
    attribute (looked up everywhere)."""
    table = collections.defaultdict(list)
    root = pathlib.Path(B.__file__).parent
    for path in sorted(root.rglob("*.py")):
        if "dropin" in path.parts:
            continue
        for node in ast.walk(ast.parse(path.read_text(encoding="utf-8"))):
            if not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            doc = node.body[0].value if node.body and isinstance(node.body[0], ast.Expr) and \
                isinstance(node.body[0].value, ast.Constant) else None
            calls, words, sided = set(), set(), False
            for sub in ast.walk(node):
                if isinstance(sub, ast.Call):
                    f = sub.func
                    if isinstance(f, ast.Attribute):
                        calls.add((None, f.attr))
                        sided |= f.attr == "call" and isinstance(f.value, ast.Name) and \
                            f.value.id == "side"
                    elif isinstance(f, ast.Name):
                        calls.add((path.stem, f.id))
                if isinstance(sub, ast.Attribute) and sub.attr.startswith("hdem_"):
                    words.add(sub.attr)
                if isinstance(sub, ast.Constant) and isinstance(sub.value, str) and \
                        sub is not doc and re.fullmatch(r"hdem_\w+", sub.value):
                    words.add(sub.value)
            table[path.stem, node.name].append((calls, words, sided))
    return table


_FUNCTIONS = None


def _lookup(module, name):
    """The package's functions a called name may mean."""
    if module is not None and (module, name) in _FUNCTIONS:
        return _FUNCTIONS[module, name]
    return [f for (_, n), fs in _FUNCTIONS.items() if n == name for f in fs]


def symbols_reached(case):
    """The symbols of ``backend.SIGNATURES`` that ``case.run`` reaches (see the module's text)."""
    global _FUNCTIONS
    if _FUNCTIONS is None:
        _FUNCTIONS = _package_functions()
    source = inspect.getsource(case.run)
    found = set(re.findall(r"\b(hdem_\w+)\b", source))
    own = set(re.findall(r"\bdef (\w+)\(", source))
    # (what the case calls, it calls on a module of the package: ``B.flowacc_dev(``)
    todo = {(None, name) for name in re.findall(r"\.(\w+)\(", source)} - {(None, n) for n in own}
    seen = set()
    while todo:
        key = todo.pop()
        if key in seen:
            continue
        seen.add(key)
        for calls, words, sided in _lookup(*key):
            found |= words
            if sided:
                found |= {w + "_dev" for w in words}
            todo |= calls - seen
    return found & set(B.SIGNATURES)
