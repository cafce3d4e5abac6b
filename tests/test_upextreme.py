"""
Upstream D8 extremes and depression breaching (``UpstreamExtreme``, ``BreachDepressions``,
``hdem_upextreme_u8``, ``hdem_breach_f32``): the CPU half.

The host references live here and are used by tests/test_gpu_upextreme.py.  Both reduce the
64-bit word of the contract, ``key << 32 | index`` under unsigned min or ``key << 32 | ~index``
under unsigned max, a NaN being the identity:
  (a) ``upext_brute``  every cell carries its word down its path (bounded by H*W steps) with
                       ``np.minimum.at`` / ``np.maximum.at`` -- tiny grids;
  (b) ``upext_kahn``   NumPy Kahn peeling over a frontier -- any size a test uses.
``carve_ref`` is the pit stencil plus (b) in min mode; ``oracle_forest`` the forest of the
guarantee from the oracles (the eps = 0 fill, its D8, the flat resolution of tests/test_flats.py).
No GPU here: the references agree with each other and give the hand values of the order, the
carving has the properties the header promises, the operators are importable from the package
and the drop-in ``filters``, reject what they must without a device, and the header and the
library carry the entry points.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import hdem_synth
from oracle.hdem_oracle_np import D8_OFFSETS, d8_flow_direction, sinkfill_jacobi
from test_flats import resolve_flats_bfs, shifted
from test_flowacc import random_acyclic_codes, receivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOWHERE = 0xFFFFFFFF
QUIET_NAN = 0x7FC00000
IDENTITY = {"min": np.uint64(0xFFFFFFFFFFFFFFFF), "max": np.uint64(0)}


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def keys_of(values):
    """uint32 keys whose unsigned order is the values' order: a float's bits with the sign bit
    flipped (positive) or all bits flipped (negative), so -0.0 lies below +0.0; a uint32 as it
    is."""
    values = np.ascontiguousarray(values)
    if values.dtype == np.uint32:
        return values.ravel().copy()
    assert values.dtype == np.float32
    b = values.ravel().view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def words_of(values, mode):
    """The reduction word of every cell, flat uint64; the identity for a NaN."""
    values = np.ascontiguousarray(values)
    idx = np.arange(values.size, dtype=np.uint64)
    low = idx if mode == "min" else (~idx & np.uint64(0xFFFFFFFF))
    words = keys_of(values).astype(np.uint64) << np.uint64(32) | low
    if values.dtype == np.float32:
        words[np.isnan(values.ravel())] = IDENTITY[mode]
    return words


def split_words(words, mode, dtype, shape):
    """(extreme, where) of final words: the holder's bits and its flat index."""
    present = words != IDENTITY[mode]
    low = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    where = np.where(present, low if mode == "min" else ~low, np.uint32(NOWHERE))
    key = (words >> np.uint64(32)).astype(np.uint32)
    if np.dtype(dtype) == np.uint32:
        extreme = key
    else:
        bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key)
        extreme = np.where(present, bits, np.uint32(QUIET_NAN)).astype(np.uint32).view(np.float32)
    return extreme.reshape(shape), where.astype(np.uint32).reshape(shape)


def _reduce_at(mode):
    return np.minimum.at if mode == "min" else np.maximum.at


def upext_brute(codes, values, mode):
    """(a): every cell carries its own word down its path, all cells in step; a path longer
    than H*W cells is a cycle."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    total = np.full(n, IDENTITY[mode], np.uint64)
    pos = np.arange(n, dtype=np.int64)
    carried = words_of(values, mode)
    for _ in range(n):
        _reduce_at(mode)(total, pos, carried)
        pos = rec[pos]
        keep = pos >= 0
        pos, carried = pos[keep], carried[keep]
        if not pos.size:
            return split_words(total, mode, np.asarray(values).dtype, codes.shape)
    raise ValueError("flow directions form a cycle")


def upext_kahn(codes, values, mode):
    """(b): peel the cells whose donors are all done, one frontier at a time."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    indeg = np.bincount(rec[rec >= 0], minlength=n)
    total = words_of(values, mode)
    assert total.size == n
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        r = rec[frontier]
        keep = r >= 0
        f, r = frontier[keep], r[keep]
        _reduce_at(mode)(total, r, total[f])
        np.subtract.at(indeg, r, 1)
        cand = np.unique(r)
        frontier = cand[indeg[cand] == 0]
    if done != n:
        raise ValueError(f"flow directions form a cycle: {n - done} cells never drain")
    return split_words(total, mode, np.asarray(values).dtype, codes.shape)


def pits_of(dem):
    """The pit stencil: non-NaN cells off the one-cell ring with no NaN neighbour and no
    strictly lower one."""
    dem = np.asarray(dem, np.float32)
    pit = ~np.isnan(dem)
    pit[0, :] = pit[-1, :] = False
    pit[:, 0] = pit[:, -1] = False
    with np.errstate(invalid="ignore"):
        for dy, dx in D8_OFFSETS:
            n = shifted(dem, dy, dx, np.float32(np.inf))
            pit &= ~np.isnan(n) & ~(n < dem)
    return pit


def carve_ref(dem, codes):
    """(carved, source, pits, lowered) of the definition."""
    dem = np.ascontiguousarray(dem, np.float32)
    pit = pits_of(dem)
    seeds = np.where(pit, dem, np.float32(np.nan)).astype(np.float32)
    t, holder = upext_kahn(codes, seeds, "min")
    with np.errstate(invalid="ignore"):
        lower = ~np.isnan(t) & (t < dem)
    carved = np.where(lower, t.view(np.uint32), dem.view(np.uint32)).view(np.float32)
    source = np.where(lower, holder, np.uint32(NOWHERE)).astype(np.uint32)
    return carved, source, int(pit.sum()), int(lower.sum())


def oracle_forest(dem):
    """The forest of the guarantee: the ResolveFlats codes of the eps = 0 fill."""
    filled, _ = sinkfill_jacobi(dem)
    codes, _ = resolve_flats_bfs(filled, d8_flow_direction(filled))
    return codes


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def raster_of(kind, shape):
    """The three raster kinds of the carving tests."""
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    if kind == "noise":
        return rng.random(shape, dtype=np.float32) * np.float32(100)
    if kind == "steps":
        return np.floor(rng.random(shape) * 8).astype(np.float32)   # ties and flats everywhere
    assert kind == "synth"
    z = hdem_synth.synth_dem(*shape)
    if shape == (300, 300):
        z[50:60, 70:90] = np.nan
        z[120, 30] = np.nan
    return z


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
def values_of(dtype, shape, rng):
    if dtype == np.uint32:
        return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    v = ((rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(200))
    v[rng.random(shape) < 0.05] = np.nan
    return v


@pytest.mark.parametrize("dtype", [np.float32, np.uint32], ids=["f32", "u32"])
@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp, mode, dtype):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    v = values_of(dtype, shape, np.random.default_rng(shape[0] + 31 * shape[1]))
    (ea, wa), (eb, wb) = upext_brute(codes, v, mode), upext_kahn(codes, v, mode)
    assert ea.dtype == eb.dtype == v.dtype and wa.dtype == wb.dtype == np.uint32
    assert same_bytes(ea, eb) and same_bytes(wa, wb)
    # the holder holds the extreme, and lies upstream: at a cell without donors it is the cell
    present = wb != NOWHERE
    assert same_bytes(v.ravel()[wb[present]], eb[present])
    leaves = np.bincount(receivers(codes)[receivers(codes) >= 0], minlength=v.size) == 0
    own = leaves & present.ravel()
    assert np.array_equal(wb.ravel()[own], np.flatnonzero(own))
    # the extreme over the whole raster arrives at some terminal cell
    if dtype == np.uint32:
        best = v.min() if mode == "min" else v.max()
        assert best in eb.ravel()[receivers(codes) < 0]


def test_hand_values_of_the_order():
    row = np.full((1, 6), 1, np.uint8)                  # every cell drains east
    v = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, 5.0]], np.float32)
    e, w = upext_kahn(row, v, "min")
    assert same_bytes(e, np.array([[0.0, -0.0, -0.0, -np.inf, -np.inf, -np.inf]], np.float32))
    assert w.tolist() == [[0, 1, 1, 3, 3, 3]]
    e, w = upext_kahn(row, v, "max")
    assert same_bytes(e, np.array([[0.0, 0.0, np.inf, np.inf, np.inf, np.inf]], np.float32))
    assert w.tolist() == [[0, 0, 2, 2, 2, 2]]
    # -0.0 then +0.0: the minimum stays -0.0, the maximum turns +0.0
    v = np.array([[-0.0, 0.0]], np.float32)
    assert same_bytes(upext_kahn(row[:, :2], v, "min")[0], np.array([[-0.0, -0.0]], np.float32))
    assert same_bytes(upext_kahn(row[:, :2], v, "max")[0], np.array([[-0.0, 0.0]], np.float32))
    for ref in (upext_kahn, upext_brute):
        # nothing present upstream: the quiet NaN and no holder, whatever the NaN's payload
        v = np.array([0x7FC00001, 0xFFFFFFFF, 0x3F800000], np.uint32).view(np.float32)[None, :]
        for mode in ("min", "max"):
            e, w = ref(row[:, :3], v, mode)
            assert e.view(np.uint32).tolist() == [[QUIET_NAN, QUIET_NAN, 0x3F800000]]
            assert w.tolist() == [[NOWHERE, NOWHERE, 2]]
        # equal values: the smallest index in both modes
        v = np.array([[2.0, 7.0, 7.0, 2.0, 7.0, 2.0]], np.float32)
        assert ref(row, v, "min")[1].tolist() == [[0, 0, 0, 0, 0, 0]]
        assert ref(row, v, "max")[1].tolist() == [[0, 1, 1, 1, 1, 1]]
        west = np.full((1, 6), 16, np.uint8)            # and with the path running the other way
        assert ref(west, v, "min")[1].tolist() == [[0, 3, 3, 3, 5, 5]]
        assert ref(west, v, "max")[1].tolist() == [[1, 1, 2, 4, 4, 5]]
        # uint32 0 and 0xFFFFFFFF are ordinary values
        u = np.array([[7, 0, 0xFFFFFFFF, 3]], np.uint32)
        e, w = ref(row[:, :4], u, "min")
        assert e.tolist() == [[7, 0, 0, 0]] and w.tolist() == [[0, 1, 1, 1]]
        e, w = ref(row[:, :4], u, "max")
        assert e.tolist() == [[7, 7, 0xFFFFFFFF, 0xFFFFFFFF]] and w.tolist() == [[0, 0, 2, 2]]
        u = np.array([[0xFFFFFFFF, 0xFFFFFFFF]], np.uint32)
        assert ref(row[:, :2], u, "min")[1].tolist() == [[0, 0]]
        u = np.array([[0, 0]], np.uint32)
        assert ref(row[:, :2], u, "max")[1].tolist() == [[0, 0]]
    pair = np.array([[1, 16]], np.uint8)                # E then W: a 2-cycle
    for ref in (upext_kahn, upext_brute):
        with pytest.raises(ValueError):
            ref(pair, np.ones((1, 2), np.float32), "min")


# ---------------------------------------------------------------------------
# the carving
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def carved_once(kind, shape):
    dem = raster_of(kind, shape)
    codes = oracle_forest(dem)
    return (dem, codes) + carve_ref(dem, codes)


@pytest.mark.parametrize("kind,shape", [("noise", (63, 63)), ("noise", (130, 197)),
                                        ("steps", (63, 63)), ("steps", (130, 197)),
                                        ("synth", (300, 300))])
def test_the_carved_dem_has_no_sinks_and_carving_it_again_changes_nothing(kind, shape):
    dem, _, carved, source, pits, lowered = carved_once(kind, shape)
    nan = np.isnan(dem)
    assert np.all(carved[~nan] <= dem[~nan])
    assert np.array_equal(carved.view(np.uint32)[nan], dem.view(np.uint32)[nan])
    assert pits > 0 and lowered > 0
    assert lowered == int((source != NOWHERE).sum())
    assert same_bytes(dem.ravel()[source[source != NOWHERE]], carved[source != NOWHERE])
    refilled, _ = sinkfill_jacobi(carved)
    assert np.array_equal(refilled, carved, equal_nan=True)
    again, source2, _, lowered2 = carve_ref(carved, oracle_forest(carved))
    assert same_bytes(again, carved) and lowered2 == 0
    assert np.all(source2 == NOWHERE)
    if kind == "synth":
        assert nan.sum() == 201


def test_the_figures_of_the_noise_raster():
    _, _, _, _, pits, lowered = carved_once("noise", (130, 197))
    print("130 x 197 noise:", pits, "pits,", lowered, "lowered")
    assert 0 < pits < lowered


def test_rasters_without_a_pit_come_back_byte_for_byte():
    plane = np.tile(np.arange(40, 0, -1, dtype=np.float32), (30, 1))    # tilted east
    for dem in (plane, np.array([[3.5]], np.float32), np.full((3, 3), 2.0, np.float32) -
                np.eye(3, dtype=np.float32)):
        codes = oracle_forest(dem) if min(dem.shape) >= 3 else np.zeros(dem.shape, np.uint8)
        carved, source, pits, lowered = carve_ref(dem, codes)
        if dem.shape == (3, 3):
            # the centre of a 3 x 3 raster may be a pit: it has no upstream cell to lower and
            # is not below itself
            assert pits <= 1
        else:
            assert pits == 0
        assert lowered == 0 and same_bytes(carved, dem) and np.all(source == NOWHERE)


def test_a_trench_runs_from_the_pit_to_the_ring():
    dem = np.full((5, 40), 1000.0, np.float32)
    dem[2] = 500 - np.float32(0.1) * np.arange(40, dtype=np.float32)
    dem[2, 1] = -50
    carved, source, pits, lowered = carve_ref(dem, oracle_forest(dem))
    assert pits == 1 and lowered == 38
    want = dem.copy()
    want[2, 1:] = -50                                   # the outlet on the ring is lowered too
    assert same_bytes(carved, want)
    assert np.all(source[2, 2:] == 2 * 40 + 1) and (source != NOWHERE).sum() == 38


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd import upextreme
    from hydrodem_amd.filters import custom_filters
    assert hd.UpstreamExtreme is custom_filters.UpstreamExtreme
    assert hd.BreachDepressions is custom_filters.BreachDepressions
    assert issubclass(hd.UpstreamExtreme, hd.Filter)
    assert issubclass(hd.BreachDepressions, hd.ComposedFilter)
    assert hd.UpstreamExtreme.auto_device is True
    assert {"upextreme", "upextreme_dev", "breach", "breach_dev"} <= set(dir(upextreme))
    v = np.ones((4, 4), np.float32)
    f = hd.UpstreamExtreme(v)
    assert f.mode == "max" and f.output == "extreme" and f.values is v
    assert f.dtype == np.float32 and f.stats == {}
    assert hd.UpstreamExtreme(v, "min", "where").dtype == np.uint32
    assert hd.UpstreamExtreme(v.astype(np.uint32)).dtype == np.uint32
    b = hd.BreachDepressions()
    assert b.keep_partial_results is False and b.stats == {}
    assert b.filled is None and b.codes is None and b.source is None
    assert hd.BreachDepressions(keep_partial_results=True).keep_partial_results is True
    # the conditioning chain is what it was
    chain = hd.HydroConditioning()
    assert chain.flats == "keep" and chain.filters[0].epsilon == 0.0


def test_the_operators_resolve_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import UpstreamExtreme, BreachDepressions
        import hydrodem_amd
        assert UpstreamExtreme is hydrodem_amd.UpstreamExtreme
        assert BreachDepressions is hydrodem_amd.BreachDepressions
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operators_reject_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend, upextreme

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    v = np.ones((4, 4), np.float32)
    make = hd.UpstreamExtreme
    with pytest.raises(ValueError, match="needs the values"):
        make(None)
    with pytest.raises(ValueError, match="values is a NumPy array or a DeviceRaster"):
        make([[1.0]])
    with pytest.raises(ValueError, match="got float64"):
        make(v.astype(np.float64))                              # refused, not narrowed
    with pytest.raises(ValueError, match="got uint8"):
        make(v.astype(np.uint8))
    with pytest.raises(ValueError, match="values is a 2-D raster"):
        make(np.ones(4, np.float32))
    for bad in ("mean", 0, None, ("min",)):
        with pytest.raises(ValueError, match="mode is one of"):
            make(v, mode=bad)
    for bad in ("index", ("extreme", "where"), None):
        with pytest.raises(ValueError, match="output is one of"):
            make(v, output=bad)

    f = make(v)
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    ctx = backend.Context.__new__(backend.Context)             # a context that is never used
    ctx.lib, ctx.handle, ctx.device = None, ctypes.c_void_p(1), 0

    def wrap_device(a):
        return backend.DeviceRaster.wrap(0x10000, a.shape, a.dtype, ctx=ctx)
    for form, wrap in (("apply", lambda a: a), ("apply_device", wrap_device)):
        run = getattr(f, form)
        with pytest.raises(ValueError, match="uint8 D8 codes, got float32"):
            run(wrap(np.zeros((4, 4), np.float32)))
        with pytest.raises(ValueError, match="a 2-D raster, got 3 dimensions"):
            run(wrap(np.zeros((2, 4, 4), np.uint8)))
        with pytest.raises(ValueError, match=r"the values are \(4, 4\), the codes \(4, 5\)"):
            run(wrap(np.zeros((4, 5), np.uint8)))
        g = make(v)
        g.mode = "least"                                       # a mutable operand attribute
        with pytest.raises(ValueError, match="mode is one of"):
            getattr(g, form)(wrap(codes))
        breach = getattr(hd.BreachDepressions(), form)
        with pytest.raises(ValueError, match="a float32 DEM, got float64"):
            breach(wrap(np.zeros((4, 4), np.float64)))
        with pytest.raises(ValueError, match="a 2-D raster, got 3 dimensions"):
            breach(wrap(np.zeros((2, 4, 4), np.float32)))
    with pytest.raises(ValueError, match="unknown upstream extreme outputs"):
        upextreme.upextreme(codes, v, want=("extreme", "index"))
    with pytest.raises(ValueError, match="no output wanted"):
        upextreme.upextreme(codes, v, want=())
    with pytest.raises(ValueError, match="codes is a NumPy array"):
        upextreme.upextreme([[1]], v)
    with pytest.raises(ValueError, match="values is a NumPy array"):
        upextreme.upextreme(codes, [[1.0]])
    assert upextreme.upextreme_args(codes, v, "min", ("where", "extreme")) == \
        (1, 0, ("extreme", "where"))
    assert upextreme.upextreme_args(codes, v.astype(np.uint32), "max", "where") == \
        (2, 1, ("where",))
    with pytest.raises(ValueError, match="a float32 DEM, got uint8"):
        upextreme.breach(codes, codes)
    with pytest.raises(ValueError, match="uint8 D8 codes, got float32"):
        upextreme.breach(v, v)
    with pytest.raises(ValueError, match=r"the codes are \(4, 5\), the DEM \(4, 4\)"):
        upextreme.breach(v, np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="unknown depression breaching outputs"):
        upextreme.breach(v, codes, want=("carved", "pits"))
    assert upextreme.breach_args(v, codes, "source") == ("carved", "source")
    assert upextreme.breach_args(v, codes, ()) == ("carved",)


# ---------------------------------------------------------------------------
# the header and the library
# ---------------------------------------------------------------------------
NAMES = ("hdem_upextreme_u8", "hdem_upextreme_u8_dev", "hdem_breach_f32", "hdem_breach_f32_dev")


def test_the_header_declares_the_entry_points():
    from hydrodem_amd import backend, upextreme
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"hdem_upextreme_u8": ["hdem_ctx *ctx", "const uint8_t *d8", "int H", "int W",
                                  "const void *values", "int value_type", "int mode",
                                  "void *extreme", "uint32_t *where",
                                  "hdem_upextreme_stats *stats"],
            "hdem_breach_f32": ["hdem_ctx *ctx", "const float *dem", "const uint8_t *d8",
                                "int H", "int W", "float *carved", "uint32_t *source",
                                "hdem_breach_stats *stats"]}
    for name in NAMES:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", plain)
        assert proto, name
        args = [" ".join(a.split()) for a in proto.group(1).split(",")]
        assert args == want[name[:-4] if name.endswith("_dev") else name]
        assert len(backend.SIGNATURES[name]) == len(args)
    assert backend.SIGNATURES["hdem_upextreme_u8"] == backend.SIGNATURES["hdem_upextreme_u8_dev"]
    assert backend.SIGNATURES["hdem_breach_f32"] == backend.SIGNATURES["hdem_breach_f32_dev"]
    consts = {k: int(v) for k, v in re.findall(r"\b(HDEM_UPEXT_[A-Z0-9]+)\s*=\s*(\d+)", header)}
    assert consts == {"HDEM_UPEXT_F32": 1, "HDEM_UPEXT_U32": 2, "HDEM_UPEXT_MIN": 0,
                      "HDEM_UPEXT_MAX": 1}
    assert upextreme.VALUE_TYPES == {np.dtype(np.float32): 1, np.dtype(np.uint32): 2}
    assert upextreme.MODES == {"min": 0, "max": 1}
    assert "A17" in header and "A18" in header
    # the structs, their sizeof notes, and no kernel id of their own
    assert re.search(r"\}\s*hdem_upextreme_stats;\s*/\* sizeof == 48 \*/", header)
    assert re.search(r"\}\s*hdem_breach_stats;\s*/\* sizeof == 64 \*/", header)
    enums = dict(re.findall(r"\b(HDEM_K_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert int(enums["HDEM_K_COUNT"]) == 21 and "HDEM_K_UPEXT" not in header
    stats = backend._UpExtremeStats                  # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 48 and stats().struct_size == 48
    assert stats.exits.offset == 8 and stats.absent.offset == 16 and stats.ms_tile.offset == 32
    assert set(stats().as_dict()) == {"max_hops", "exits", "absent", "tile_h", "tile_w",
                                      "ms_tile", "ms_forest", "ms_final"}
    stats = backend._BreachStats                     # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 64 and stats().struct_size == 64
    assert stats.absent.offset == 16 and stats.pits.offset == 48 and stats.lowered.offset == 56
    assert set(stats().as_dict()) == {"max_hops", "exits", "absent", "tile_h", "tile_w", "ms_tile",
                                      "ms_forest", "ms_final", "pits", "lowered"}
    # the weighted ABI is what it was
    assert ctypes.sizeof(backend._FlowSumStats) == 48    # pylint: disable=protected-access
    assert len(backend.SIGNATURES["hdem_flowsum_u8"]) == 12


def test_the_library_exports_the_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    for name in NAMES + ("hdem_flowsum_u8", "hdem_flowacc_u8"):
        assert hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile")).read()
    assert "hdem_upextreme.hip" in makefile
    # the argument checks that come before the context is used: a null context first
    lib = backend.load_library()
    for name in NAMES:
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
