"""
D8 flow trace (``FlowDistance``, ``HeightAboveDrainage``, ``DemToHAND``,
``hdem_flowtrace_u8``): the CPU half.

For every cell the trace gives ``stop`` (1 + flat index of the first stop on the cell's D8
path, the cell included; 0 when that stop is a terminal cell that is no stream cell) and
``ncard`` / ``ndiag``, the cardinal and diagonal steps to it.  A stop is a terminal cell or,
with streams, a stream cell.  The host references live here and are used by
tests/test_gpu_flowtrace.py:
  (a) ``trace_walk``      all cells step down their paths together -- tiny grids;
  (b) ``trace_doubling``  (ptr, nc, nd) <- (ptr[ptr], nc + nc[ptr], nd + nd[ptr]) on the flat
                          receiver array, ceil(log2 n) + 1 rounds, ``ValueError`` on a cycle;
  (c) ``trace_holds``     the local property, band by band, any size: a stop holds (own index
                          + 1, 0, 0) -- with streams a stream cell does, and a terminal cell
                          that is no stream cell holds (0, 0, 0) --, any other cell holds its
                          receiver's ``stop`` and its receiver's counts plus one in the count
                          its own code selects.  On acyclic codes that has one solution, so
                          (c) is a proof.
``distance_of`` and ``hand_of`` are the two NumPy formulas of the float rasters.  No GPU
here: the references agree with each other and with the watershed references, the operators
are importable from the package and the drop-in ``filters``, reject what they must without a
device, and the library exports its entry points.
"""
import ctypes
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_flowacc import (CODE_OFFSETS, acc_kahn, random_acyclic_codes, receivers,
                          terminal_mask)
from test_watersheds import labels_doubling, random_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)]
DIAGONAL = (2, 8, 32, 128)                               # SE, SW, NW, NE


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def _setup(codes, streams):
    """codes, flat receivers, stop cells, stream cells (None without streams), diagonal."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    stop = rec < 0
    stream = None
    if streams is not None:
        streams = np.asarray(streams)
        assert streams.shape == codes.shape
        stream = streams.ravel() != 0
        stop = stop | stream
    return codes, rec, stop, stream, np.isin(codes.ravel(), DIAGONAL)


def _rasters(shape, at, nc, nd, stream):
    stop = at + 1
    if stream is not None:
        stop[~stream[at]] = 0                            # ended in a dry terminal cell
    return tuple(a.astype(np.uint32).reshape(shape) for a in (stop, nc, nd))


def trace_walk(codes, streams=None):
    """(a): (stop, ncard, ndiag), all cells stepping together until each stands on a stop; a
    path longer than H*W cells is a cycle."""
    codes, rec, stop, stream, diag = _setup(codes, streams)
    n = rec.size
    pos = np.arange(n, dtype=np.int64)
    nc, nd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for _ in range(n + 1):
        moving = ~stop[pos]
        if not moving.any():
            return _rasters(codes.shape, pos, nc, nd, stream)
        nd[moving] += diag[pos[moving]]
        nc[moving] += ~diag[pos[moving]]
        pos[moving] = rec[pos[moving]]
    raise ValueError(f"flow directions form a cycle: {int(moving.sum())} cells never resolve")


def trace_doubling(codes, streams=None):
    """(b): pointer doubling with the two step counts as payload, a stop pointing at itself."""
    codes, rec, stop, stream, diag = _setup(codes, streams)
    n = rec.size
    ptr = np.where(stop, np.arange(n, dtype=np.int64), rec)
    nc = np.where(stop, 0, ~diag).astype(np.int64)
    nd = np.where(stop, 0, diag).astype(np.int64)
    for _ in range(math.ceil(math.log2(n)) + 1 if n > 1 else 1):
        nc, nd, ptr = nc + nc[ptr], nd + nd[ptr], ptr[ptr]
    lost = ~stop[ptr]
    if lost.any():
        raise ValueError(f"flow directions form a cycle: {int(lost.sum())} cells never resolve")
    return _rasters(codes.shape, ptr, nc, nd, stream)


def trace_holds(codes, stop, ncard, ndiag, streams=None, band=1024):
    """(c): every cell satisfies the local property.  ``streams``: a mask of the codes' shape
    (non-zero = stream) or None."""
    codes = np.asarray(codes, dtype=np.uint8)
    h, w = codes.shape
    if not (stop.shape == ncard.shape == ndiag.shape == codes.shape):
        return False
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        c = codes[r0:r1]
        # what each cell must hold; a cell that no case below touches is terminal
        own = (np.arange(r0, r1, dtype=np.int64)[:, None] * w
               + np.arange(w, dtype=np.int64)[None, :] + 1)
        want = [own.copy(), np.zeros(own.shape, np.int64), np.zeros(own.shape, np.int64)]
        has_receiver = np.zeros(own.shape, bool)
        for code, (dy, dx) in CODE_OFFSETS:
            y0, y1 = max(r0, -dy), min(r1, h - dy)       # rows whose receiver is inside
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            sel = c[y0 - r0:y1 - r0, x0:x1] == code
            step = (0, int(code not in DIAGONAL), int(code in DIAGONAL))
            for k, raster in enumerate((stop, ncard, ndiag)):
                tgt = raster[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                sub = want[k][y0 - r0:y1 - r0, x0:x1]
                sub[sel] = tgt[sel].astype(np.int64) + step[k]
            has_receiver[y0 - r0:y1 - r0, x0:x1] |= sel
        if streams is not None:
            stream = np.asarray(streams[r0:r1]) != 0
            want[0][~has_receiver & ~stream] = 0         # a dry terminal cell
            want[0][stream] = own[stream]
            want[1][stream] = 0
            want[2][stream] = 0
        for k, raster in enumerate((stop, ncard, ndiag)):
            if not np.array_equal(want[k], raster[r0:r1]):
                return False
    return True


def distance_of(stop, ncard, ndiag, cellsize=1.0):
    """The float32 distance raster of the C ABI's definition; NaN where unreached."""
    cs = float(cellsize)
    d = (ncard.astype(np.float64) * cs + ndiag.astype(np.float64) * (cs * np.sqrt(2.0)))
    d = d.astype(np.float32)
    d[stop == 0] = np.nan
    return d


def hand_of(stop, z):
    """``z - z[stop - 1]`` in float32; NaN where unreached."""
    z = np.asarray(z, dtype=np.float32)
    at = np.maximum(stop.astype(np.int64) - 1, 0)
    hand = z - z.ravel()[at]
    hand[stop == 0] = np.nan
    return hand.astype(np.float32)


def streams_of(codes, threshold=10):
    return acc_kahn(codes) >= threshold


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
def _same(a, b):
    return all(x.dtype == y.dtype == np.uint32 and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_references_agree_without_streams(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    a, b = trace_walk(codes), trace_doubling(codes)
    assert _same(a, b)
    stop, nc, nd = b
    term = terminal_mask(codes)
    assert stop.min() >= 1 and not nc[term].any() and not nd[term].any()
    assert ((nc + nd)[~term] >= 1).all()
    assert np.array_equal(stop, labels_doubling(codes))
    assert trace_holds(codes, *b, band=5)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_references_agree_with_streams(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    for streams in (streams_of(codes, 3), random_seeds(shape, seed=sum(shape), every=10) != 0):
        a, b = trace_walk(codes, streams), trace_doubling(codes, streams)
        assert _same(a, b)
        stop, nc, nd = b
        own = np.arange(codes.size).reshape(shape) + 1
        assert np.array_equal(stop[streams], own[streams])
        assert not nc[streams].any() and not nd[streams].any()
        dry = terminal_mask(codes) & ~streams
        assert not stop[dry].any() and not nc[dry].any() and not nd[dry].any()
        seeds = (own * streams).astype(np.uint32)
        assert np.array_equal(stop, labels_doubling(codes, seeds))
        assert trace_holds(codes, *b, streams=streams, band=5)
        # the counts of an unreached cell are those to its terminal cell
        free = trace_doubling(codes)
        assert np.array_equal(nc[stop == 0], free[1][stop == 0])
        assert np.array_equal(nd[stop == 0], free[2][stop == 0])


@pytest.mark.parametrize("shape", [(17, 23), (130, 257)])
def test_the_local_property_rejects_a_single_altered_cell_in_each_raster(shape):
    codes = random_acyclic_codes(*shape, seed=5, ramp=True)
    streams = streams_of(codes)
    for s in (None, streams):
        good = trace_doubling(codes, s)
        assert trace_holds(codes, *good, streams=s, band=7)
        reached = (good[0] != 0).mean()
        if s is not None and codes.size > 1000:
            assert 0.5 < reached < 1.0                   # both cases occur
        for k in range(3):
            for cell in (0, codes.size // 2, codes.size - 1):
                wrong = [r.copy() for r in good]
                wrong[k].flat[cell] += 1
                assert not trace_holds(codes, *wrong, streams=s, band=7)


def test_references_on_a_row_nested_streams_and_cycles():
    row = np.full((1, 50), 1, np.uint8)
    for fn in (trace_walk, trace_doubling):
        stop, nc, nd = fn(row)
        assert np.array_equal(stop[0], np.full(50, 50))
        assert np.array_equal(nc[0], np.arange(49, -1, -1)) and not nd.any()
    streams = np.zeros((1, 50), bool)
    streams[0, 10] = streams[0, 30] = True               # nested: upstream takes the upper
    for fn in (trace_walk, trace_doubling):
        stop, nc, nd = fn(row, streams)
        assert np.array_equal(stop[0], [11] * 11 + [31] * 20 + [0] * 19)
        assert np.array_equal(nc[0], list(range(10, -1, -1)) + list(range(19, -1, -1))
                              + list(range(18, -1, -1)))
    diag = np.full((6, 6), 2, np.uint8)                  # SE everywhere
    stop, nc, nd = trace_doubling(diag)
    assert not nc.any() and np.array_equal(np.diag(nd), [5, 4, 3, 2, 1, 0])
    d = distance_of(stop, nc, nd, 30.0)
    assert d.dtype == np.float32 and d[0, 0] == np.float32(5 * (30.0 * np.sqrt(2.0)))
    pair = np.array([[1, 16, 16]], np.uint8)             # E then W: a 2-cycle and a donor
    with pytest.raises(ValueError, match="3 cells never resolve"):
        trace_doubling(pair)
    with pytest.raises(ValueError, match="cycle"):
        trace_walk(pair)
    # a loop that holds a stream cell ends there
    streams = np.array([[0, 1, 0]], np.uint8)
    for fn in (trace_walk, trace_doubling):
        stop, nc, nd = fn(pair, streams)
        assert np.array_equal(stop, [[2, 2, 2]]) and np.array_equal(nc, [[1, 0, 1]])


def test_the_float_formulas():
    stop = np.array([[1, 0, 3]], np.uint32)
    z = np.array([[5.0, 7.0, np.nan]], np.float32)
    hand = hand_of(stop, z)
    assert hand.dtype == np.float32
    assert hand[0, 0] == 0 and np.isnan(hand[0, 1]) and np.isnan(hand[0, 2])
    d = distance_of(stop, np.array([[3, 1, 0]], np.uint32), np.array([[2, 1, 0]], np.uint32))
    assert d[0, 0] == np.float32(3.0 + 2.0 * np.sqrt(2.0)) and np.isnan(d[0, 1]) and d[0, 2] == 0


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd.filters import custom_filters
    for name in ("FlowDistance", "HeightAboveDrainage", "DemToHAND"):
        cls = getattr(hd, name)
        assert cls is getattr(custom_filters, name)
        assert issubclass(cls, hd.Filter)
    assert hd.FlowDistance.auto_device is True and hd.HeightAboveDrainage.auto_device is True
    assert issubclass(hd.DemToHAND, hd.ComposedFilter)
    f = hd.FlowDistance()
    assert f.streams is None and f.threshold is None and f.cellsize == 1.0 and f.stats == {}
    g = hd.HeightAboveDrainage(dem=np.zeros((2, 2), np.float32), streams=np.ones((2, 2), bool))
    assert g.distance is None and g.drainage is None and g.stats == {}
    assert g.streams.dtype == np.uint8                   # a bool mask goes as bytes
    d = hd.DemToHAND(threshold=100)
    assert [type(m).__name__ for m in d.filters] == ["SinkFill", "D8FlowDirection",
                                                     "FlowAccumulation"]
    assert d.filters[0].epsilon == 1e-3 and d.stats == {}
    assert d.filled is None and d.codes is None and d.accumulation is None
    assert d.distance is None


def test_the_operators_resolve_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import FlowDistance, HeightAboveDrainage, DemToHAND
        import hydrodem_amd
        assert FlowDistance is hydrodem_amd.FlowDistance
        assert HeightAboveDrainage is hydrodem_amd.HeightAboveDrainage
        assert DemToHAND is hydrodem_amd.DemToHAND
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operators_reject_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    mask = np.zeros((4, 4), np.uint8)
    acc = np.ones((4, 4), np.uint32)
    dem = np.zeros((4, 4), np.float32)
    # the codes
    for f in (hd.FlowDistance(), hd.FlowDistance(mask),
              hd.HeightAboveDrainage(dem=dem, streams=mask)):
        with pytest.raises(hd.NumpyArrayExpectedError):
            f.apply([[1, 2], [4, 8]])
        with pytest.raises(ValueError, match="uint8"):
            f.apply(np.zeros((4, 4), np.float32))
        with pytest.raises(ValueError, match="2-D"):
            f.apply(np.zeros((2, 4, 4), np.uint8))
    # the streams
    with pytest.raises(ValueError, match="NumPy array or a DeviceRaster"):
        hd.FlowDistance([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowDistance(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowDistance(np.zeros((4, 4), np.float32), threshold=1)
    with pytest.raises(ValueError, match="2-D"):
        hd.FlowDistance(np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match=r"streams are \(3, 4\)"):
        hd.FlowDistance(np.zeros((3, 4), np.uint8)).apply(codes)
    with pytest.raises(ValueError, match=r"streams are \(3, 4\)"):
        hd.FlowDistance(np.ones((3, 4), np.uint32), threshold=1).apply(codes)
    # the threshold
    with pytest.raises(ValueError, match="needs a threshold"):
        hd.FlowDistance(acc)
    with pytest.raises(ValueError, match="takes no threshold"):
        hd.FlowDistance(mask, threshold=1)
    with pytest.raises(ValueError, match="takes no threshold"):
        hd.FlowDistance(mask != 0, threshold=1)
    with pytest.raises(ValueError, match="threshold needs"):
        hd.FlowDistance(threshold=1)
    for bad in (0, -1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="threshold is an integer"):
            hd.FlowDistance(acc, threshold=bad)
    # the cell size
    for bad in (0, -30.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="cellsize"):
            hd.FlowDistance(cellsize=bad)
        with pytest.raises(ValueError, match="cellsize"):
            hd.DemToHAND(threshold=10, cellsize=bad)
    # HAND: the dem
    with pytest.raises(TypeError):
        hd.HeightAboveDrainage(streams=mask)             # keyword-only and required
    with pytest.raises(ValueError, match="needs the dem"):
        hd.HeightAboveDrainage(dem=None, streams=mask)
    with pytest.raises(ValueError, match="needs streams"):
        hd.HeightAboveDrainage(dem=dem, streams=None)
    with pytest.raises(ValueError, match="NumPy array or a DeviceRaster"):
        hd.HeightAboveDrainage(dem=[[0.0]], streams=mask)
    with pytest.raises(ValueError, match="float32"):
        hd.HeightAboveDrainage(dem=dem.astype(np.float64), streams=mask)
    with pytest.raises(ValueError, match=r"dem is \(4, 5\)"):
        hd.HeightAboveDrainage(dem=np.zeros((4, 5), np.float32), streams=mask).apply(codes)
    # the chain
    with pytest.raises(ValueError, match="threshold is an integer"):
        hd.DemToHAND(threshold=0)
    with pytest.raises(ValueError, match="needs a threshold"):
        hd.DemToHAND(threshold=None)
    chain = hd.DemToHAND(threshold=10)
    with pytest.raises(hd.NumpyArrayExpectedError):
        chain.apply([[1.0]])
    with pytest.raises(ValueError, match="float32"):
        chain.apply(np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError, match="2-D"):
        chain.apply(np.zeros(4, np.float32))
    # the backend's own checks come before the device too
    with pytest.raises(ValueError, match="uint8 D8 codes"):
        backend.flowtrace(codes.astype(np.int32))
    with pytest.raises(ValueError, match="NumPy array"):
        backend.flowtrace([[1]])
    with pytest.raises(ValueError, match="unknown flow trace outputs"):
        backend.flowtrace(codes, want=("length",))
    with pytest.raises(ValueError, match="no output wanted"):
        backend.flowtrace(codes, want=())
    with pytest.raises(ValueError, match="hand needs the dem"):
        backend.flowtrace(codes, mask, want=("hand",))
    with pytest.raises(ValueError, match="needs a threshold"):
        backend.flowtrace(codes, acc)


def test_library_exports_the_flowtrace_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_flowtrace_u8") and hasattr(lib, "hdem_flowtrace_u8_dev")
    assert {"hdem_flowtrace_u8", "hdem_flowtrace_u8_dev"} <= set(backend.SIGNATURES)
    assert backend.SIGNATURES["hdem_flowtrace_u8"] == backend.SIGNATURES["hdem_flowtrace_u8_dev"]
    assert len(backend.SIGNATURES["hdem_flowtrace_u8"]) == 16
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    enums = dict(re.findall(r"\b(HDEM_K_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert int(enums["HDEM_K_COUNT"]) == 21              # the call has no kernel id
    written = re.search(r"\}\s*hdem_flowtrace_stats;\s*/\*\s*sizeof == (\d+)\s*\*/", header)
    assert written and ctypes.sizeof(backend.FlowTraceStats) == int(written.group(1))
    assert backend.FlowTraceStats.struct_size.offset == 0
    assert backend.FlowTraceStats().struct_size == ctypes.sizeof(backend.FlowTraceStats)
    for name in ("forest_rounds", "stops", "unreached", "exits", "tile_h", "tile_w", "ms_tile",
                 "ms_forest", "ms_final"):
        assert hasattr(backend.FlowTraceStats, name)
    kinds = {m.group(1): int(m.group(2))
             for m in re.finditer(r"#define HDEM_FT_STREAMS_([A-Z0-9_]+) (\d+)", header)}
    assert kinds == {"NONE": backend.FT_STREAMS_NONE, "MASK_U8": backend.FT_STREAMS_MASK_U8,
                     "ACC_U32": backend.FT_STREAMS_ACC_U32}
