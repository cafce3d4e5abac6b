"""
Strahler stream order, Shreve magnitude and stream links (``StreamOrder``,
``hdem_streamorder_u8``): the CPU half.

``S`` is the stream set; a stream donor of ``c`` is a neighbour in ``S`` whose code points at
``c``.  Off the streams everything is 0.  On them ``order`` is 1 without a stream donor, else
``m + 1`` when two or more stream donors have the greatest order ``m`` and ``m`` otherwise;
``magnitude`` is 1 without a stream donor, else the donors' sum; ``link`` is 1 + the flat
index of the first cell on the path that is terminal, or whose receiver is off the streams, or
whose receiver has two or more stream donors.

The host references live here and are used by tests/test_gpu_streamorder.py, none of them
knows about links when it works out orders:
  ``order_kahn``   NumPy Kahn peeling of the stream cells, one frontier at a time;
  ``order_brute``  the plain recursion, cell by cell -- tiny grids;
  ``link_ends``    the link raster by pointer doubling;
  ``order_holds``  the local equations at every cell, row band by row band -- any size.  For
                   acyclic codes their solution is unique, so it alone proves a result exact.
No GPU here: the references agree with each other and tell a wrong rule from the right one,
the operators are importable from the package and the drop-in ``filters``, reject what they
must without a device, and the library exports its entry points.
"""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_flowacc import CODE_OFFSETS, acc_kahn, random_acyclic_codes, receivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def stream_of(codes, streams=None, threshold=None):
    """The stream set as a bool raster, from the operator's three forms."""
    shape = np.shape(codes)
    if streams is None:
        return np.ones(shape, bool)
    streams = np.asarray(streams)
    return streams >= threshold if threshold is not None else streams != 0


def order_kahn(codes, stream, count_all=False):
    """Peel the stream cells whose stream donors are all done, one frontier at a time:
    (order, magnitude) as int64 rasters.  ``count_all``: the wrong rule, which counts every
    donor and not only those of the greatest order."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool).ravel()
    rec = receivers(codes)
    n = rec.size
    rec = np.where(stream & (rec >= 0) & stream[np.maximum(rec, 0)], rec, -1)   # stream edges
    indeg = np.bincount(rec[rec >= 0], minlength=n)
    order, mag = np.zeros(n, np.int64), np.zeros(n, np.int64)
    hi, cnt, arriving = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    frontier = np.flatnonzero(stream & (indeg == 0))
    order[frontier], mag[frontier] = 1, 1
    done = 0
    while frontier.size:
        done += frontier.size
        r = rec[frontier]
        keep = r >= 0
        f, r = frontier[keep], r[keep]
        arriving[r] = 0
        np.maximum.at(arriving, r, order[f])
        raised = np.unique(r[arriving[r] > hi[r]])
        hi[raised] = arriving[raised]
        if not count_all:
            cnt[raised] = 0
        np.add.at(cnt, r, 1 if count_all else (order[f] == hi[r]).astype(np.int64))
        np.add.at(mag, r, mag[f])
        np.subtract.at(indeg, r, 1)
        cand = np.unique(r)
        frontier = cand[indeg[cand] == 0]
        order[frontier] = hi[frontier] + (cnt[frontier] >= 2)
    if done != int(stream.sum()):
        raise ValueError(f"flow directions form a cycle: {int(stream.sum()) - done} stream "
                         "cells never drain")
    return order.reshape(codes.shape), mag.reshape(codes.shape)


def order_brute(codes, stream):
    """The definition, recursively, in Python integers; a cycle is a ValueError."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool).ravel().tolist()
    rec = receivers(codes).tolist()
    n = len(rec)
    donors = [[] for _ in range(n)]
    for d, c in enumerate(rec):
        if c >= 0 and stream[d] and stream[c]:
            donors[c].append(d)
    memo, open_ = {}, set()

    def solve(c):
        if c in memo:
            return memo[c]
        if c in open_:
            raise ValueError("flow directions form a cycle")
        open_.add(c)
        got = [solve(d) for d in donors[c]]
        open_.discard(c)
        if not got:
            memo[c] = (1, 1)
        else:
            m = max(o for o, _ in got)
            memo[c] = (m + (sum(o == m for o, _ in got) >= 2), sum(g for _, g in got))
        return memo[c]

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 100))
    try:
        res = [solve(c) if stream[c] else (0, 0) for c in range(n)]
    finally:
        sys.setrecursionlimit(limit)
    return (np.array([o for o, _ in res], np.int64).reshape(codes.shape),
            np.array([g for _, g in res], np.int64).reshape(codes.shape))


def stream_donors(codes, stream):
    """nin: the number of stream donors of every cell (int64 raster)."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool)
    rec = receivers(codes)
    gives = stream.ravel() & (rec >= 0)
    return np.bincount(rec[gives], minlength=rec.size).reshape(codes.shape)


def link_stops(codes, stream):
    """Bool raster: the last cell of every link."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool)
    rec = receivers(codes)
    nin = stream_donors(codes, stream).ravel()
    to = np.maximum(rec, 0)
    stop = stream.ravel() & ((rec < 0) | ~stream.ravel()[to] | (nin[to] >= 2))
    return stop.reshape(codes.shape)


def link_ends(codes, stream):
    """The link raster: every stream cell follows its path to the first stop, by pointer
    doubling (a stream cell that is no stop has its receiver on the streams)."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool)
    stop = link_stops(codes, stream).ravel()
    rec = receivers(codes)
    at = np.arange(rec.size)
    nxt = np.where(stream.ravel() & ~stop, rec, at)
    for _ in range(max(1, int(rec.size).bit_length() + 1)):
        nxt = nxt[nxt]
    if (stream.ravel() & ~stop[nxt]).any():
        raise ValueError("flow directions form a cycle")
    return np.where(stream.ravel(), nxt + 1, 0).reshape(codes.shape)


def order_holds(codes, stream, order, magnitude, link, band=1024, count_all=False):
    """The local equations at every cell: order and magnitude from the stream donors' (0 off
    the streams), ``link == own index + 1`` at a stop and the receiver's elsewhere.
    ``count_all``: the equations of the wrong rule of ``order_kahn``."""
    codes = np.asarray(codes, dtype=np.uint8)
    stream = np.asarray(stream, bool)
    h, w = codes.shape
    if any(np.shape(a) != codes.shape for a in (stream, order, magnitude, link)):
        return False
    order, magnitude = np.asarray(order, np.int64), np.asarray(magnitude, np.int64)
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        shape = (r1 - r0, w)
        nin, top, cnt, total = (np.zeros(shape, np.int64) for _ in range(4))
        for counting in (False, True):
            for code, (dy, dx) in CODE_OFFSETS:
                # donors at rows y with y + dy in [r0, r1), columns with x + dx inside
                y0, y1 = max(0, r0 - dy), min(h, r1 - dy)
                x0, x1 = max(0, -dx), min(w, w - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                gives = (codes[y0:y1, x0:x1] == code) & stream[y0:y1, x0:x1]
                to = (slice(y0 + dy - r0, y1 + dy - r0), slice(x0 + dx, x1 + dx))
                o = np.where(gives, order[y0:y1, x0:x1], 0)
                if not counting:
                    nin[to] += gives
                    top[to] = np.maximum(top[to], o)
                    total[to] += np.where(gives, magnitude[y0:y1, x0:x1], 0)
                else:
                    cnt[to] += gives & (count_all | (o == top[to]))
        s = stream[r0:r1]
        want_o = np.where(s, np.where(nin == 0, 1, top + (cnt >= 2)), 0)
        want_m = np.where(s, np.where(nin == 0, 1, total), 0)
        if not (np.array_equal(want_o, order[r0:r1]) and np.array_equal(want_m, magnitude[r0:r1])):
            return False
    stop = link_stops(codes, stream).ravel()
    rec = receivers(codes)
    flat = np.asarray(link, np.int64).ravel()
    want = np.where(stop, np.arange(rec.size) + 1, flat[np.maximum(rec, 0)])
    return bool(np.array_equal(np.where(stream.ravel(), want, 0), flat))


# ---------------------------------------------------------------------------
# constructed networks (also used on the GPU)
# ---------------------------------------------------------------------------
def comb(n=300):
    """3 x n: row 1 flows east, rows 0 and 2 flow into it."""
    codes = np.empty((3, n), np.uint8)
    codes[0], codes[1], codes[2] = S, E, N
    return codes


def binary_tree(shape=(160, 256), levels=6, row=30, col=40):
    """A perfect binary tree of 2^levels leaves on ``row`` at columns col, col + 2, ...: at
    level j each pair runs 2^(j-1) steps SE and SW to its meeting cell.  Codes, the tree as a
    mask, and the root."""
    codes = np.zeros(shape, np.uint8)
    mask = np.zeros(shape, bool)
    nodes = [(row, col + 2 * k) for k in range(2 ** levels)]
    for j in range(1, levels + 1):
        step = 2 ** (j - 1)
        merged = []
        for (ay, ax), (by, bx) in zip(nodes[0::2], nodes[1::2]):
            for s in range(step):
                codes[ay + s, ax + s], codes[by + s, bx - s] = SE, SW
                mask[ay + s, ax + s] = mask[by + s, bx - s] = True
            assert (ay + step, ax + step) == (by + step, bx - step)
            merged.append((ay + step, ax + step))
        nodes = merged
    mask[nodes[0]] = True
    return codes, mask, nodes[0]


def star():
    codes = np.array([[SE, S, SW], [E, 0, W_], [NE, N, NW]], np.uint8)
    return codes


def triple(third):
    """A 9 x 9 raster whose centre (4, 4) has three donors: two of order 2 from the NW and the
    NE, and a third from the N (``third == 2``) or, of order 3, from the S (``third == 3``)."""
    codes = np.zeros((9, 9), np.uint8)
    r, c = 4, 4
    codes[r - 1, c - 1], codes[r - 2, c - 2], codes[r - 1, c - 2] = SE, SE, E
    codes[r - 1, c + 1], codes[r - 2, c + 2], codes[r - 1, c + 2] = SW, SW, W_
    if third == 2:
        codes[r - 1, c], codes[r - 2, c], codes[r - 2, c - 1] = S, S, SE
    else:
        codes[r + 1, c] = N
        codes[r + 2, c - 1], codes[r + 2, c - 2], codes[r + 3, c - 2] = NE, E, NE
        codes[r + 2, c + 1], codes[r + 2, c + 2], codes[r + 3, c + 2] = NW, W_, NW
    return codes, (r, c)


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
def stream_sets(codes, seed):
    rng = np.random.default_rng(seed)
    yield "all", np.ones(codes.shape, bool)
    yield "acc", acc_kahn(codes) >= 4
    yield "mask", rng.random(codes.shape) < 0.6


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    for _, stream in stream_sets(codes, shape[1]):
        a = order_brute(codes, stream)
        b = order_kahn(codes, stream)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        link = link_ends(codes, stream)
        assert order_holds(codes, stream, *b, link, band=5)
        assert ((b[0] > 0) == stream).all() and ((link > 0) == stream).all()
        # the magnitude counts the heads upstream
        heads = stream & (stream_donors(codes, stream) == 0)
        assert int(b[1][_ends(codes, stream)].sum()) == heads.sum()
        # order and magnitude are constant on a link
        for raster in b:
            ends = (link - 1)[stream]
            assert np.array_equal(raster[stream], raster.ravel()[ends])
        if stream.any():
            at = np.unravel_index(np.flatnonzero(stream)[-1], codes.shape)
            for k in (0, 1, 2):
                wrong = [b[0].copy(), b[1].copy(), link.copy()]
                wrong[k][at] += 1
                assert not order_holds(codes, stream, *wrong, band=5)


def _ends(codes, stream):
    """Stream cells whose receiver is no stream cell: where the network's magnitudes leave."""
    rec = receivers(codes)
    flat = np.asarray(stream, bool).ravel()
    return (flat & ((rec < 0) | ~flat[np.maximum(rec, 0)])).reshape(np.shape(codes))


def test_the_comb_tells_the_rule_from_plus_one_at_every_junction():
    codes = comb()
    stream = np.ones(codes.shape, bool)
    order, mag = order_kahn(codes, stream)
    link = link_ends(codes, stream)
    assert (order[1] == 2).all() and (order[0] == 1).all() and (order[2] == 1).all()
    assert mag[1, 299] == 600 and np.array_equal(mag[1], 2 * np.arange(1, 301))
    assert np.array_equal(link.ravel(), np.arange(900) + 1)       # 900 links
    assert order_holds(codes, stream, order, mag, link)
    wrong, _ = order_kahn(codes, stream, count_all=True)
    assert np.array_equal(wrong[1], np.arange(2, 302))
    assert not order_holds(codes, stream, wrong, mag, link)
    # the wrong result solves the wrong equations, so the check is about the rule
    assert order_holds(codes, stream, wrong, mag, link, count_all=True)
    assert not order_holds(codes, stream, order, mag, link, count_all=True)


def test_the_star_the_triples_and_the_tree():
    codes = star()
    order, mag = order_kahn(codes, np.ones((3, 3), bool))
    assert (order[1, 1], mag[1, 1]) == (2, 8) and order.sum() == 10
    for third in (2, 3):
        codes, at = triple(third)
        for ref in (order_kahn, order_brute):
            order, mag = ref(codes, np.ones(codes.shape, bool))
            assert order[at] == 3 and mag[at] == (6 if third == 2 else 8)
            got = sorted(order[y, x] for y, x in [(3, 3), (3, 5), (3, 4) if third == 2 else (5, 4)])
            assert got == [2, 2, third]
    codes, mask, root = binary_tree()
    assert root == (93, 103)
    for stream in (mask, np.ones(codes.shape, bool)):
        order, mag = order_kahn(codes, stream)
        link = link_ends(codes, stream)
        assert (order[root], mag[root]) == (7, 64)
        assert order_holds(codes, stream, order, mag, link)
        assert [int(((order == k) & mask).sum()) for k in range(1, 8)] == [64] * 6 + [1]
        assert np.unique(link[mask]).size == 127
    nin = stream_donors(codes, mask)
    assert int((mask & (nin == 0)).sum()) == 64 and int((mask & (nin >= 2)).sum()) == 63
    # the tree crosses the tile seams at row 64 and columns 64 and 128
    assert mask[63:65].any(axis=1).all() and mask[:, 63:65].any(axis=0).all() and \
        mask[:, 127:129].any(axis=0).all()


def test_references_refuse_a_stream_loop():
    codes = np.zeros((6, 6), np.uint8)
    codes[2, 2], codes[2, 3], codes[3, 3], codes[3, 2] = E, S, W_, N
    codes[2, 1] = E
    stream = codes != 0
    for ref in (order_kahn, order_brute):
        with pytest.raises(ValueError, match="cycle"):
            ref(codes, stream)
    with pytest.raises(ValueError):
        order_kahn(np.array([[3]], np.uint8), np.ones((1, 1), bool))


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd import streamorder
    from hydrodem_amd.filters import custom_filters
    assert hd.StreamOrder is custom_filters.StreamOrder
    assert hd.DemToStreamOrder is custom_filters.DemToStreamOrder
    assert issubclass(hd.StreamOrder, hd.Filter) and issubclass(hd.DemToStreamOrder, hd.Filter)
    assert hd.StreamOrder.auto_device is True
    f = hd.StreamOrder()
    assert f.method == "strahler" and f.keep_partial_results is False and f.threshold is None
    assert f.stats == {} and f.order is None and f.magnitude is None and f.links is None
    with pytest.raises(TypeError):
        hd.StreamOrder(None, 100)                              # keyword-only
    assert {"streamorder_args", "streamorder", "streamorder_dev"} <= set(dir(streamorder))
    chain = hd.DemToStreamOrder(threshold=100)
    assert chain.method == "strahler" and chain.flats == "keep" and chain.stats == {}
    assert [type(m).__name__ for m in chain.filters] == ["SinkFill", "D8FlowDirection",
                                                         "FlowAccumulation"]
    assert chain.filters[0].epsilon == pytest.approx(1e-3)


def test_the_operators_resolve_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import StreamOrder, DemToStreamOrder
        import hydrodem_amd
        assert StreamOrder is hydrodem_amd.StreamOrder
        assert DemToStreamOrder is hydrodem_amd.DemToStreamOrder
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operators_reject_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend, streamorder

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    acc = np.ones((4, 4), np.uint32)
    f = hd.StreamOrder()
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    ctx = backend.Context.__new__(backend.Context)             # a context that is never used
    ctx.lib, ctx.handle, ctx.device = None, ctypes.c_void_p(1), 0
    for form, wrap in (("apply", lambda a: a),
                       ("apply_device",
                        lambda a: backend.DeviceRaster.wrap(0x10000, a.shape, a.dtype, ctx=ctx))):
        run = getattr(f, form)
        with pytest.raises(ValueError, match="uint8 D8 codes, got float32"):
            run(wrap(np.zeros((4, 4), np.float32)))
        with pytest.raises(ValueError, match="a 2-D raster, got 3 dimensions"):
            run(wrap(np.zeros((2, 4, 4), np.uint8)))
        with pytest.raises(ValueError, match="a 2-D raster, got 1 dimensions"):
            run(wrap(np.zeros(4, np.uint8)))
        with pytest.raises(ValueError, match=r"streams are \(3, 4\), the codes \(4, 4\)"):
            getattr(hd.StreamOrder(np.ones((3, 4), bool)), form)(wrap(codes))
        with pytest.raises(ValueError, match=r"streams are \(4, 5\), the codes \(4, 4\)"):
            getattr(hd.StreamOrder(np.ones((4, 5), np.uint32), threshold=2), form)(wrap(codes))
    with pytest.raises(ValueError, match="a threshold needs the uint32 raster"):
        hd.StreamOrder(threshold=5)
    with pytest.raises(ValueError, match="a uint8 stream mask takes no threshold"):
        hd.StreamOrder(np.ones((4, 4), bool), threshold=5)
    with pytest.raises(ValueError, match="a uint8 stream mask takes no threshold"):
        hd.StreamOrder(np.ones((4, 4), np.uint8), threshold=5)
    with pytest.raises(ValueError, match="a uint32 stream raster needs a threshold"):
        hd.StreamOrder(acc)
    for bad in (0, -3, 2.5, True, 2 ** 32):
        with pytest.raises(ValueError, match="threshold is an integer in 1"):
            hd.StreamOrder(acc, threshold=bad)
        with pytest.raises(ValueError, match="threshold is an integer in 1"):
            hd.DemToStreamOrder(threshold=bad)
        with pytest.raises(ValueError, match="threshold is an integer in 1"):
            streamorder.streamorder(codes, acc, bad)
    with pytest.raises(ValueError, match="streams has dtype bool or uint8 or uint32"):
        hd.StreamOrder(np.ones((4, 4), np.float32))
    with pytest.raises(ValueError, match="streams is a 2-D raster"):
        hd.StreamOrder(np.ones(4, np.uint8))
    for bad in ("horton", None, "Strahler"):
        with pytest.raises(ValueError, match="method is 'strahler' or 'shreve'"):
            hd.StreamOrder(method=bad)
        with pytest.raises(ValueError, match="method is 'strahler' or 'shreve'"):
            hd.DemToStreamOrder(threshold=10, method=bad)
        g = hd.StreamOrder()
        g.method = bad                                         # a mutable operand attribute
        with pytest.raises(ValueError, match="method is 'strahler' or 'shreve'"):
            g.apply(codes)
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve'"):
        hd.DemToStreamOrder(threshold=10, flats="fill")
    with pytest.raises(ValueError, match="a float32 DEM"):
        hd.DemToStreamOrder(threshold=10).apply(np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError, match="unknown stream order outputs"):
        streamorder.streamorder(codes, want=("order", "horton"))
    with pytest.raises(ValueError, match="no output wanted"):
        streamorder.streamorder(codes, want=())
    with pytest.raises(ValueError, match="codes is a NumPy array"):
        streamorder.streamorder([[1]])


def test_library_exports_the_streamorder_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_streamorder_u8") and hasattr(lib, "hdem_streamorder_u8_dev")
    assert backend.SIGNATURES["hdem_streamorder_u8"] == \
        backend.SIGNATURES["hdem_streamorder_u8_dev"]
    assert len(backend.SIGNATURES["hdem_streamorder_u8"]) == 12
    stats = backend._StreamOrderStats               # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 64
    assert stats().struct_size == 64
    assert stats.stream_cells.offset == 8 and stats.links.offset == 32
    assert stats.max_hops.offset == 40 and stats.ms_nodes.offset == 52
    assert set(stats().as_dict()) == {"max_order", "stream_cells", "heads", "junctions", "links",
                                      "max_hops", "tile_h", "tile_w", "ms_nodes", "ms_walk",
                                      "ms_gather"}
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    assert "HDEM_K_STREAMORDER" not in header and "sizeof == 64" in header


def test_null_context_calls_return_bad_arg(built):
    from hydrodem_amd import backend
    lib = backend.load_library()
    for name in ("hdem_streamorder_u8", "hdem_streamorder_u8_dev"):
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and b"ctx is null" in lib.hdem_last_error()
