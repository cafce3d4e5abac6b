"""
The stream network as a table (``StreamNetwork``, ``hdem_streamlinks_u8``): the CPU half.

``S`` is the stream set, stream donors, ``nin``, links and link ends are those of
tests/test_streamorder.py.  The links are numbered in ascending flat index of their end cell;
row ``r`` of every column describes link ``r`` (include/hydrodem_hip.h A12).

The host references live here and are used by tests/test_gpu_streamnet.py; neither knows
anything of tiles:
  ``table_brute``  walks cell by cell in Python integers -- tiny grids;
  ``table_np``     NumPy grouping over ``link_ends``, plus a pointer-chasing first stream cell.
No GPU here: the references agree with each other, keep the invariants of the definitions,
give the known tables of constructed networks and tell a wrong rule from the right one; the
operators are importable from the package and the drop-in ``filters``, reject what they must
without a device, and the library exports its entry points.
"""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_flowacc import acc_kahn, random_acyclic_codes, receivers
from test_streamorder import (binary_tree, comb, link_ends, order_brute, order_kahn, star,
                              stream_donors, stream_sets, triple)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
NONE = 0xFFFFFFFF
COLUMNS = (("end", np.uint32), ("top", np.uint32), ("down", np.uint32), ("order", np.uint8),
           ("magnitude", np.uint32), ("cells", np.uint32), ("ncard", np.uint32),
           ("ndiag", np.uint32), ("length", np.float32), ("catchment", np.uint32),
           ("z_top", np.float32), ("z_end", np.float32))
COUNTERS = ("links", "stream_cells", "catchment_cells", "tops")


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def first_stream_cell(codes, stream):
    """1 + the flat index of the first stream cell on every cell's D8 path (the cell itself
    included), 0 where the path meets none: pointer doubling."""
    rec = receivers(codes)
    s = np.asarray(stream, bool).ravel()
    at = np.arange(rec.size)
    nxt = np.where(s | (rec < 0), at, rec)
    for _ in range(max(1, int(rec.size).bit_length() + 1)):
        nxt = nxt[nxt]
    return np.where(s[nxt], nxt + 1, 0)


def _length(ncard, ndiag, cellsize):
    return (np.asarray(ncard, np.float64) * cellsize +
            np.asarray(ndiag, np.float64) * (cellsize * np.sqrt(2.0))).astype(np.float32)


def _typed(table, dem):
    return {name: np.asarray(table[name]).astype(dtype) for name, dtype in COLUMNS
            if dem is not None or not name.startswith("z_")}


def table_np(codes, stream, dem=None, cellsize=1.0, own_step=True):
    """The table, the ``row`` raster and the counters by NumPy grouping.  ``own_step=False``:
    the wrong rule, which leaves the end cell's own step out of ``ncard`` / ``ndiag``."""
    codes = np.asarray(codes, dtype=np.uint8)
    s = np.asarray(stream, bool).ravel()
    n = codes.size
    at = np.arange(n)
    rec = receivers(codes)
    to = np.maximum(rec, 0)
    link = link_ends(codes, stream).ravel()
    ends = np.flatnonzero(link == at + 1)
    k = ends.size
    row_of_end = np.full(n, -1, np.int64)
    row_of_end[ends] = np.arange(k)
    r = np.where(s, row_of_end[np.maximum(link - 1, 0)], -1)
    nin = stream_donors(codes, stream).ravel()
    tops = np.flatnonzero(s & (nin != 1))
    assert (np.bincount(r[tops], minlength=k) == 1).all(), "a link without its one top"
    top = np.zeros(k, np.int64)
    top[r[tops]] = tops
    to_stream = s & (rec >= 0) & s[to]
    down = np.where(to_stream[ends], r[to[ends]], NONE)
    diagonal = np.isin(codes.ravel(), (SE, SW, NW, NE))
    steps = to_stream & (own_step | (link != at + 1))
    ncard = np.bincount(r[steps & ~diagonal], minlength=k)
    ndiag = np.bincount(r[steps & diagonal], minlength=k)
    first = first_stream_cell(codes, stream)
    reached = first > 0
    order, magnitude = order_kahn(codes, stream)
    table = {"end": ends, "top": top, "down": down, "order": order.ravel()[ends],
             "magnitude": magnitude.ravel()[ends], "cells": np.bincount(r[s], minlength=k),
             "ncard": ncard, "ndiag": ndiag, "length": _length(ncard, ndiag, cellsize),
             "catchment": np.bincount(r[first[reached] - 1], minlength=k)}
    if dem is not None:
        flat = np.asarray(dem, np.float32).ravel()
        table["z_top"], table["z_end"] = flat[top], flat[ends]
    counters = {"links": k, "stream_cells": int(s.sum()), "catchment_cells": int(reached.sum()),
                "tops": int(tops.size)}
    return _typed(table, dem), (r + 1).astype(np.uint32).reshape(codes.shape), counters


def table_brute(codes, stream, dem=None, cellsize=1.0):
    """The definitions, cell by cell, in Python integers."""
    codes = np.asarray(codes, dtype=np.uint8)
    s = np.asarray(stream, bool).ravel().tolist()
    rec = receivers(codes).tolist()
    flat = codes.ravel().tolist()
    n = len(rec)
    nin = [0] * n
    for d, c in enumerate(rec):
        if c >= 0 and s[d]:
            nin[c] += 1

    def to_stream(c):
        return rec[c] >= 0 and s[rec[c]]

    def end_of(c):                                   # the first stop on c's path
        for _ in range(n + 1):
            if not to_stream(c) or nin[rec[c]] >= 2:
                return c
            c = rec[c]
        raise ValueError("flow directions form a cycle")

    end = [end_of(c) if s[c] else -1 for c in range(n)]
    ends = sorted(set(e for e in end if e >= 0))
    row = {e: k for k, e in enumerate(ends)}
    order, magnitude = order_brute(codes, stream)
    table = {name: [] for name, _ in COLUMNS}
    for e in ends:
        members = [c for c in range(n) if end[c] == e]
        tops = [c for c in members if nin[c] != 1]
        assert len(tops) == 1
        c, ncard, ndiag = tops[0], 0, 0
        while True:                                  # from the top to the end, then one more
            if c == e and not to_stream(c):
                break
            if flat[c] in (SE, SW, NW, NE):
                ndiag += 1
            else:
                ncard += 1
            if c == e:
                break
            c = rec[c]
        catchment = 0
        for c in range(n):
            for _ in range(n + 1):
                if s[c] or rec[c] < 0:
                    break
                c = rec[c]
            catchment += s[c] and end[c] == e
        table["end"].append(e)
        table["top"].append(tops[0])
        table["down"].append(row[end[rec[e]]] if to_stream(e) else NONE)
        table["order"].append(int(order.ravel()[e]))
        table["magnitude"].append(int(magnitude.ravel()[e]))
        table["cells"].append(len(members))
        table["ncard"].append(ncard)
        table["ndiag"].append(ndiag)
        table["catchment"].append(catchment)
        if dem is not None:
            table["z_top"].append(np.asarray(dem, np.float32).ravel()[tops[0]])
            table["z_end"].append(np.asarray(dem, np.float32).ravel()[e])
    table["length"] = _length(table["ncard"], table["ndiag"], cellsize)
    raster = np.array([row[e] + 1 if e >= 0 else 0 for e in end], np.uint32)
    return _typed(table, dem), raster.reshape(codes.shape)


def same_table(a, b):
    """Bit for bit, NaN included (the float columns are compared as their bytes)."""
    return set(a) == set(b) and all(
        a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
        a[k].tobytes() == b[k].tobytes() for k in a)


def accumulate_down(down, values):
    """``values`` of every link plus those of all links upstream of it."""
    down = np.asarray(down, np.int64)
    total = np.asarray(values, np.int64).copy()
    indeg = np.bincount(down[down != NONE], minlength=down.size)
    ready = list(np.flatnonzero(indeg == 0))
    while ready:
        r = ready.pop()
        d = down[r]
        if d != NONE:
            total[d] += total[r]
            indeg[d] -= 1
            if indeg[d] == 0:
                ready.append(d)
    return total


def lengths_add_up(codes, stream, table):
    """The steps counted cell by cell from every link's top down to where the network ends
    are the sum of ``ncard`` / ``ndiag`` over the links along ``down``."""
    codes = np.asarray(codes, dtype=np.uint8)
    s = np.asarray(stream, bool).ravel()
    rec = receivers(codes)
    to_stream = s & (rec >= 0) & s[np.maximum(rec, 0)]
    diagonal = np.isin(codes.ravel(), (SE, SW, NW, NE))
    pos = table["top"].astype(np.int64)
    walked = np.zeros((2, pos.size), np.int64)
    alive = np.ones(pos.size, bool)
    for _ in range(codes.size + 1):
        alive &= to_stream[pos]
        if not alive.any():
            break
        walked[0] += alive & ~diagonal[pos]
        walked[1] += alive & diagonal[pos]
        pos = np.where(alive, rec[pos], pos)
    down = table["down"].astype(np.int64)
    summed = np.stack([table["ncard"], table["ndiag"]]).astype(np.int64)
    at = down.copy()
    for _ in range(pos.size + 1):
        on = at != NONE
        if not on.any():
            break
        summed[:, on] += np.stack([table["ncard"], table["ndiag"]]).astype(np.int64)[:, at[on]]
        at[on] = down[at[on]]
    return bool(np.array_equal(walked, summed))


def invariants_hold(codes, stream, table, counters):
    down_is_link = table["down"] != NONE
    return bool(
        int(table["cells"].sum()) == counters["stream_cells"] == int(np.sum(stream)) and
        counters["links"] == counters["tops"] == table["end"].size and
        np.array_equal(table["ncard"].astype(np.int64) + table["ndiag"],
                       table["cells"].astype(np.int64) - 1 + down_is_link) and
        int(table["catchment"].sum()) == counters["catchment_cells"] and
        (np.diff(table["end"].astype(np.int64)) > 0).all() and
        lengths_add_up(codes, stream, table))


def random_dem(shape, seed):
    rng = np.random.default_rng(seed)
    dem = rng.normal(100.0, 30.0, shape).astype(np.float32)
    dem[rng.random(shape) < 0.05] = np.nan
    return dem


# ---------------------------------------------------------------------------
# constructed networks (also used on the GPU)
# ---------------------------------------------------------------------------
def row_link(n=130):
    """1 x n flowing east: one link of n cells."""
    return np.full((1, n), E, np.uint8)


def serpentine(shape=(129, 200)):
    """Even rows flow east and odd rows west, the last cell of a row south: one link over the
    whole raster that crosses every tile seam many times."""
    h, w = shape
    codes = np.empty(shape, np.uint8)
    codes[0::2], codes[1::2] = E, W_
    codes[0:h - 1:2, w - 1] = S
    codes[1:h - 1:2, 0] = S
    return codes


def constructed():
    """(name, codes, stream) of every constructed network."""
    yield "comb", comb(), np.ones((3, 300), bool)
    yield "star", star(), np.ones((3, 3), bool)
    for third in (2, 3):
        codes, _ = triple(third)
        yield f"triple{third}", codes, codes != 0
        yield f"triple{third}-all", codes, np.ones(codes.shape, bool)
    codes, mask, _ = binary_tree()
    yield "tree", codes, mask
    yield "tree-all", codes, np.ones(codes.shape, bool)
    yield "row", row_link(), np.ones((1, 130), bool)
    yield "serpentine", serpentine(), np.ones((129, 200), bool)


def known_table(name):
    """What a constructed network's table must hold, column by column."""
    if name == "comb":
        x = np.arange(300)
        return {"end": np.arange(900), "top": np.arange(900),
                "down": np.concatenate([300 + x, np.append(301 + x[:-1], NONE), 300 + x]),
                "order": np.repeat([1, 2, 1], 300),
                "magnitude": np.concatenate([np.ones(300), 2 * (x + 1), np.ones(300)]),
                "cells": np.ones(900), "ncard": np.append(np.ones(599), 0).tolist() + [1] * 300,
                "ndiag": np.zeros(900), "catchment": np.ones(900)}
    if name == "star":
        return {"end": np.arange(9), "top": np.arange(9), "down": [4, 4, 4, 4, NONE, 4, 4, 4, 4],
                "order": [1, 1, 1, 1, 2, 1, 1, 1, 1], "magnitude": [1, 1, 1, 1, 8, 1, 1, 1, 1],
                "cells": np.ones(9), "ncard": [0, 1, 0, 1, 0, 1, 0, 1, 0],
                "ndiag": [1, 0, 1, 0, 0, 0, 1, 0, 1], "catchment": np.ones(9)}
    if name == "row":
        return {"end": [129], "top": [0], "down": [NONE], "order": [1], "magnitude": [1],
                "cells": [130], "ncard": [129], "ndiag": [0], "catchment": [130]}
    if name == "serpentine":
        return {"end": [25799], "top": [0], "down": [NONE], "order": [1], "magnitude": [1],
                "cells": [25800], "ncard": [25799], "ndiag": [0], "catchment": [25800]}
    raise KeyError(name)


def holds_known(name, table):
    """The known columns of ``name``; for the tree, what its construction says of the links."""
    if name == "tree":
        level = np.log2(table["cells"].astype(np.float64)).astype(np.int64) + 1
        root = table["down"] == NONE
        return bool(
            table["end"].size == 127 and root.sum() == 1 and
            sorted(np.bincount(table["cells"]).tolist()) == sorted([0, 65, 32, 0, 16] + [0] * 3 +
                                                                   [8] + [0] * 7 + [4] +
                                                                   [0] * 15 + [2]) and
            np.array_equal(table["order"][~root], level[~root]) and
            np.array_equal(table["magnitude"][~root], 2 ** (level[~root] - 1)) and
            (table["order"][root], table["magnitude"][root]) == (7, 64) and
            (table["ncard"] == 0).all() and
            np.array_equal(table["ndiag"][~root], table["cells"][~root]) and
            table["ndiag"][root] == 0 and np.array_equal(table["catchment"], table["cells"]))
    try:
        want = known_table(name)
    except KeyError:
        return True
    return all(np.array_equal(table[k].astype(np.int64), np.asarray(v, np.int64))
               for k, v in want.items())


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    dem = random_dem(shape, shape[1])
    acc = acc_kahn(codes)
    for kind, stream in stream_sets(codes, shape[1]):
        table, raster, counters = table_np(codes, stream, dem, 2.5)
        brute, brute_raster = table_brute(codes, stream, dem, 2.5)
        assert same_table(table, brute) and np.array_equal(raster, brute_raster)
        assert invariants_hold(codes, stream, table, counters)
        assert ((raster > 0) == stream).all()
        assert np.array_equal(raster.ravel()[table["end"]], np.arange(table["end"].size) + 1)
        if kind != "mask":                           # S closed downstream
            total = accumulate_down(table["down"], table["catchment"])
            assert np.array_equal(total, acc.ravel()[table["end"]])
        if kind == "all":
            assert np.array_equal(table["catchment"], table["cells"])


def test_constructed_networks_have_their_known_tables():
    for name, codes, stream in constructed():
        table, raster, counters = table_np(codes, stream)
        assert holds_known(name, table), name
        assert invariants_hold(codes, stream, table, counters), name
        assert "z_top" not in table and raster.dtype == np.uint32
        if codes.size <= 100:
            brute, brute_raster = table_brute(codes, stream)
            assert same_table(table, brute) and np.array_equal(raster, brute_raster), name
    codes, at = triple(3)
    table, raster, _ = table_np(codes, np.ones(codes.shape, bool))
    centre = int(raster[at]) - 1
    assert table["order"][centre] == 3 and table["magnitude"][centre] == 8
    assert table["top"][centre] == at[0] * 9 + at[1] and (table["down"] == centre).sum() == 3
    # the serpentine crosses the seams at row 64 and 128 and at columns 64 and 128
    table, _, _ = table_np(serpentine(), np.ones((129, 200), bool), cellsize=30.0)
    assert table["length"][0] == np.float32(25799 * 30.0)


def test_a_rule_without_the_end_cells_own_step_fails_the_lengths():
    for name, codes, stream in constructed():
        right, _, counters = table_np(codes, stream)
        wrong, _, _ = table_np(codes, stream, own_step=False)
        assert lengths_add_up(codes, stream, right), name
        if (right["down"] != NONE).any():
            assert not lengths_add_up(codes, stream, wrong), name
            assert not invariants_hold(codes, stream, wrong, counters), name
        else:
            assert same_table(right, wrong), name
    codes = random_acyclic_codes(17, 23, seed=5)
    stream = acc_kahn(codes) >= 4
    assert lengths_add_up(codes, stream, table_np(codes, stream)[0])
    assert not lengths_add_up(codes, stream, table_np(codes, stream, own_step=False)[0])


def test_first_stream_cell_and_length_formula():
    codes = row_link(5)
    stream = np.array([[0, 0, 1, 0, 1]], bool)
    assert first_stream_cell(codes, stream).tolist() == [3, 3, 3, 5, 5]
    assert first_stream_cell(codes, np.zeros((1, 5), bool)).tolist() == [0] * 5
    table, raster, counters = table_np(codes, stream)
    assert table["catchment"].tolist() == [3, 2] and raster.tolist() == [[0, 0, 1, 0, 2]]
    assert table["down"].tolist() == [NONE, NONE] and counters["catchment_cells"] == 5
    # one rounding per operation: (8119, 0) and (0, 5741) have the same float32 length
    assert _length([8119], [0], 1.0) == _length([0], [5741], 1.0)


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd import streamnet
    from hydrodem_amd.filters import custom_filters
    assert hd.StreamNetwork is custom_filters.StreamNetwork
    assert hd.DemToStreamNetwork is custom_filters.DemToStreamNetwork
    assert issubclass(hd.StreamNetwork, hd.Filter) and issubclass(hd.DemToStreamNetwork, hd.Filter)
    assert hd.StreamNetwork.auto_device is True
    f = hd.StreamNetwork()
    assert f.columns is None and f.keep_partial_results is False and f.threshold is None
    assert f.stats == {} and f.table is None and f.count == 0 and f.cellsize == 1.0
    assert f.order is None and f.magnitude is None and f.links is None
    with pytest.raises(TypeError):
        hd.StreamNetwork(None, 100)                            # keyword-only
    assert {"streamnet_args", "streamlinks", "streamlinks_dev",
            "STREAMNET_COLUMNS"} <= set(dir(streamnet))
    assert tuple(streamnet.STREAMNET_COLUMNS) == COLUMNS
    chain = hd.DemToStreamNetwork(100)
    assert chain.threshold == 100 and chain.flats == "keep" and chain.stats == {}
    assert chain.cellsize == 1.0 and chain.columns is None and chain.table is None
    assert [type(m).__name__ for m in chain.filters] == ["SinkFill", "D8FlowDirection",
                                                         "FlowAccumulation"]
    assert chain.filters[0].epsilon == pytest.approx(hd.DemToStreamOrder(threshold=1)
                                                     .filters[0].epsilon)


def test_the_operators_resolve_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import StreamNetwork, DemToStreamNetwork
        import hydrodem_amd
        assert StreamNetwork is hydrodem_amd.StreamNetwork
        assert DemToStreamNetwork is hydrodem_amd.DemToStreamNetwork
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operators_reject_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend, streamnet

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    acc = np.ones((4, 4), np.uint32)
    link = np.zeros((4, 4), np.uint32)
    f = hd.StreamNetwork()
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
        with pytest.raises(ValueError, match=r"streams are \(3, 4\), the codes \(4, 4\)"):
            getattr(hd.StreamNetwork(np.ones((3, 4), bool)), form)(wrap(codes))
        with pytest.raises(ValueError, match=r"the dem is \(4, 5\), the codes \(4, 4\)"):
            getattr(hd.StreamNetwork(dem=np.ones((4, 5), np.float32)), form)(wrap(codes))
    # everything StreamOrder refuses
    with pytest.raises(ValueError, match="a threshold needs the uint32 raster"):
        hd.StreamNetwork(threshold=5)
    with pytest.raises(ValueError, match="a uint8 stream mask takes no threshold"):
        hd.StreamNetwork(np.ones((4, 4), bool), threshold=5)
    with pytest.raises(ValueError, match="a uint32 stream raster needs a threshold"):
        hd.StreamNetwork(acc)
    for bad in (0, -3, 2.5, True, 2 ** 32):
        with pytest.raises(ValueError, match="threshold is an integer in 1"):
            hd.StreamNetwork(acc, threshold=bad)
        with pytest.raises(ValueError, match="threshold is an integer in 1"):
            hd.DemToStreamNetwork(bad)
    with pytest.raises(ValueError, match="streams has dtype bool or uint8 or uint32"):
        hd.StreamNetwork(np.ones((4, 4), np.float32))
    with pytest.raises(ValueError, match="dem has dtype float32"):
        hd.StreamNetwork(dem=np.ones((4, 4), np.float64))
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="cellsize"):
            hd.StreamNetwork(cellsize=bad)
        with pytest.raises(ValueError, match="cellsize"):
            hd.DemToStreamNetwork(10, cellsize=bad)
    # the table's own
    for make in (lambda **kw: hd.StreamNetwork(**kw), lambda **kw: hd.DemToStreamNetwork(10, **kw)):
        with pytest.raises(ValueError, match="unknown stream network columns"):
            make(columns=("cells", "width"))
    for column in ("z_top", "z_end"):
        with pytest.raises(ValueError, match=f"the column {column} needs the dem"):
            hd.StreamNetwork(columns=(column,))
        hd.StreamNetwork(columns=(column,), dem=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="flats is 'keep' or 'resolve'"):
        hd.DemToStreamNetwork(10, flats="fill")
    with pytest.raises(ValueError, match="a float32 DEM"):
        hd.DemToStreamNetwork(10).apply(np.zeros((4, 4), np.float64))
    # the binding
    with pytest.raises(ValueError, match="codes is a NumPy array"):
        streamnet.streamlinks([[1]], link, 0)
    with pytest.raises(ValueError, match="needs the link raster"):
        streamnet.streamlinks(codes, None, 0)
    with pytest.raises(ValueError, match=r"the links are \(3, 4\), the codes \(4, 4\)"):
        streamnet.streamlinks(codes, link[:3], 0)
    with pytest.raises(ValueError, match="the links are uint32, got int32"):
        streamnet.streamlinks(codes, link.astype(np.int32), 0)
    with pytest.raises(ValueError, match="the column order needs the order raster"):
        streamnet.streamlinks(codes, link, 0, columns=("order",))
    with pytest.raises(ValueError, match="the column magnitude needs the magnitude raster"):
        streamnet.streamlinks(codes, link, 0, columns=("magnitude",))
    with pytest.raises(ValueError, match="no output wanted"):
        streamnet.streamlinks(codes, link, 0, columns=())
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="count is the number of links"):
            streamnet.streamlinks(codes, link, bad)
    # no link and no raster wanted: nothing to launch, typed empty columns
    table, row, stats = streamnet.streamlinks(codes, link, 0)
    assert row is None and stats["links"] == 0
    assert list(table) == [n for n, _ in COLUMNS if n not in ("order", "magnitude", "z_top", "z_end")]
    assert all(table[n].shape == (0,) and table[n].dtype == dict(COLUMNS)[n] for n in table)


def test_library_exports_the_streamlinks_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_streamlinks_u8") and hasattr(lib, "hdem_streamlinks_u8_dev")
    assert backend.SIGNATURES["hdem_streamlinks_u8"] == \
        backend.SIGNATURES["hdem_streamlinks_u8_dev"]
    assert len(backend.SIGNATURES["hdem_streamlinks_u8"]) == 28
    stats = backend._StreamLinksStats               # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 64 and stats().struct_size == 64
    assert stats.links.offset == 8 and stats.tops.offset == 32
    assert stats.tile_h.offset == 40 and stats.ms_rank.offset == 48
    assert set(stats().as_dict()) == set(COUNTERS) | {"tile_h", "tile_w", "ms_rank", "ms_trace",
                                                      "ms_tile", "ms_final"}
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    assert "A12" in header and "hdem_streamlinks_stats" in header
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile")).read()
    assert "hdem_streamnet.hip" in makefile


def test_null_context_calls_return_bad_arg(built):
    from hydrodem_amd import backend
    lib = backend.load_library()
    for name in ("hdem_streamlinks_u8", "hdem_streamlinks_u8_dev"):
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and b"ctx is null" in lib.hdem_last_error()
