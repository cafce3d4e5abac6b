"""
Cost distance, back link and allocation (``CostDistance``, ``CostAllocation``, ``CostPath``,
``hdem_costdistance_f32``): the CPU half.

The host references live here and are used by tests/test_gpu_costdistance.py.  They transcribe
block A28 of include/hydrodem_hip.h:
  ``cost_distance_ref``    Dijkstra with a heap on Python integers (exact), the back link by the
                           window order, nearest / label by following the back links, and the
                           counts that do not depend on a schedule;
  ``cost_distance_sweep``  an independent NumPy Bellman-Ford on uint64, to its fixed point.
No GPU here: the two agree, the reference holds the definition on written-out answers, and the
operators are importable and refuse what they must before a device is touched.
"""
import ctypes
import heapq
import math
import os
import re

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, costdistance as cd
from oracle.hdem_oracle_np import D8_CODES, D8_OFFSETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN = F32("nan")
NAN32 = 0x7FC00000
UNREACHED = 0xFFFFFFFF
SQRT2_Q31 = 3037000500
Q_MAX = 2 ** 28 - 1
SCHEDULE_FREE = ("sources", "barriers", "unreached", "tie_cells", "invalid", "max_units")


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def step_weight(s, diagonal):
    """The weight of a step between two cells whose quantised costs add up to ``s``."""
    return (s * SQRT2_Q31 + (1 << 30)) >> 31 if diagonal else s


def quantise(cost, frac_bits=16):
    """q of every cell, int64, 0 at a barrier (NaN); the refusal of the contract otherwise."""
    cost = np.asarray(cost)
    assert cost.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.rint(cost.astype(np.float64) * 2.0 ** frac_bits)
    nan = np.isnan(cost)
    bad = ~nan & ~((cost >= 0) & (scaled >= 1) & (scaled <= Q_MAX))
    if bad.any():
        raise ValueError(f"cost out of range in {int(bad.sum())} cells")
    return np.where(nan, 0.0, scaled).astype(np.int64)


def source_set(sources, threshold=None):
    sources = np.asarray(sources)
    if sources.dtype == np.bool_:
        return sources.copy()
    if sources.dtype == np.uint8 or threshold is None:
        return sources != 0
    return sources >= threshold


def cost_distance_ref(cost, sources, threshold=None, frac_bits=16, cellsize=1.0, max_units=0):
    """Block A28 on the host: ``{units, distance, backlink, nearest[, label]}`` and the
    schedule-free stats.  Python integers throughout."""
    h, w = cost.shape
    n = h * w
    q = quantise(cost, frac_bits).ravel()
    graph = np.flatnonzero(q).tolist()                     # the cells that are no barrier
    src = source_set(sources, threshold).ravel() & (q > 0)
    q, starts, src = q.tolist(), np.flatnonzero(src).tolist(), src.tolist()
    inf = 1 << 64
    dist = [inf] * n
    heap = []
    for i in starts:
        dist[i] = 0
        heap.append((0, i))
    # the neighbours of a cell, in window order, as (flat offset, dy, dx, diagonal)
    window = [(dy * w + dx, dy, dx, dy != 0 and dx != 0) for dy, dx in D8_OFFSETS]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        y, x = divmod(i, w)
        for off, dy, dx, diagonal in window:
            if not (0 <= y + dy < h and 0 <= x + dx < w):
                continue
            j = i + off
            if q[j] == 0:
                continue
            nd = d + step_weight(q[i] + q[j], diagonal)
            if nd < dist[j]:
                dist[j] = nd
                heapq.heappush(heap, (nd, j))

    units = np.full(n, -1, np.int64)
    distance = np.full(n, NAN32, np.uint32).view(np.float32)
    backlink = np.zeros(n, np.uint8)
    nearest = np.full(n, UNREACHED, np.uint32)
    scale = math.ldexp(float(cellsize), -(frac_bits + 1))
    ties = unreached = 0
    far = 0
    for i in sorted(graph, key=dist.__getitem__):          # a back link points at a smaller D
        d = dist[i]
        if d == inf or (max_units and d > max_units):
            unreached += 1
            continue
        units[i] = d
        distance[i] = F32(float(d) * scale)
        far = max(far, d)
        if src[i]:
            nearest[i] = i
            continue
        y, x = divmod(i, w)
        attain = []
        for (off, dy, dx, diagonal), code in zip(window, D8_CODES):
            if not (0 <= y + dy < h and 0 <= x + dx < w):
                continue
            j = i + off
            if q[j] and dist[j] != inf and dist[j] + step_weight(q[i] + q[j], diagonal) == d:
                attain.append((code, j))
        assert attain, "the distances solve the local equation"
        backlink[i] = attain[0][0]
        nearest[i] = nearest[attain[0][1]]
        ties += len(attain) > 1
    out = {"units": units.reshape(h, w), "distance": distance.reshape(h, w),
           "backlink": backlink.reshape(h, w), "nearest": nearest.reshape(h, w)}
    sources = np.asarray(sources)
    if sources.dtype == np.uint32 and threshold is None:
        label = np.zeros(n, np.uint32)
        hit = nearest != UNREACHED
        label[hit] = sources.ravel()[nearest[hit]]
        out["label"] = label.reshape(h, w)
    stats = {"sources": len(starts), "barriers": n - len(graph), "unreached": unreached,
             "tie_cells": ties, "invalid": 0, "max_units": far}
    return out, stats


def cost_distance_sweep(cost, sources, threshold=None, frac_bits=16, max_units=0):
    """D by Bellman-Ford on uint64 arrays, every cell from all eight neighbours at once until
    nothing changes: int64 units, -1 out of reach."""
    h, w = cost.shape
    q = np.zeros((h + 2, w + 2), np.uint64)
    q[1:-1, 1:-1] = quantise(cost, frac_bits).astype(np.uint64)
    inf = np.uint64(0xFFFFFFFFFFFFFFFF)
    dist = np.full((h + 2, w + 2), inf, np.uint64)
    dist[1:-1, 1:-1][source_set(sources, threshold) & (q[1:-1, 1:-1] > 0)] = 0
    own = q[1:-1, 1:-1]
    steps = []
    for dy, dx in D8_OFFSETS:
        qn = q[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
        s = own + qn
        weight = (s * np.uint64(SQRT2_Q31) + np.uint64(1 << 30)) >> np.uint64(31) \
            if dy and dx else s
        steps.append((dy, dx, weight, (own > 0) & (qn > 0)))
    while True:
        before = dist.copy()
        for dy, dx, weight, open_ in steps:
            dn = dist[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
            offer = np.where(open_ & (dn != inf), dn + weight, inf)
            np.minimum(dist[1:-1, 1:-1], offer, out=dist[1:-1, 1:-1])
        if np.array_equal(before, dist):
            break
    inner = dist[1:-1, 1:-1]
    gone = (inner == inf) | ((inner > np.uint64(max_units)) if max_units else False)
    return np.where(gone, np.int64(-1), inner.astype(np.int64))


def follow(backlink, cell):
    """The cells of the back-link path from ``cell``, itself included."""
    step = dict(zip(D8_CODES, D8_OFFSETS))
    cells = [cell]
    while backlink[cells[-1]]:
        dy, dx = step[int(backlink[cells[-1]])]
        cells.append((cells[-1][0] + dy, cells[-1][1] + dx))
        assert len(cells) <= backlink.size
    return cells


def random_case(shape, kind, which, seed=1):
    """The rasters of the GPU tests: costs ``0.5 + 9 U`` at frac_bits 16 (``which`` "float") or
    integers 1 ... 5 at frac_bits 0 ("integer"), 5 % NaN barriers, sources at density 0.001
    (one at least) given as a ``mask``, an ``acc`` raster with threshold 100 or ``labels``.
    Returns ``cost, sources, threshold, frac_bits``."""
    rng = np.random.default_rng(seed)
    if which == "float":
        cost, frac_bits = (0.5 + 9.0 * rng.random(shape)).astype(F32), 16
    else:
        cost, frac_bits = rng.integers(1, 6, shape).astype(F32), 0
    cost[rng.random(shape) < 0.05] = NAN
    src = rng.random(shape) < 0.001
    if not (src & ~np.isnan(cost)).any():
        flat = np.flatnonzero(~np.isnan(cost).ravel())
        src.ravel()[flat[len(flat) // 2]] = True
    if kind == "mask":
        return cost, src.astype(np.uint8), None, frac_bits
    if kind == "acc":
        acc = rng.integers(1, 100, shape).astype(np.uint32)
        acc[src] = rng.integers(100, 5000, int(src.sum()))
        return cost, acc, 100, frac_bits
    labels = np.zeros(shape, np.uint32)
    labels[src] = rng.integers(1, 2 ** 32 - 1, int(src.sum()), dtype=np.uint64)
    return cost, labels, None, frac_bits


# ---------------------------------------------------------------------------
# the two references agree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["float", "integer"])
@pytest.mark.parametrize("kind", ["mask", "acc", "labels"])
def test_dijkstra_and_the_sweep_agree_on_random_costs(kind, which):
    cost, sources, threshold, frac_bits = random_case((61, 83), kind, which, seed=3)
    want, stats = cost_distance_ref(cost, sources, threshold, frac_bits)
    assert np.array_equal(want["units"], cost_distance_sweep(cost, sources, threshold, frac_bits))
    assert stats["barriers"] == int(np.isnan(cost).sum())
    assert stats["unreached"] == int((want["units"] < 0).sum()) - stats["barriers"]
    assert stats["max_units"] == want["units"].max()


def test_dijkstra_and_the_sweep_agree_behind_walls_and_under_a_limit():
    rng = np.random.default_rng(5)
    cost = rng.integers(1, 6, (40, 57)).astype(F32)
    cost[5:35, 20] = NAN                     # a wall with a gap at either end
    cost[10, 30:57] = NAN                    # a wall to the edge
    cost[25:30, 40:45] = NAN
    cost[26:29, 41:44] = 1                   # ... and a closed pocket
    src = np.zeros(cost.shape, np.uint8)
    src[2, 3] = src[38, 50] = 1
    free, _ = cost_distance_ref(cost, src, frac_bits=0)
    assert np.array_equal(free["units"], cost_distance_sweep(cost, src, frac_bits=0))
    assert (free["units"][26:29, 41:44] == -1).all()
    limit = int(np.median(free["units"][free["units"] >= 0]))
    cut, stats = cost_distance_ref(cost, src, frac_bits=0, max_units=limit)
    assert np.array_equal(cut["units"], cost_distance_sweep(cost, src, frac_bits=0,
                                                            max_units=limit))
    inside = (free["units"] >= 0) & (free["units"] <= limit)
    assert 0 < inside.sum() < (free["units"] >= 0).sum()
    for name in ("units", "backlink", "nearest"):          # the limit changes no cell within it
        assert np.array_equal(cut[name][inside], free[name][inside])
    assert np.array_equal(cut["distance"].view(np.uint32)[inside],
                          free["distance"].view(np.uint32)[inside])
    assert (cut["units"][~inside] == -1).all() and (cut["backlink"][~inside] == 0).all()
    assert (cut["nearest"][~inside] == UNREACHED).all()
    assert (cut["distance"].view(np.uint32)[~inside] == NAN32).all()
    assert stats["max_units"] <= limit
    assert stats["unreached"] == int((~inside).sum()) - stats["barriers"]


# ---------------------------------------------------------------------------
# written-out answers
# ---------------------------------------------------------------------------
def test_the_diagonal_weight_is_the_rounded_product_with_sqrt2():
    assert SQRT2_Q31 == cd.SQRT2_Q31 == (math.isqrt(8 << 62) + 1) // 2      # round(sqrt(2) 2^31)
    assert step_weight(2, True) == 3 and step_weight(2, False) == 2
    assert step_weight(3, True) == 4
    assert step_weight(1 << 29, True) == 759250125
    for s in (2, 3, 1 << 29, 131072, 2 * Q_MAX):
        exact = (math.isqrt(8 * s * s) + 1) // 2           # round(s sqrt(2)), in integers
        assert step_weight(s, True) == exact
        assert s * SQRT2_Q31 + (1 << 30) < 1 << 64         # the product fits uint64


def test_uniform_cost_gives_the_octile_distance():
    h, w, sy, sx = 130, 197, 41, 77
    src = np.zeros((h, w), np.uint8)
    src[sy, sx] = 1
    got, stats = cost_distance_ref(np.ones((h, w), F32), src)
    a, b = np.abs(np.arange(h) - sy)[:, None], np.abs(np.arange(w) - sx)[None, :]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert np.array_equal(got["units"], 131072 * (hi - lo) + 185364 * lo)
    assert stats == {"sources": 1, "barriers": 0, "unreached": 0, "invalid": 0,
                     "tie_cells": stats["tie_cells"], "max_units": int(got["units"].max())}
    assert (got["nearest"] == sy * w + sx).all()
    assert cd.units_per_cost(1.0, 16) == 2.0 ** -17
    assert got["distance"][sy, sx + 3] == 3.0 and got["distance"][sy, sx] == 0.0
    # straight lines have one way back; everything else ties and takes the first in the window
    assert got["backlink"][sy, sx] == 0
    assert (got["backlink"][sy, sx + 1:] == 16).all() and (got["backlink"][:sy, sx] == 4).all()
    assert got["backlink"][sy - 5, sx - 5] == 2 and got["backlink"][sy + 5, sx - 5] == 128
    assert got["backlink"][sy + 2, sx + 5] == 32           # NW before W
    assert got["backlink"][sy - 2, sx + 5] == 16           # W before SW


def test_a_cheap_road_round_an_expensive_block_is_taken():
    cost = np.full((7, 9), 1, F32)
    cost[1:6, 2:7] = 100                                   # the block
    src = np.zeros(cost.shape, np.uint8)
    src[3, 0] = 1
    got, _ = cost_distance_ref(cost, src, frac_bits=0)
    cells = follow(got["backlink"], (3, 8))
    assert cells[-1] == (3, 0) and all(cost[c] == 1 for c in cells)
    # 4 diagonal and 6 cardinal steps round the block's corner, all between cost-1 cells
    assert got["units"][3, 8] == 4 * 3 + 6 * 2
    assert got["units"][3, 8] < 2 * (1 + 100)              # less than entering the block once


def test_a_pocket_behind_nan_walls_is_unreached_and_a_diagonal_squeezes_through():
    cost = np.ones((6, 6), F32)
    cost[0:4, 3] = NAN
    cost[3, 3:6] = NAN                                     # the pocket: rows 0-2, columns 4-5
    src = np.zeros(cost.shape, np.uint8)
    src[5, 0] = 1
    src[3, 3] = 1                                          # a source on a barrier is no source
    got, stats = cost_distance_ref(cost, src, frac_bits=0)
    assert (got["units"][0:3, 4:6] == -1).all() and stats["unreached"] == 6
    assert stats["sources"] == 1 and stats["barriers"] == 6
    assert got["units"][3, 3] == -1 and got["nearest"][3, 3] == UNREACHED
    cost[3, 4] = 1                                         # a door in the pocket's floor
    got, stats = cost_distance_ref(cost, src, frac_bits=0)
    assert stats["unreached"] == 0
    # (3, 4) has barriers W and E of it; its only ways in are the diagonals from row 4
    assert got["backlink"][3, 4] in (8, 4, 2) and got["backlink"][2, 4] == 4
    cost[4, 4] = NAN                                       # only the two diagonals are left
    got, _ = cost_distance_ref(cost, src, frac_bits=0)
    assert got["backlink"][3, 4] == 8                      # SW, between barriers at W and S
    assert got["units"][3, 4] == got["units"][4, 3] + 3


def test_the_first_neighbour_in_window_order_wins_a_tie():
    # the centre and its diagonal neighbours cost 1, its cardinal neighbours 2, all eight are
    # sources: 1 + 2 = 3 along a cardinal step, round(2 sqrt(2)) = 3 along a diagonal one
    cost = np.array([[1, 2, 1], [2, 1, 2], [1, 2, 1]], F32)
    src = np.ones((3, 3), np.uint8)
    src[1, 1] = 0
    for k, ((dy, dx), code) in enumerate(zip(D8_OFFSETS, D8_CODES)):
        got, stats = cost_distance_ref(cost, src, frac_bits=0)
        assert got["units"][1, 1] == 3 and got["backlink"][1, 1] == code
        assert got["nearest"][1, 1] == (1 + dy) * 3 + 1 + dx
        assert stats["tie_cells"] == (1 if k < 7 else 0) and stats["sources"] == 8 - k
        cost[1 + dy, 1 + dx] = NAN                         # the winner leaves; the next one wins


@pytest.mark.parametrize("which", ["float", "integer"])
def test_back_links_add_up_to_the_distance_and_strictly_decrease_it(which):
    cost, labels, _, frac_bits = random_case((47, 59), "labels", which, seed=7)
    got, stats = cost_distance_ref(cost, labels, None, frac_bits)
    q = quantise(cost, frac_bits)
    units, backlink = got["units"], got["backlink"]
    assert stats["tie_cells"] > 0 or which == "float"
    for cell in zip(*np.nonzero(units >= 0)):
        cells = follow(backlink, cell)
        total = 0
        for a, b in zip(cells[:-1], cells[1:]):
            assert units[b] < units[a]
            total += step_weight(int(q[a] + q[b]), a[0] != b[0] and a[1] != b[1])
        assert total == units[cell]
        end = cells[-1]
        assert labels[end] != 0 and got["nearest"][cell] == end[0] * 59 + end[1]
        assert got["label"][cell] == labels[end]
    assert (backlink[units < 0] == 0).all() and (got["label"][units < 0] == 0).all()


def test_the_reference_refuses_costs_out_of_range_with_their_count():
    src = np.ones((1, 4), np.uint8)
    for bad in (-1.0, 0.0, np.inf, 2.0 ** -18, 4096.0):
        with pytest.raises(ValueError, match="cost out of range in 2 cells"):
            cost_distance_ref(np.array([[1, bad, NAN, bad]], F32), src)
    assert quantise(np.array([[2.0 ** -16, 4095.5, NAN]], F32)).tolist() == [[1, 268402688, 0]]
    assert quantise(np.array([[2 ** 28 - 16]], F32), 0).tolist() == [[2 ** 28 - 16]]
    assert quantise(np.array([[1.5, 2.5, 3.5]], F32), 0).tolist() == [[2, 2, 4]]   # to even
    with pytest.raises(ValueError, match="in 1 cells"):
        quantise(np.array([[0.5, 1.5]], F32), 0)           # 0.5 rounds to even: 0


# ---------------------------------------------------------------------------
# the binding and the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    from hydrodem_amd.filters import custom_filters
    for name in ("CostDistance", "CostAllocation", "CostPath"):
        assert getattr(hd, name) is getattr(custom_filters, name)
        assert issubclass(getattr(hd, name), hd.Filter)
    mask = np.zeros((3, 4), bool)
    f = hd.CostDistance(mask)
    assert f.output == "distance" and f.frac_bits == 16 and f.cellsize == 1.0 and f.stats == {}
    assert f.sources.dtype == np.uint8 and f.max_distance is None
    assert hd.CostDistance(mask, output="backlink").output == "backlink"
    assert hd.CostAllocation(mask).output == "nearest"
    assert hd.CostAllocation(np.zeros((3, 4), np.uint32)).output == "label"
    assert hd.CostAllocation(np.zeros((3, 4), np.uint32), threshold=5).output == "nearest"
    assert hd.CostPath([(1, 2), (0, 0)]).cells == [(1, 2), (0, 0)]
    assert hd.CostPath(mask).destinations.dtype == np.uint8
    assert cd.ON_DEVICE == 0x40000000 and cd.units_per_cost(30.0, 0) == 15.0
    assert cd.max_units_of(None) == 0 and cd.max_units_of(10.0, 1.0, 0) == 20
    assert cd.max_units_of(0.75, 1.0, 1) == 3 and cd.max_units_of(0.74, 1.0, 1) == 2   # floor


def test_every_refusal_comes_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    cost = np.ones((4, 5), F32)
    mask = np.zeros((4, 5), np.uint8)
    acc = np.zeros((4, 5), np.uint32)

    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    args = cd.costdistance_args
    assert args(cost, mask) == (1, 0, 0, ("distance",), 1.0)
    assert args(cost, acc, 7, ("nearest", "units"), 2, 0, max_units=9) == \
        (2, 7, 9, ("units", "nearest"), 2.0)
    assert args(cost, acc, None, "label", max_distance=1.0)[:3] == (3, 0, 2 ** 17)
    assert said(lambda: args(None, mask)) == "cost distance needs the cost raster it crosses"
    assert said(lambda: args(cost, None)) == \
        "cost distance needs the source raster it measures from"
    assert said(lambda: args(cost.astype(np.float64), mask)) == \
        "cost distance takes a float32 cost raster, got float64"
    assert said(lambda: args(np.ones((2, 4, 5), F32), mask)) == \
        "cost distance takes a 2-D raster, got 3 dimensions"
    assert said(lambda: args(cost, mask[:3])) == "the sources are (3, 5), the cost (4, 5)"
    assert said(lambda: args(cost, mask.astype(np.int32))) == \
        "sources are a uint8 mask, a uint32 raster with a threshold or a uint32 label raster, " \
        "got int32"
    assert said(lambda: args(cost, mask, 3)) == "a uint8 source mask takes no threshold"
    for bad in (0, 1.5, True, 2 ** 32):
        assert said(lambda: args(cost, acc, bad)) == \
            f"threshold is an integer in 1 ... 2^32 - 1, got {bad!r}"
    assert said(lambda: args(cost, mask, want="label")) == \
        "label needs a uint32 label raster as sources (and no threshold)"
    assert said(lambda: args(cost, acc, 5, want="label")) == \
        "label needs a uint32 label raster as sources (and no threshold)"
    assert said(lambda: args(cost, mask, want=())) == \
        "no output wanted: choose among ['units', 'distance', 'backlink', 'nearest', 'label']"
    assert said(lambda: args(cost, mask, want="d2")) == \
        "unknown cost distance outputs ['d2']: choose among " \
        "['units', 'distance', 'backlink', 'nearest', 'label']"
    for bad in (-1, 17, 1.0, True):
        assert said(lambda: args(cost, mask, frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 16, got {bad!r}"
    assert said(lambda: args(cost, mask, cellsize=0)) == \
        "cellsize must be finite and positive, got 0.0"
    for bad in (0, -2.0, float("inf"), True):
        assert said(lambda: args(cost, mask, max_distance=bad)) == \
            f"max_distance must be finite and positive, got {bad!r}"
    assert said(lambda: args(cost, mask, max_distance="far")) == \
        "max_distance is a number, got 'far'"
    assert said(lambda: args(cost, mask, max_distance=1e-9)).startswith(
        "max_distance 1e-09 is 0 units of ")
    assert said(lambda: args(cost, mask, max_distance=3.0, max_units=4)) == \
        "give max_distance or max_units, not both"
    for bad in (-1, 2 ** 63, 0.5, True):
        assert said(lambda: args(cost, mask, max_units=bad)) == \
            f"max_units is an integer in 0 ... 2^63 - 1 (0: no limit), got {bad!r}"

    class Huge:                                            # pylint: disable=too-few-public-methods
        dtype, shape = np.dtype(np.float32), (65536, 65536)
    assert said(lambda: args(Huge(), mask)) == \
        "cost distance works in uint32: 65536 x 65536 is more than 2^32 - 1 cells"
    # the bindings and the operators
    assert said(lambda: cd.costdistance([[1.0]], mask)) == \
        "cost is a NumPy array, got <class 'list'>"
    assert said(lambda: cd.costdistance(cost, mask, want="units", max_units=-3)).startswith(
        "max_units is an integer")
    assert said(lambda: hd.CostDistance(None)).startswith(
        "CostDistance needs the sources it measures from")
    assert said(lambda: hd.CostDistance(mask.astype(np.int16))) == \
        "sources has dtype bool or uint8 or uint32, got int16"
    assert said(lambda: hd.CostDistance(mask, output="nearest")) == \
        "output is one of ['distance', 'units', 'backlink'], got 'nearest'"
    assert said(lambda: hd.CostAllocation(mask, output="label")) == \
        "label needs a uint32 label raster as sources (and no threshold)"
    assert said(lambda: hd.CostAllocation(mask, output="distance")) == \
        "output is one of ['nearest', 'label'], got 'distance'"
    assert said(lambda: hd.CostDistance(mask, frac_bits=20)) == \
        "frac_bits is an integer in 0 ... 16, got 20"
    assert said(lambda: hd.CostDistance(mask, max_distance=-1)) == \
        "max_distance must be finite and positive, got -1"
    assert said(lambda: hd.CostDistance(mask).apply(cost.astype(np.float64))) == \
        "cost distance takes a float32 cost raster, got float64"
    assert said(lambda: hd.CostDistance(mask).apply(cost[:2])) == \
        "the sources are (4, 5), the cost (2, 5)"
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.CostDistance(mask).apply([[1.0]])
    assert said(lambda: hd.CostPath(None)).startswith("CostPath needs the destinations")
    assert said(lambda: hd.CostPath(5)).startswith(
        "destinations are a uint8 mask or a list of (row, column) cells, got 5")
    assert said(lambda: hd.CostPath([(1, -1)])).startswith("destinations are a uint8 mask")
    assert said(lambda: hd.CostPath([])).startswith("destinations are a uint8 mask")
    assert said(lambda: hd.CostPath(acc)) == "destinations has dtype bool or uint8, got uint32"
    assert said(lambda: hd.CostPath([(4, 0)]).apply(mask)) == \
        "destination (4, 0) lies outside the 4 x 5 raster"
    assert said(lambda: hd.CostPath([(0, 0)]).apply(acc)) == \
        "CostPath takes uint8 back-link codes, got uint32"


def test_the_header_declares_the_entry_point_and_the_binding_mirrors_it(built):
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "A28  CostDistance.apply" in header
    args = re.search(r"int hdem_costdistance_f32\((.*?)\);", header, re.S).group(1)
    assert len(args.split(",")) == 17 == len(backend.SIGNATURES["hdem_costdistance_f32"])
    struct = re.search(r"typedef struct hdem_costdistance_stats \{(.*?)\} "
                       r"hdem_costdistance_stats;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?(?:\[\d+\])?;",
                       re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    declared = [n for pair in names for n in pair if n]
    stats = backend._CostDistanceStats                      # pylint: disable=protected-access
    assert declared == [name for name, _ in stats._fields_]
    assert ctypes.sizeof(stats) == 96
    assert "hdem_costdistance_stats;   /* sizeof == 96 */" in header
    assert set(SCHEDULE_FREE) < set(stats().as_dict()) and "reserved" not in stats().as_dict()
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "hdem_costdistance.hip" in makefile
    # one symbol: no _dev twin anywhere, and nothing new in the backend's public names
    assert "hdem_costdistance_f32_dev" not in header
    assert not [n for n in backend.SIGNATURES if "costdistance" in n and n.endswith("_dev")]
    assert not [n for n in dir(backend) if "cost" in n.lower() and n.endswith("_dev")]
    assert not [n for n in backend.__all__ if "cost" in n.lower()]
    # the library exports it, and a null context is BAD_ARG, whatever else is passed
    lib = backend.load_library()
    rc = lib.hdem_costdistance_f32(*[t() for t in backend.SIGNATURES["hdem_costdistance_f32"]])
    assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
    with pytest.raises(AttributeError):
        getattr(lib, "hdem_costdistance_f32_dev")
