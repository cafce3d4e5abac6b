"""
D-infinity distance down and HAND (``DInfDistanceDown``, ``DInfHeightAboveDrainage``,
``DemToDInfHAND``, ``hdem_dinfdist_u32``): the CPU half.

The host reference lives here and is used by tests/test_gpu_dinfdist.py.  It transcribes block
A26 of include/hydrodem_hip.h:
  ``distance_ref``   Kahn's order over the reversed graph: the stop cells and the cells without
                     outflow first, then every cell whose receivers are all done, one frontier
                     at a time, float64 in the contract's order of operations;
  ``distance_walk``  the same pull by plain recursion, cell by cell -- tiny grids.
No GPU here: the reference holds the definition on written-out answers, agrees with the walk and
with the D8 flow trace on canonical words, keeps the order of the three statistics, and the
operators are importable and refuse what they must before a device is touched.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, dinf
from hydrodem_amd.dinf import FACETS, Q_ONE
from test_dinf import direction_ref, plane, random_dem, receivers
from test_flowacc import acc_kahn, random_acyclic_codes, terminal_mask
from test_flowtrace import distance_of, hand_of, trace_doubling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KINDS = ("horizontal", "vertical", "surface")
STATISTICS = ("average", "minimum", "maximum")
NAN32 = np.uint32(0x7FC00000)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def stops_of(words, streams=None, threshold=None):
    """The stop set as a bool raster: the cells with facet 0, a mask, or ``>= threshold``."""
    if streams is None:
        return np.asarray(words) >> 16 == 0
    streams = np.asarray(streams)
    return streams >= threshold if threshold is not None else streams != 0


def _costs(words, dem, kind, dx, dy):
    """(cost to the cardinal receiver, to the diagonal one) as functions of (cells, receivers)."""
    facet = (np.asarray(words, np.uint32) >> 16).ravel()
    east_west = np.isin(facet, [k for k, ((ey, _), _, _, _) in FACETS.items() if ey == 0])
    h_card = np.where(east_west, float(dx), float(dy))
    diag = math.sqrt(dx * dx + dy * dy)
    z = None if dem is None else np.asarray(dem, F32).ravel().astype(np.float64)

    def cost(cells, rec, h):
        if kind == "horizontal":
            return h
        v = z[cells] - z[rec]
        return v if kind == "vertical" else np.sqrt(h * h + v * v)

    return (lambda cells, rec: cost(cells, rec, h_card[cells]),
            lambda cells, rec: cost(cells, rec, np.full(cells.size, diag)))


def _combine(statistic, q, a1, a2):
    """D of cells with two receivers."""
    if statistic == "average":
        return ((Q_ONE - q).astype(np.float64) * a1 + q.astype(np.float64) * a2) * 2.0 ** -15
    n1, n2 = np.isnan(a1), np.isnan(a2)
    if statistic == "maximum":
        return np.where(n1 | n2, np.nan, np.where(a2 > a1, a2, a1))
    return np.where(n1, a2, np.where(n2, a1, np.where(a2 < a1, a2, a1)))


def _to_f32(d):
    with np.errstate(over="ignore"):
        out = d.astype(F32)
    out.view(np.uint32)[np.isnan(out)] = NAN32             # one NaN bit pattern
    return out


def distance_ref(words, stops, dem=None, kind="horizontal", statistic="average", dx=1.0, dy=1.0):
    """float32 ``distance`` of block A26 in Kahn's order over the reversed graph; ValueError with
    the count for invalid words, receivers outside the raster and "N cells never resolve"."""
    words = np.asarray(words, np.uint32)
    card, diag, q = receivers(words)
    n = words.size
    stop = np.asarray(stops, bool).ravel()
    done = stop | (words.ravel() >> 16 == 0)
    d = np.full(n, np.nan)
    d[stop] = 0.0
    cost_card, cost_diag = _costs(words, dem, kind, dx, dy)
    # the edges donor -> receiver of the cells that are not final, by receiver
    need = np.where(done, 0, (card >= 0).astype(np.int64) + (diag >= 0))
    src = np.concatenate([np.flatnonzero((rec >= 0) & ~done) for rec in (card, diag)])
    dst = np.concatenate([rec[(rec >= 0) & ~done] for rec in (card, diag)])
    order = np.argsort(dst, kind="stable")
    src, first = src[order], np.searchsorted(dst[order], np.arange(n + 1))
    frontier = np.flatnonzero(done)
    resolved = 0
    with np.errstate(all="ignore"):
        while frontier.size:
            resolved += frontier.size
            count = first[frontier + 1] - first[frontier]
            at = np.repeat(first[frontier] - (np.cumsum(count) - count), count) + \
                np.arange(int(count.sum()))
            donors = src[at]
            np.subtract.at(need, donors, 1)
            cells = np.unique(donors)
            cells = cells[need[cells] == 0]
            c1, c2, qc = card[cells], diag[cells], q[cells]
            a1 = np.where(c1 >= 0, cost_card(cells, c1) + d[c1], np.nan)
            a2 = np.where(c2 >= 0, cost_diag(cells, c2) + d[c2], np.nan)
            d[cells] = np.where(c2 < 0, a1, np.where(c1 < 0, a2, _combine(statistic, qc, a1, a2)))
            frontier = cells
    if resolved != n:
        raise ValueError(f"D-infinity words form a cycle without a stop cell: {n - resolved} "
                         "cells never resolve")
    return _to_f32(d).reshape(words.shape)


def distance_walk(words, stops, dem=None, kind="horizontal", statistic="average", dx=1.0, dy=1.0):
    """The same pull, cell by cell with memoised recursion (tiny acyclic grids)."""
    words = np.asarray(words, np.uint32)
    h, w = words.shape
    stops = np.asarray(stops, bool)
    diag_len = math.sqrt(dx * dx + dy * dy)
    memo = {}

    def arrive(y, x, step, length):
        ny, nx = y + step[0], x + step[1]
        if kind == "horizontal":
            cost = length
        else:
            v = float(dem[y, x]) - float(dem[ny, nx])
            cost = v if kind == "vertical" else math.sqrt(length * length + v * v)
        return cost + down(ny, nx)

    def down(y, x):
        if (y, x) not in memo:
            facet, q = int(words[y, x] >> 16), int(words[y, x] & 0xFFFF)
            if stops[y, x]:
                memo[y, x] = 0.0
            elif facet == 0:
                memo[y, x] = math.nan
            else:
                e1, e2, _, _ = FACETS[facet]
                a1 = arrive(y, x, e1, dx if e1[0] == 0 else dy) if q != Q_ONE else None
                a2 = arrive(y, x, e2, diag_len) if q != 0 else None
                if a1 is None or a2 is None:
                    memo[y, x] = a2 if a1 is None else a1
                else:
                    memo[y, x] = float(_combine(statistic, np.int64(q), np.float64(a1),
                                                np.float64(a2)))
        return memo[y, x]

    with np.errstate(all="ignore"):
        return _to_f32(np.array([[down(y, x) for x in range(w)] for y in range(h)], np.float64))


def counts_of(words, stops, distance):
    """The stats of the distance that do not depend on the schedule."""
    q = np.asarray(words) & 0xFFFF
    return {"split_cells": int(((q != 0) & (q != Q_ONE)).sum()),
            "terminal_cells": int((np.asarray(words) >> 16 == 0).sum()),
            "stop_cells": int(np.asarray(stops, bool).sum()),
            "unreached_cells": int(np.isnan(distance).sum()),
            "invalid": 0, "outside": 0, "unresolved": 0, "tile_h": 64, "tile_w": 64}


def same_bits(a, b):
    return a.dtype == b.dtype == F32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ulps_apart(a, b):
    """The float32 steps between two finite non-negative float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def d8_case(shape, seed, lo=64.0, span=192.0):
    """Acyclic D8 codes whose every code stays inside the raster, a DEM in [64, 256) whose
    elevations are multiples of 2^-17 above 64, and a stream mask from the accumulation."""
    codes = random_acyclic_codes(*shape, seed=seed, ramp=True)
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    z = (lo + np.random.default_rng(seed).random(shape) * span).astype(F32)
    assert z.min() >= 64 and z.max() < 256
    return codes, z, acc_kahn(codes) >= 8


# ---------------------------------------------------------------------------
# the definition on written-out answers
# ---------------------------------------------------------------------------
def test_a_plane_tilted_east_with_a_stream_column():
    z = plane((6, 9), 0.5, 0.0)
    words = direction_ref(z)[0]
    streams = np.zeros((6, 9), bool)
    streams[:, 6] = True
    offset = np.arange(6, -1, -1, dtype=F32)
    got = distance_ref(words, streams)
    assert np.array_equal(got[1:-1, 1:7], np.tile(offset[1:], (4, 1)))
    assert np.isnan(got[1:-1, 7:]).all() and np.isnan(got[0, :6]).all()    # the ring: no outflow
    assert np.isnan(got[:, 0]).all()
    assert (got[:, 6] == 0).all()                                          # a stop, ring or not
    drop = distance_ref(words, streams, z, "vertical")
    assert np.array_equal(drop[1:-1, 1:7], np.tile(offset[1:] * F32(0.5), (4, 1)))
    surface = distance_ref(words, streams, z, "surface")
    assert np.array_equal(surface[1:-1, 5], np.full(4, F32(math.sqrt(1.25))))
    for kind in KINDS:
        for statistic in STATISTICS:                       # one receiver: the statistic is moot
            a = distance_ref(words, streams, None if kind == "horizontal" else z, kind, statistic)
            assert same_bits(a, distance_walk(words, streams, z, kind, statistic))
            assert same_bits(a, {"horizontal": got, "vertical": drop, "surface": surface}[kind])
    # to the outlet: the ring is the stop set, the interior counts its steps to column 8
    out = distance_ref(words, stops_of(words))
    assert np.array_equal(out[1:-1, 1:], np.tile(np.arange(7, -1, -1, dtype=F32), (4, 1)))
    assert not out[:, 0].any()
    assert not out[0].any() and not out[-1].any()


def test_a_plane_towards_22_5_degrees_on_five_by_five_averages_in_halves():
    theta = math.pi / 8
    z = plane((5, 5), math.cos(theta), math.sin(theta))
    words = direction_ref(z)[0]
    facet, q = dinf.unpack(words)
    assert (facet[1:-1, 1:-1] == 1).all() and (q[1:-1, 1:-1] == 16384).all()
    stops = stops_of(words)                                # the ring
    r2 = math.sqrt(2.0)
    want = np.zeros((5, 5))
    for x in (3, 2, 1):                                    # east to west is downstream first
        for y in (1, 2, 3):
            want[y, x] = (16384.0 * (1.0 + want[y, x + 1]) +
                          16384.0 * (r2 + want[y - 1, x + 1])) * 2.0 ** -15
    assert want[1, 3] == want[3, 3] == (1.0 + r2) / 2       # both receivers on the ring
    assert want[1, 2] == (1.0 + (1.0 + r2) / 2 + r2) / 2    # E is interior, NE on the ring
    assert want[2, 2] == (1.0 + (1.0 + r2) / 2 + r2 + (1.0 + r2) / 2) / 2
    got = distance_ref(words, stops)
    assert same_bits(got, want.astype(F32)) and same_bits(got, distance_walk(words, stops))
    # the shortest way out is one step east from column 3, the longest a diagonal step more
    low = distance_ref(words, stops, statistic="minimum")
    high = distance_ref(words, stops, statistic="maximum")
    assert (low[1:-1, 3] == 1).all() and (high[1:-1, 3] == F32(r2)).all()
    assert low[3, 1] == 3 and low[1, 1] == F32(r2) and high[3, 1] == F32(3 * r2)
    # vertical: a plane drops by the same amount along either receiver's path to a given cell,
    # but the two paths end on different ring cells; the average stays between the extremes
    for kind in ("vertical", "surface"):
        a, lo, hi = (distance_ref(words, stops, z, kind, s) for s in STATISTICS)
        assert (lo <= a).all() and (a <= hi).all() and (lo[1:-1, 1:-1] > 0).all()
        assert same_bits(a, distance_walk(words, stops, z, kind))


def test_a_cone_and_cells_that_are_not_square():
    rows, cols = np.mgrid[0:9, 0:9]
    z = (-np.hypot(rows - 4, cols - 4)).astype(F32)
    words = direction_ref(z)[0]
    stops = stops_of(words)
    assert ((words & 0xFFFF != 0) & (words & 0xFFFF != Q_ONE)).sum() > 20
    for kind in KINDS:
        for statistic in STATISTICS:
            got = distance_ref(words, stops, z, kind, statistic) if kind != "horizontal" else \
                distance_ref(words, stops, None, kind, statistic)
            assert same_bits(got, distance_walk(words, stops, z, kind, statistic))
            assert np.isfinite(got).all()
    # the summit is three steps of the ring away along its axis, and no path is shorter
    assert distance_ref(words, stops, statistic="minimum")[4, 4] == 4
    # vertical on the cone: every path from the summit ends on the ring, between its corner's and
    # its edge midpoint's elevation
    drop = distance_ref(words, stops, z, "vertical")[4, 4]
    assert 4.0 <= drop <= math.hypot(4, 4)
    # dx != dy: east costs dx, north dy, the diagonal sqrt(dx^2 + dy^2)
    dx, dy = 30.0, 10.0
    z = plane((5, 6), 3.0, 0.5, dx, dy)
    words = direction_ref(z, dx, dy)[0]
    q = int(words[2, 2] & 0xFFFF)
    assert (dinf.unpack(words)[0][1:-1, 1:-1] == 1).all() and 0 < q < Q_ONE
    got = distance_ref(words, stops_of(words), None, "horizontal", "average", dx, dy)
    assert got[1, 4] == F32(((Q_ONE - q) * dx + q * math.sqrt(dx * dx + dy * dy)) * 2.0 ** -15)
    assert distance_ref(words, stops_of(words), None, "horizontal", "minimum", dx, dy)[3, 1] == \
        F32(3 * math.sqrt(1000.0))                         # three diagonal steps beat four east
    assert same_bits(got, distance_walk(words, stops_of(words), None, "horizontal", "average",
                                        dx, dy))
    north = direction_ref(plane((5, 6), 0.0, 2.0, dx, dy), dx, dy)[0]
    assert distance_ref(north, stops_of(north), None, "horizontal", "average", dx, dy)[3, 2] == 30


# ---------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (9, 14), (17, 23)])
def test_the_reference_agrees_with_the_walk_on_random_dems(shape):
    z = random_dem(shape, seed=shape[0] * 100 + shape[1], nan=0.02)
    words = direction_ref(z)[0]
    rng = np.random.default_rng(shape[1])
    for stops in (stops_of(words), rng.random(shape) < 0.1, np.zeros(shape, bool)):
        for kind in KINDS:
            for statistic in STATISTICS:
                dem = None if kind == "horizontal" else z
                got = distance_ref(words, stops, dem, kind, statistic, 2.0, 3.0)
                assert same_bits(got, distance_walk(words, stops, dem, kind, statistic, 2.0, 3.0))
    assert np.isnan(distance_ref(words, np.zeros(shape, bool))).all()


@pytest.mark.parametrize("shape", [(9, 14), (40, 70), (130, 197)])
def test_canonical_words_reproduce_the_d8_flow_trace(shape):
    codes, z, streams = d8_case(shape, seed=shape[1])
    words = dinf.words_from_d8(codes)
    for mask in (None, streams):
        stop, ncard, ndiag = trace_doubling(codes, mask)
        stops = stops_of(words, mask)
        got = {s: distance_ref(words, stops, z, "vertical", s) for s in STATISTICS}
        # elevations in [64, 256) are multiples of 2^-17: every float64 sum is exact, and its one
        # rounding to float32 is the float32 subtraction's
        want = hand_of(stop, z)
        want.view(np.uint32)[np.isnan(want)] = NAN32
        assert same_bits(got["average"], want)
        assert same_bits(got["minimum"], want) and same_bits(got["maximum"], want)
        # the sequential float64 sum of <= a few thousand steps is off by < 1e-12 relative
        length = distance_ref(words, stops)
        want = distance_of(stop, ncard, ndiag)
        reached = ~np.isnan(want)
        assert np.array_equal(np.isnan(length), ~reached)
        assert ulps_apart(length[reached], want[reached]).max() <= 1
        assert reached.mean() > 0.3


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_statistics_keep_their_order(kind):
    z = random_dem((60, 80), seed=7, nan=0.01)
    words = direction_ref(z)[0]
    rng = np.random.default_rng(3)                         # most pits are stops, some are not
    streams = (rng.random(z.shape) < 0.05) | (stops_of(words) & (rng.random(z.shape) < 0.8))
    dem = None if kind == "horizontal" else z
    average, low, high = (distance_ref(words, streams, dem, kind, s, 2.0, 3.0) for s in STATISTICS)
    finite = np.isfinite(average) & np.isfinite(low) & np.isfinite(high)
    assert finite.sum() > 0.2 * z.size
    assert (low[finite] <= average[finite]).all() and (average[finite] <= high[finite]).all()
    assert np.array_equal(np.isnan(average), np.isnan(high))
    assert not np.isnan(low[~np.isnan(average)]).any()
    assert np.isnan(average).sum() > np.isnan(low).sum() > 0
    for got in (average, low, high):
        assert (got.view(np.uint32)[np.isnan(got)] == NAN32).all()


def test_the_reference_refuses_what_the_operator_refuses():
    ok = dinf.pack(np.array([[0, 4, 4]]), np.array([[0, 0, 0]]))
    assert distance_ref(ok, stops_of(ok)).tolist() == [[0, 1, 2]]
    bad = ok.copy()
    bad[0, 2] = 9 << 16
    with pytest.raises(ValueError, match="invalid D-infinity word in 1 cells"):
        distance_ref(bad, stops_of(ok))
    with pytest.raises(ValueError, match="outside the raster in 1 cells"):
        distance_ref(dinf.pack(np.array([[0, 0, 1]]), np.array([[0, 0, 0]])), stops_of(ok))
    loop = dinf.pack(np.array([[1, 4, 4]]), np.array([[0, 0, 0]]))
    with pytest.raises(ValueError, match="3 cells never resolve"):
        distance_ref(loop, np.zeros((1, 3), bool))
    # a stop cell cuts the cycle, whatever its word
    assert distance_ref(loop, np.array([[False, True, False]])).tolist() == [[1, 0, 1]]


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    from hydrodem_amd.filters import custom_filters
    for name in ("DInfDistanceDown", "DInfHeightAboveDrainage", "DemToDInfHAND"):
        assert getattr(hd, name) is getattr(custom_filters, name)
        assert issubclass(getattr(hd, name), hd.Filter)
    f = hd.DInfDistanceDown()
    assert f.kind == "horizontal" and f.statistic == "average" and f.stats == {}
    assert f.streams is None and f.dem is None and f.threshold is None
    hand = hd.DInfHeightAboveDrainage(dem=np.zeros((2, 2), F32), streams=np.zeros((2, 2), bool))
    assert hand.kind == "vertical" and hand.statistic == "average"
    assert hand.streams.dtype == np.uint8
    chain = hd.DemToDInfHAND(threshold=30)
    assert chain.flats == "keep" and chain.words is None and chain.stats == {}
    assert chain.statistic == "average" and chain.filters[0].epsilon == 1e-3
    assert [type(m).__name__ for m in chain.filters] == [
        "SinkFill", "D8FlowDirection", "FlowAccumulation", "DInfFlowDirection"]


def test_every_refusal_comes_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    words = np.zeros((4, 5), np.uint32)
    z = np.zeros((4, 5), F32)
    acc = np.ones((4, 5), np.uint32)

    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    assert said(lambda: hd.DInfDistanceDown().apply(words.astype(np.uint8))) == \
        "D-infinity distance down takes uint32 D-infinity words, got uint8"
    assert said(lambda: hd.DInfDistanceDown().apply(np.zeros((2, 4, 5), np.uint32))) == \
        "D-infinity distance down takes a 2-D raster, got 3 dimensions"
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.DInfDistanceDown().apply([[0]])
    assert said(lambda: dinf.dinfdist_args(None)) == \
        "D-infinity distance down needs the words it follows"
    assert said(lambda: dinf.dinfdist([[0]])) == "words is a NumPy array, got <class 'list'>"
    assert said(lambda: hd.DInfDistanceDown(kind="slope")) == \
        "kind is one of ['horizontal', 'vertical', 'surface'], got 'slope'"
    assert said(lambda: hd.DInfDistanceDown(statistic="median")) == \
        "statistic is one of ['average', 'minimum', 'maximum'], got 'median'"
    assert said(lambda: hd.DInfDistanceDown(statistic=0)) == \
        "statistic is one of ['average', 'minimum', 'maximum'], got 0"
    # a missing or surplus dem
    assert said(lambda: hd.DInfDistanceDown(kind="vertical")) == \
        "the vertical distance needs the dem it is measured on"
    assert said(lambda: hd.DInfDistanceDown(kind="surface")) == \
        "the surface distance needs the dem it is measured on"
    assert said(lambda: hd.DInfDistanceDown(dem=z)) == "the horizontal distance takes no dem"
    assert said(lambda: hd.DInfDistanceDown(kind="vertical", dem=z.astype(np.float64))) == \
        "dem has dtype float32, got float64"
    assert said(lambda: hd.DInfDistanceDown(kind="vertical", dem=z[:3]).apply(words)) == \
        "the dem is (3, 5), the words (4, 5)"
    assert said(lambda: dinf.dinfdist(words, dem=z.astype(np.float64), kind="vertical")) == \
        "the dem is float32, got float64"
    # the stop set
    assert said(lambda: hd.DInfDistanceDown(threshold=3)) == \
        "a threshold needs the uint32 raster it applies to"
    assert said(lambda: hd.DInfDistanceDown(streams=acc > 0, threshold=3)) == \
        "a uint8 stream mask takes no threshold"
    assert said(lambda: hd.DInfDistanceDown(streams=acc)) == \
        "a uint32 stream raster needs a threshold"
    for bad in (0, -1, 1.5, True, 2 ** 32):
        assert said(lambda: hd.DInfDistanceDown(streams=acc, threshold=bad)) == \
            f"threshold is an integer in 1 ... 2^32 - 1, got {bad!r}"
    assert said(lambda: hd.DInfDistanceDown(streams=acc.astype(np.int32), threshold=3)) == \
        "streams has dtype bool or uint8 or uint32, got int32"
    assert said(lambda: dinf.dinfdist(words, acc.astype(np.int32), 3)) == \
        "streams are a uint8 mask or a uint32 raster with a threshold, got int32"
    assert said(lambda: hd.DInfDistanceDown(streams=acc[:, :4], threshold=3).apply(words)) == \
        "streams are (4, 4), the words (4, 5)"
    # the cell
    assert said(lambda: hd.DInfDistanceDown(cellsize=0)) == \
        "cellsize must be finite and positive, got 0.0"
    assert said(lambda: hd.DInfDistanceDown(cellsize=(30.0, float("nan")))) == \
        "cellsize must be finite and positive, got nan"
    assert said(lambda: hd.DInfDistanceDown(cellsize=(1, 2, 3))) == \
        "cellsize is a number or a (dx, dy) pair, got (1, 2, 3)"

    class Huge:                                            # pylint: disable=too-few-public-methods
        dtype, shape = np.dtype(np.uint32), (65536, 65536)
    assert said(lambda: dinf.dinfdist_args(Huge())) == \
        "D-infinity distance down works in uint32: 65536 x 65536 cells is more than 2^32 - 1"
    # the two that wrap it
    assert said(lambda: hd.DInfHeightAboveDrainage(dem=None, streams=acc > 0)) == \
        "DInfHeightAboveDrainage needs the dem it is measured on"
    assert said(lambda: hd.DInfHeightAboveDrainage(dem=z, streams=None)) == \
        "DInfHeightAboveDrainage needs streams (a mask, or a uint32 raster with a threshold)"
    assert said(lambda: hd.DemToDInfHAND(threshold=0)) == \
        "threshold is an integer in 1 ... 2^32 - 1, got 0"
    assert said(lambda: hd.DemToDInfHAND(threshold=None)) == \
        "a uint32 stream raster needs a threshold"
    assert said(lambda: hd.DemToDInfHAND(threshold=30, flats="fill")) == \
        "flats is 'keep' or 'resolve', got 'fill'"
    assert said(lambda: hd.DemToDInfHAND(threshold=30, statistic="mean")) == \
        "statistic is one of ['average', 'minimum', 'maximum'], got 'mean'"
    assert said(lambda: hd.DemToDInfHAND(threshold=30, cellsize=-1)) == \
        "cellsize must be finite and positive, got -1.0"
    assert said(lambda: hd.DemToDInfHAND(threshold=30).apply(z.astype(np.float64))) == \
        "DemToDInfHAND takes a float32 DEM, got float64"
    assert said(lambda: hd.DemToDInfHAND(threshold=30).apply(np.zeros((2, 4, 5), F32))) == \
        "DemToDInfHAND takes a 2-D raster, got 3 dimensions"


def test_the_header_declares_the_entry_point_and_the_binding_mirrors_it(built):
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "A26  DInfDistanceDown.apply" in header
    args = re.search(r"int hdem_dinfdist_u32\((.*?)\);", header, re.S).group(1)
    assert len(args.split(",")) == 15 == len(backend.SIGNATURES["hdem_dinfdist_u32"])
    assert "hdem_dinfdist_u32_dev" not in header
    assert "hdem_dinfdist_u32_dev" not in backend.SIGNATURES
    struct = re.search(r"typedef struct hdem_dinfdist_stats \{(.*?)\} hdem_dinfdist_stats;",
                       header, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    declared = [n for pair in names for n in pair if n]
    stats = backend._DInfDistStats                          # pylint: disable=protected-access
    assert declared == [name for name, _ in stats._fields_]
    assert ctypes.sizeof(stats) == 96 and "hdem_dinfdist_stats;       /* sizeof == 96 */" in header
    for name, value in (("HDEM_DD_HORIZONTAL", 0), ("HDEM_DD_VERTICAL", 1), ("HDEM_DD_SURFACE", 2),
                        ("HDEM_DD_AVERAGE", 0), ("HDEM_DD_MINIMUM", 1), ("HDEM_DD_MAXIMUM", 2)):
        assert re.search(rf"#define {name} {value}\b", header)
    assert dinf.DIST_KINDS == {"horizontal": 0, "vertical": 1, "surface": 2}
    assert dinf.DIST_STATISTICS == {"average": 0, "minimum": 1, "maximum": 2}
    assert dinf.ON_DEVICE == 0x40000000 and "#define HDEM_ON_DEVICE 0x40000000" in header
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "hdem_dinfdist.hip" in makefile
    # a null context is BAD_ARG, whatever else is passed
    lib = backend.load_library()
    rc = lib.hdem_dinfdist_u32(*[t() for t in backend.SIGNATURES["hdem_dinfdist_u32"]])
    assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
