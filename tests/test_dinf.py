"""
D-infinity flow direction and accumulation (``DInfFlowDirection``, ``DInfFlowAccumulation``,
``DemToDInfArea``, ``hdem_dinf_f32``, ``hdem_dinfacc_u32``): the CPU half.

The host references live here and are used by tests/test_gpu_dinf.py.  They transcribe blocks
A20 and A21 of include/hydrodem_hip.h:
  ``direction_ref``   the eight facets as eight slices of the raster, float64 on the float32
                      elevations, the first strictly steepest facet wins;
  ``accumulate_ref``  Kahn's order: the cells whose donors are all done, one frontier at a
                      time, int64 throughout;
  ``accumulate_walk`` the same pull by plain recursion, cell by cell -- tiny grids.
No GPU here: the references hold the definition on written-out answers, agree with each other
and with the D8 reference on canonical words, conserve every unit, and the operators are
importable and refuse what they must before a device is touched.
"""
import math
import os
import re

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, dinf
from hydrodem_amd.dinf import FACETS, Q_ONE
from test_flowacc import acc_kahn, random_acyclic_codes, terminal_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def direction_ref(dem, dx=1.0, dy=1.0, fallback=None):
    """(words uint32, angle float64, slope float32, fallback cells) of block A20."""
    z = np.asarray(dem, F32)
    h, w = z.shape
    words = np.zeros((h, w), np.uint32)
    angle = np.full((h, w), -1.0)
    slope = np.zeros((h, w), np.float64)
    if h >= 3 and w >= 3:
        e0 = z[1:-1, 1:-1].astype(np.float64)
        best = np.zeros(e0.shape)
        facet = np.zeros(e0.shape, np.uint32)
        q_best = np.zeros(e0.shape, np.uint32)
        a_best = np.full(e0.shape, -1.0)
        with np.errstate(all="ignore"):
            for k, ((y1, x1), (y2, x2), ac, af) in FACETS.items():
                e1 = z[1 + y1:h - 1 + y1, 1 + x1:w - 1 + x1].astype(np.float64)
                e2 = z[1 + y2:h - 1 + y2, 1 + x2:w - 1 + x2].astype(np.float64)
                d1, d2 = (dx, dy) if y1 == 0 else (dy, dx)
                theta = math.atan2(d2, d1)
                s1 = (e0 - e1) / d1
                s2 = (e1 - e2) / d2
                card = s2 <= 0
                diag = ~card & (s2 * d1 >= s1 * d2)
                s = np.where(card, s1, np.where(diag, (e0 - e2) / math.sqrt(d1 * d1 + d2 * d2),
                                                np.sqrt(s1 * s1 + s2 * s2)))
                r = np.where(card, 0.0, np.where(diag, theta, np.arctan2(s2, s1)))
                wins = ~np.isnan(e0) & ~np.isnan(e1) & ~np.isnan(e2) & (s > best)
                q = np.where(card, 0.0, np.where(diag, float(Q_ONE),
                                                 np.rint(r / theta * 32768.0)))
                a = af * r + ac * (math.pi / 2)
                a = np.where(a >= 2 * math.pi, 0.0, a)
                best = np.where(wins, s, best)
                facet = np.where(wins, np.uint32(k), facet)
                q_best = np.where(wins, np.where(wins, q, 0.0).astype(np.uint32), q_best)
                a_best = np.where(wins, a, a_best)
        words[1:-1, 1:-1] = (facet << np.uint32(16)) | q_best
        angle[1:-1, 1:-1] = a_best
        slope[1:-1, 1:-1] = best
    taken = np.zeros((h, w), bool)
    if fallback is not None:
        fallback = np.asarray(fallback, np.uint8)
        taken = (words == 0) & (fallback != 0)
        words = np.where(taken, dinf.words_from_d8(fallback), words)
        eighths = np.zeros(256)
        for code, n in dinf.D8_EIGHTHS.items():
            eighths[code] = n
        angle = np.where(taken, eighths[fallback] * (math.pi / 4), angle)
    with np.errstate(over="ignore"):
        slope = np.where(np.isnan(z), np.nan, slope).astype(F32)
    return words, angle, slope, int(taken.sum())


def receivers(words):
    """Flat index of the cardinal and of the diagonal receiver of every cell (-1: none), after
    the checks of block A21: ValueError with the count for invalid words and for receivers
    outside the raster."""
    words = np.asarray(words, np.uint32)
    h, w = words.shape
    facet, q = (words >> 16) & 15, (words & 0xFFFF).astype(np.int64)
    bad = (words >> 20 != 0) | (facet > 8) | (q > Q_ONE) | ((facet == 0) & (q != 0))
    if bad.any():
        raise ValueError(f"invalid D-infinity word in {int(bad.sum())} cells")
    ys, xs = np.mgrid[0:h, 0:w]
    card = np.full((h, w), -1, np.int64)
    diag = np.full((h, w), -1, np.int64)
    outside = np.zeros((h, w), bool)
    for k, ((y1, x1), (y2, x2), _, _) in FACETS.items():
        for (dy, dx), gives, into in (((y1, x1), q != Q_ONE, card), ((y2, x2), q != 0, diag)):
            m = (facet == k) & gives
            ny, nx = ys + dy, xs + dx
            inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
            outside |= m & ~inside
            into[m & inside] = (ny * w + nx)[m & inside]
    if outside.any():
        raise ValueError(f"D-infinity words send flow outside the raster in {int(outside.sum())} "
                         "cells")
    return card.ravel(), diag.ravel(), q.ravel()


def accumulate_ref(words, frac_bits=16):
    """int64 ``A`` of block A21 in Kahn's order; ValueError "N cells never resolve" on a cycle."""
    words = np.asarray(words, np.uint32)
    card, diag, q = receivers(words)
    n = words.size
    indeg = np.bincount(card[card >= 0], minlength=n) + np.bincount(diag[diag >= 0], minlength=n)
    acc = np.full(n, 1 << frac_bits, np.int64)
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        to_diag = (acc[frontier] * q[frontier]) >> 15
        to_card = acc[frontier] - to_diag
        woken = []
        for rec, share in ((diag[frontier], to_diag), (card[frontier], to_card)):
            has = rec >= 0
            np.add.at(acc, rec[has], share[has])
            np.subtract.at(indeg, rec[has], 1)
            woken.append(rec[has])
        woken = np.unique(np.concatenate(woken))
        frontier = woken[indeg[woken] == 0]
    if done != n:
        raise ValueError(f"D-infinity words form a cycle: {n - done} cells never resolve")
    return acc.reshape(words.shape)


def accumulate_walk(words, frac_bits=16):
    """The same pull, cell by cell with memoised recursion (tiny acyclic grids)."""
    words = np.asarray(words, np.uint32)
    h, w = words.shape
    memo = {}

    def area(y, x):
        if (y, x) not in memo:
            total = 1 << frac_bits
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if (dy or dx) and 0 <= ny < h and 0 <= nx < w and words[ny, nx] >> 16:
                        facet, q = int(words[ny, nx] >> 16), int(words[ny, nx] & 0xFFFF)
                        e1, e2, _, _ = FACETS[facet]
                        if e2 == (-dy, -dx) and q:
                            total += (area(ny, nx) * q) >> 15
                        if e1 == (-dy, -dx) and q != Q_ONE:
                            total += area(ny, nx) - ((area(ny, nx) * q) >> 15)
            memo[y, x] = total
        return memo[y, x]

    return np.array([[area(y, x) for x in range(w)] for y in range(h)], np.int64)


def value_of(acc, frac_bits=16):
    """The float32 ``value`` output of an int64 ``sum``."""
    return (acc.astype(np.float64) * 2.0 ** -frac_bits).astype(F32)


def counts_of(words):
    """The stats of the accumulation that do not depend on the schedule."""
    q = words & 0xFFFF
    return {"split_cells": int(((q != 0) & (q != Q_ONE)).sum()),
            "terminal_cells": int((words >> 16 == 0).sum()),
            "invalid": 0, "outside": 0, "unresolved": 0, "tile_h": 64, "tile_w": 64}


def plane(shape, east, north, dx=1.0, dy=1.0):
    """A float32 plane that drops by ``east`` per unit eastwards and ``north`` northwards."""
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]]
    return (-(east * cols * dx - north * rows * dy)).astype(F32)


def random_dem(shape, seed, nan=0.0):
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:shape[0], 0:shape[1]]
    z = (rng.random(shape) * 3 + 0.05 * rows + 0.02 * cols).astype(F32)
    if nan:
        z[rng.random(shape) < nan] = np.nan
    return z


# ---------------------------------------------------------------------------
# the definition on written-out answers
# ---------------------------------------------------------------------------
def test_a_plane_tilted_east_takes_the_first_of_the_two_tied_facets():
    words, angle, slope, _ = direction_ref(plane((6, 7), 1.0, 0.0))
    facet, q = dinf.unpack(words)
    assert (facet[1:-1, 1:-1] == 1).all() and not q.any()          # 1 and 8 tie: the first
    assert (angle[1:-1, 1:-1] == 0).all() and (slope[1:-1, 1:-1] == 1).all()
    ring = np.ones((6, 7), bool)
    ring[1:-1, 1:-1] = False
    assert not words[ring].any() and (angle[ring] == -1).all() and not slope[ring].any()
    # westwards: facets 4 and 5 tie, and pi is pi
    words, angle, _, _ = direction_ref(plane((5, 5), -1.0, 0.0))
    assert (dinf.unpack(words)[0][1:-1, 1:-1] == 4).all()
    assert (angle[1:-1, 1:-1] == math.pi).all()
    # south: facets 6 and 7; just short of east from below: facet 8, the angle below 2 pi
    assert (dinf.unpack(direction_ref(plane((5, 5), 0.0, -1.0))[0])[0][1:-1, 1:-1] == 6).all()
    words, angle, _, _ = direction_ref(plane((5, 5), 1.0, -0.25))
    facet, q = dinf.unpack(words)
    assert (facet[1:-1, 1:-1] == 8).all()
    assert (q[1:-1, 1:-1] == round(math.atan2(0.25, 1.0) / (math.pi / 4) * 32768)).all()
    assert np.allclose(angle[1:-1, 1:-1], 2 * math.pi - math.atan2(0.25, 1.0), rtol=0, atol=1e-15)


def test_a_plane_towards_22_5_degrees_splits_every_area_in_halves():
    theta = math.pi / 8
    z = plane((7, 8), math.cos(theta), math.sin(theta))
    words, angle, slope, _ = direction_ref(z)
    facet, q = dinf.unpack(words)
    assert (facet[1:-1, 1:-1] == 1).all() and (q[1:-1, 1:-1] == 16384).all()
    assert np.allclose(angle[1:-1, 1:-1], theta, rtol=0, atol=1e-5)
    assert np.allclose(slope[1:-1, 1:-1], 1.0, rtol=0, atol=1e-5)
    for frac_bits in (0, 16):
        acc = accumulate_ref(words, frac_bits)
        assert np.array_equal(acc, accumulate_walk(words, frac_bits))
        unit = 1 << frac_bits
        want = np.full(z.shape, unit, np.int64)
        for x in range(1, 7):                            # west to east, north to south ...
            for y in range(5, 0, -1):                    # ... is upstream first
                half = want[y, x] >> 1
                want[y - 1, x + 1] += half               # NE
                want[y, x + 1] += want[y, x] - half      # E: the odd unit stays cardinal
        assert np.array_equal(acc, want)
        assert int(acc[words == 0].sum()) == z.size * unit


def test_a_five_by_five_cone():
    rows, cols = np.mgrid[0:5, 0:5]
    z = (-np.hypot(rows - 2, cols - 2)).astype(F32)
    words, angle, slope, _ = direction_ref(z)
    facet, q = dinf.unpack(words)
    assert not words[0].any() and not words[-1].any() and not words[:, 0].any()
    # the summit: eight equal facets, the first wins, and tan(pi / 8) = sqrt 2 - 1
    assert facet[2, 2] == 1 and q[2, 2] == 16384
    assert abs(angle[2, 2] - math.pi / 8) < 1e-7
    # east of it: facets 1 and 8 tie at atan((sqrt 5 - 2) / 1)
    low = float(F32(math.sqrt(5))) - 2.0
    assert facet[2, 3] == 1 and q[2, 3] == round(math.atan2(low, 1.0) / (math.pi / 4) * 32768)
    assert slope[2, 3] == F32(math.sqrt(1.0 + low * low))
    # north-east of it: facets 1 and 2 tie on either side of the diagonal, short of it
    s1 = float(F32(math.sqrt(5))) - float(F32(math.sqrt(2)))
    s2 = float(F32(math.sqrt(8))) - float(F32(math.sqrt(5)))
    assert facet[1, 3] == 1 and q[1, 3] == round(math.atan2(s2, s1) / (math.pi / 4) * 32768)
    assert angle[1, 3] == math.atan2(s2, s1) and slope[1, 3] == F32(math.sqrt(s1 * s1 + s2 * s2))
    # the other six of the ring by the same two patterns, turned
    assert facet[1:4, 1:4].tolist() == [[3, 2, 1], [4, 1, 1], [5, 6, 7]]
    assert q[1, 1] == q[3, 1] == q[3, 3] == q[1, 3] and q[1, 2] == q[2, 1] == q[3, 2] == q[2, 3]
    acc = accumulate_ref(words)
    assert np.array_equal(acc, accumulate_walk(words))
    assert acc[2, 2] == 1 << 16 and int(acc[words == 0].sum()) == 25 << 16
    assert acc[2, 3] == (1 << 16) + (1 << 15)            # the summit's cardinal half


def test_cells_that_are_not_square():
    dx, dy = 30.0, 10.0
    # straight along the cell's diagonal: s2 * d1 == s1 * d2, everything to NE
    words, angle, slope, _ = direction_ref(plane((5, 6), 3.0, 1.0, dx, dy), dx, dy)
    facet, q = dinf.unpack(words)
    assert (facet[1:-1, 1:-1] == 1).all() and (q[1:-1, 1:-1] == Q_ONE).all()
    assert (angle[1:-1, 1:-1] == math.atan2(10, 30)).all()
    assert (slope[1:-1, 1:-1] == F32(math.sqrt(10))).all()
    # half as far north: between E and NE, measured against the cell's own diagonal
    words, angle, slope, _ = direction_ref(plane((5, 6), 3.0, 0.5, dx, dy), dx, dy)
    facet, q = dinf.unpack(words)
    r = math.atan2(0.5, 3.0)
    assert (facet[1:-1, 1:-1] == 1).all()
    assert (q[1:-1, 1:-1] == round(r / math.atan2(10, 30) * 32768)).all()
    assert (angle[1:-1, 1:-1] == r).all() and (slope[1:-1, 1:-1] == F32(math.sqrt(9.25))).all()
    # north: d1 is dy there; north-north-east is facet 2, measured from north
    words, angle, slope, _ = direction_ref(plane((5, 6), 0.0, 2.0, dx, dy), dx, dy)
    assert (dinf.unpack(words)[0][1:-1, 1:-1] == 2).all() and (slope[1:-1, 1:-1] == 2).all()
    assert (angle[1:-1, 1:-1] == math.pi / 2).all()
    words, angle, _, _ = direction_ref(plane((5, 6), 1.0, 2.0, dx, dy), dx, dy)
    facet, q = dinf.unpack(words)
    r = math.atan2(1.0, 2.0)
    assert (facet[1:-1, 1:-1] == 2).all()
    assert (q[1:-1, 1:-1] == round(r / math.atan2(30, 10) * 32768)).all()
    assert (angle[1:-1, 1:-1] == -r + math.pi / 2).all()
    # the angle the words stand for is the unquantised one to 15 bits
    assert np.allclose(dinf.angle_of(words, dx, dy), angle, rtol=0, atol=math.pi / 2 / 32768)


def test_nodata_flats_and_the_fallback():
    z = plane((6, 6), 1.0, 0.0)
    z[2, 3] = np.nan
    words, angle, slope, _ = direction_ref(z)
    facet = dinf.unpack(words)[0]
    assert words[2, 3] == 0 and angle[2, 3] == -1 and np.isnan(slope[2, 3])
    # west of it: east is nodata, so round it by the diagonal, facet 2 first
    assert facet[2, 2] == 2 and words[2, 2] & 0xFFFF == Q_ONE
    assert slope[2, 2] == F32(1 / math.sqrt(2)) and angle[2, 2] == math.pi / 2 - math.pi / 4
    assert facet[1, 2] == 1 and facet[3, 2] == 8         # facets with a NaN corner are skipped
    flat = np.full((4, 5), 7, F32)
    codes = np.zeros((4, 5), np.uint8)
    codes[1, 1:4], codes[2, 1:4] = (1, 128, 64), (2, 4, 8)
    words, angle, slope, taken = direction_ref(flat, fallback=codes)
    assert taken == 6 and not slope.any()
    assert np.array_equal(words, dinf.words_from_d8(codes))
    assert dinf.unpack(words)[0][1:3, 1:4].tolist() == [[1, 1, 2], [7, 6, 5]]
    assert dinf.unpack(words)[1][1:3, 1:4].tolist() == [[0, Q_ONE, 0], [Q_ONE, 0, Q_ONE]]
    assert angle[1, 1:4].tolist() == [0, math.pi / 4, math.pi / 2]
    assert angle[2, 1:4].tolist() == [7 * (math.pi / 4), 6 * (math.pi / 4), 5 * (math.pi / 4)]
    # a cell with a way down keeps it
    words, _, _, taken = direction_ref(plane((5, 5), 1.0, 0.0), fallback=np.full((5, 5), 4, np.uint8))
    assert taken == 16 and (dinf.unpack(words)[0][1:-1, 1:-1] == 1).all()


# ---------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (3, 3), (17, 23), (40, 31)])
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_every_unit_arrives_at_a_terminal(shape, frac_bits):
    z = random_dem(shape, seed=shape[0] * 100 + shape[1], nan=0.02)
    words, _, _, _ = direction_ref(z)
    acc = accumulate_ref(words, frac_bits)
    assert int(acc[words >> 16 == 0].sum()) == z.size << frac_bits
    assert acc.min() >= 1 << frac_bits
    if z.size <= 400:
        assert np.array_equal(acc, accumulate_walk(words, frac_bits))
    counts = counts_of(words)
    assert counts["split_cells"] + counts["terminal_cells"] <= z.size
    assert shape[0] < 17 or counts["split_cells"] > 0.1 * z.size


@pytest.mark.parametrize("shape,ramp", [((1, 1), False), ((9, 14), False), ((40, 70), True)])
def test_canonical_words_reproduce_d8(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=3, ramp=ramp)
    # the D8 reference lets a code point outside; a word may not
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    words = dinf.words_from_d8(codes)
    for frac_bits in (0, 5, 16):
        assert np.array_equal(accumulate_ref(words, frac_bits), acc_kahn(codes) << frac_bits)
    assert np.array_equal(dinf.angle_of(words) >= 0, codes != 0)


def test_pack_and_unpack_round_trip():
    rng = np.random.default_rng(1)
    facet = rng.integers(0, 9, (30, 40))
    q = np.where(facet == 0, 0, rng.integers(0, Q_ONE + 1, (30, 40)))
    words = dinf.pack(facet, q)
    assert words.dtype == np.uint32 and not (words >> 20).any()
    got_facet, got_q = dinf.unpack(words)
    assert np.array_equal(got_facet, facet) and np.array_equal(got_q, q)
    assert dinf.pack(8, Q_ONE) == (8 << 16) | Q_ONE
    for bad_facet, bad_q in ((9, 0), (-1, 0), (1, Q_ONE + 1), (0, 1)):
        with pytest.raises(ValueError):
            dinf.pack(bad_facet, bad_q)
    with pytest.raises(ValueError, match="uint32"):
        dinf.unpack(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        dinf.words_from_d8(np.array([[3, 1, 255]], np.uint8))


def test_the_reference_refuses_what_the_operator_refuses():
    ok = dinf.pack(np.array([[0, 1, 0]]), np.array([[0, 0, 0]]))
    assert accumulate_ref(ok).tolist() == [[1 << 16, 1 << 16, 2 << 16]]
    for word in (9 << 16, (1 << 16) | (Q_ONE + 1), 5, 1 << 20, 1 << 31):
        bad = ok.copy()
        bad[0, 0] = word
        with pytest.raises(ValueError, match="invalid D-infinity word in 1 cells"):
            accumulate_ref(bad)
    with pytest.raises(ValueError, match="outside the raster in 1 cells"):
        accumulate_ref(dinf.pack(np.array([[0, 0, 1]]), np.array([[0, 0, 0]])))
    with pytest.raises(ValueError, match="outside the raster in 2 cells"):   # NE of a single row
        accumulate_ref(dinf.pack(np.array([[1, 0, 1]]), np.array([[1, 0, Q_ONE]])))
    loop = dinf.pack(np.array([[1, 4, 0]]), np.array([[0, 0, 0]]))
    with pytest.raises(ValueError, match="2 cells never resolve"):
        accumulate_ref(loop)


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    from hydrodem_amd.filters import custom_filters
    for name in ("DInfFlowDirection", "DInfFlowAccumulation", "DemToDInfArea"):
        assert getattr(hd, name) is getattr(custom_filters, name)
        assert issubclass(getattr(hd, name), hd.Filter)
    f = hd.DInfFlowDirection()
    assert f.stats == {} and f.angle is None and f.slope is None
    assert f.keep_partial_results is False and f.fallback is None
    a = hd.DInfFlowAccumulation()
    assert a.frac_bits == 16 and a.output == "value" and a.dtype == np.float32
    assert hd.DInfFlowAccumulation(output="sum").dtype == np.int64
    chain = hd.DemToDInfArea()
    assert chain.flats == "keep" and chain.words is None and chain.stats == {}
    assert [type(m).__name__ for m in chain.filters] == [
        "SinkFill", "D8FlowDirection", "DInfFlowDirection", "DInfFlowAccumulation"]
    assert chain.filters[0].epsilon == 1e-3
    assert not [n for n in backend.__all__ if "dinf" in n.lower()]


def test_every_refusal_comes_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    z = np.zeros((4, 5), F32)
    words = np.zeros((4, 5), np.uint32)

    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    # the direction
    assert said(lambda: hd.DInfFlowDirection().apply(z.astype(np.float64))) == \
        "D-infinity flow direction takes a float32 DEM, got float64"
    assert said(lambda: hd.DInfFlowDirection().apply(np.zeros((2, 4, 5), F32))) == \
        "D-infinity flow direction takes a 2-D raster, got 3 dimensions"
    assert said(lambda: hd.DInfFlowDirection().apply(np.zeros(4, F32))) == \
        "D-infinity flow direction takes a 2-D raster, got 1 dimensions"
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.DInfFlowDirection().apply([[0.0]])
    assert said(lambda: hd.DInfFlowDirection(cellsize=0)) == \
        "cellsize must be finite and positive, got 0.0"
    assert said(lambda: hd.DInfFlowDirection(cellsize=(30.0, float("inf")))) == \
        "cellsize must be finite and positive, got inf"
    assert said(lambda: hd.DInfFlowDirection(cellsize="wide")) == \
        "cellsize is a number, got 'wide'"
    assert said(lambda: hd.DInfFlowDirection(cellsize=(1, 2, 3))) == \
        "cellsize is a number or a (dx, dy) pair, got (1, 2, 3)"
    assert said(lambda: hd.DInfFlowDirection(fallback=np.zeros((4, 5), np.uint32))) == \
        "fallback has dtype uint8, got uint32"
    assert said(lambda: hd.DInfFlowDirection(fallback=[[0]])) == \
        "fallback is a NumPy array or a DeviceRaster, got <class 'list'>"
    assert said(lambda: hd.DInfFlowDirection(fallback=np.zeros((3, 5), np.uint8)).apply(z)) == \
        "the fallback is (3, 5), the dem (4, 5)"
    assert said(lambda: dinf.dinf(z, fallback=np.zeros((4, 5), np.int8))) == \
        "the fallback is uint8 D8 codes, got int8"
    assert said(lambda: dinf.dinf(z, want=("aspect",))) == \
        "unknown D-infinity outputs ['aspect']: choose among ['angle', 'slope']"
    assert said(lambda: dinf.dinf(None)) == \
        "D-infinity flow direction needs the dem it is derived from"
    # the accumulation
    assert said(lambda: hd.DInfFlowAccumulation().apply(words.astype(np.uint8))) == \
        "D-infinity flow accumulation takes uint32 D-infinity words, got uint8"
    assert said(lambda: hd.DInfFlowAccumulation().apply(np.zeros((2, 4, 5), np.uint32))) == \
        "D-infinity flow accumulation takes a 2-D raster, got 3 dimensions"
    for bad in (-1, 17, 1.5, True, None):
        assert said(lambda: hd.DInfFlowAccumulation(frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 16, got {bad!r}"
        assert said(lambda: hd.DemToDInfArea(frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 16, got {bad!r}"
    assert said(lambda: hd.DInfFlowAccumulation(output="mask")) == \
        "output is one of ['sum', 'value'], got 'mask'"
    assert said(lambda: dinf.dinfacc(words, want=())) == \
        "no output wanted: choose among ['sum', 'value']"
    assert said(lambda: dinf.dinfacc(words, want=("area",))) == \
        "unknown D-infinity accumulation outputs ['area']: choose among ['sum', 'value']"
    assert said(lambda: dinf.dinfacc([[0]])) == "words is a NumPy array, got <class 'list'>"
    # the chain
    assert said(lambda: hd.DemToDInfArea(flats="fill")) == \
        "flats is 'keep' or 'resolve', got 'fill'"
    assert said(lambda: hd.DemToDInfArea(output="mask")) == \
        "output is one of ['sum', 'value'], got 'mask'"
    assert said(lambda: hd.DemToDInfArea(cellsize=-1)) == \
        "cellsize must be finite and positive, got -1.0"
    assert said(lambda: hd.DemToDInfArea().apply(z.astype(np.float64))) == \
        "DemToDInfArea takes a float32 DEM, got float64"
    assert said(lambda: hd.DemToDInfArea().apply(np.zeros((2, 4, 5), F32))) == \
        "DemToDInfArea takes a 2-D raster, got 3 dimensions"


def test_the_header_declares_both_pairs_and_the_binding_mirrors_them(built):
    import ctypes
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "A20  DInfFlowDirection.apply" in header and "A21  DInfFlowAccumulation.apply" in header
    for name, count in (("hdem_dinf_f32", 12), ("hdem_dinfacc_u32", 9)):
        host = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        dev = re.search(rf"int {name}_dev\((.*?)\);", header, re.S).group(1)
        assert " ".join(host.split()) == " ".join(dev.split())
        assert len(host.split(",")) == count
        assert len(backend.SIGNATURES[name]) == count
        assert backend.SIGNATURES[name] == backend.SIGNATURES[name + "_dev"]
    assert ctypes.sizeof(backend._DInfStats) == 24          # pylint: disable=protected-access
    assert ctypes.sizeof(backend._DInfAccStats) == 80       # pylint: disable=protected-access
    assert "sizeof == 24" in header and "hdem_dinfacc_stats;        /* sizeof == 80 */" in header
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "hdem_dinf.hip" in makefile
    # a null context is BAD_ARG, whatever else is passed
    lib = backend.load_library()
    for name in ("hdem_dinf_f32", "hdem_dinf_f32_dev", "hdem_dinfacc_u32", "hdem_dinfacc_u32_dev"):
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
