"""
Multiple-flow-direction flow direction and accumulation (``MFDFlowDirection``,
``MFDFlowAccumulation``, ``DemToMFDArea``, ``hdem_mfd_f32``, ``hdem_mfdacc_u64``): the CPU half.

The host references live here and are used by tests/test_gpu_mfd.py.  They transcribe blocks A24
and A25 of include/hydrodem_hip.h:
  ``pw``              the contract's power function, operation for operation;
  ``direction_ref``   the eight directions as eight slices of the NaN-padded raster, float64 on
                      the float32 elevations;
  ``accumulate_ref``  Kahn's order over the edges of the words, int64 throughout;
  ``accumulate_walk`` the same pull by plain recursion over Python integers -- tiny grids.
No GPU here: the references hold the definition on written-out answers, agree with each other
and with the D8 reference on canonical words, conserve every unit, and the operators are
importable and refuse what they must before a device is touched.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, dinf, mfd
from hydrodem_amd.mfd import DIRECTIONS, HAS_FLOW
from test_dinf import plane, random_dem, value_of            # noqa: F401  (value_of: the GPU half)
from test_flowacc import acc_kahn, random_acyclic_codes, terminal_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T_MIN = 2.0 ** -64


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def pw(t, e):
    """``pw(t, e)`` of block A24 on float64 arrays: every line is one line of the header."""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        m, k = np.frexp(t)
        low = m < 0.7071067811865476
        m = np.where(low, m * 2.0, m)
        k = np.where(low, k - 1, k)
        s = (m - 1.0) / (m + 1.0)
        s2 = s * s
        r = np.full(t.shape, 1.0 / 15.0)
        for n in (13, 11, 9, 7, 5, 3, 1):
            r = r * s2 + 1.0 / n
        l2 = k.astype(np.float64) + ((2.0 * s) * r) * 1.4426950408889634
        y = e * l2
        n = np.floor(y + 0.5)
        u = (y - n) * 0.6931471805599453
        p = np.ones(t.shape)
        for i in range(12, 1, -1):
            p = 1.0 + (u * p) * (1.0 / i)
        p = 1.0 + u * p
        return np.ldexp(p, np.where(np.isfinite(n), n, 0).astype(np.int32))


def direction_ref(dem, method="freeman", exponent=None, dx=1.0, dy=1.0, fallback=None):
    """(words uint64, slope float32, stats) of block A24; ValueError with the count for fallback
    bytes that are no D8 code."""
    exponent, w_card, w_diag = mfd.method_of(method, exponent)
    z = np.asarray(dem, F32)
    h, w = z.shape
    padded = np.full((h + 2, w + 2), np.nan)
    padded[1:-1, 1:-1] = z
    e0 = z.astype(np.float64)
    finite = np.isfinite(z)
    diag = math.sqrt(dx * dx + dy * dy)
    s = np.zeros((8, h, w))
    with np.errstate(all="ignore"):
        for d, (oy, ox) in enumerate(DIRECTIONS):
            zn = padded[1 + oy:h + 1 + oy, 1 + ox:w + 1 + ox]
            dist = diag if d & 1 else dy if d & 2 else dx
            drop = e0 - zn
            s[d] = np.where(finite & ~np.isnan(zn) & (drop > 0), drop / dist, 0.0)
        smax = s.max(axis=0)
        has = smax > 0
        t = np.where(s == smax, 1.0, s / smax)
        power = t if exponent == 1.0 else pw(t, exponent)
        c = np.array([w_diag if d & 1 else w_card for d in range(8)])[:, None, None]
        f = np.where((s > 0) & (t >= T_MIN), c * power, 0.0)
        main = np.argmax(f, axis=0)                        # the first of the greatest
        total = f[0]
        for d in range(1, 8):
            total = total + f[d]
        share = np.floor((256.0 * f) / total + 0.5)
    words = np.uint64(HAS_FLOW) | (main.astype(np.uint64) << np.uint64(56))
    for d in range(8):
        field = np.where(has & (main != d) & (f[d] > 0), share[d], 0.0).astype(np.uint64)
        where = ((d - main) & 7) - 1                       # -1 for the main one: its field is 0
        words = words | (field << (8 * np.maximum(where, 0)).astype(np.uint64))
    words = np.where(has, words, np.uint64(0))
    taken = np.zeros((h, w), bool)
    if fallback is not None:
        used = np.where(has, 0, np.asarray(fallback, np.uint8)).astype(np.uint8)
        taken = used != 0
        words = np.where(taken, mfd.words_from_d8(used), words)
    with np.errstate(over="ignore"):
        slope = np.where(np.isnan(z), np.nan, smax).astype(F32)
    stats = {"no_flow": int((words == 0).sum()), "fallback_cells": int(taken.sum()),
             "split_cells": int(((words & np.uint64((1 << 56) - 1)) != 0).sum())}
    return words, slope, stats


def edges(words):
    """(receiver flat index by direction (n, 8), -1 outside; shares (n, 8) in 2^-8 units with
    the main one filled in; main (n,)) after the checks of block A25: ValueError with the count
    for invalid words and for receivers outside the raster."""
    words = np.asarray(words, np.uint64)
    h, w = words.shape
    bad = mfd.invalid(words)
    if bad.any():
        raise ValueError(f"invalid MFD word in {int(bad.sum())} cells")
    shares = mfd.shares_of(words).reshape(h * w, 8)
    ys, xs = np.mgrid[0:h, 0:w]
    rec = np.full((h * w, 8), -1, np.int64)
    for d, (oy, ox) in enumerate(DIRECTIONS):
        ny, nx = ys + oy, xs + ox
        inside = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        rec[:, d] = np.where(inside, ny * w + nx, -1).ravel()
    outside = ((shares > 0) & (rec < 0)).any(axis=1)
    if outside.any():
        raise ValueError(f"MFD words send flow outside the raster in {int(outside.sum())} cells")
    return rec, shares, mfd.unpack(words)[1].ravel().astype(np.int64)


def own_terms(words, weights=None, frac_bits=16):
    """int64 own(c) of block A25 after A22's checks of the weights."""
    if weights is None:
        return np.full(words.size, 1 << frac_bits, np.int64)
    weights = np.asarray(weights)
    refused = np.zeros(weights.shape, bool)
    if weights.dtype == F32:
        with np.errstate(invalid="ignore"):
            refused = (weights < 0) | np.isposinf(weights)
        weights = np.where(refused, F32(0), weights)
    q = dinf.quantise(weights, frac_bits)                   # a NaN counts 0
    off = int(refused.sum()) + int((q > 2 ** 31 - 1).sum())
    if off:
        raise ValueError(f"weights out of range in {off} cells")
    if int(q.sum()) >= 2 ** 48:
        raise ValueError(f"the quantised weights sum to {int(q.sum())}")
    return q.ravel().astype(np.int64)


def accumulate_ref(words, weights=None, frac_bits=16):
    """int64 ``A`` of block A25 in Kahn's order; ValueError "N cells never resolve" on a cycle."""
    words = np.asarray(words, np.uint64)
    rec, shares, main = edges(words)
    acc = own_terms(words, weights, frac_bits)
    n = words.size
    gives = shares > 0
    indeg = np.bincount(rec[gives], minlength=n)
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        a = acc[frontier]
        sent = np.zeros(frontier.size, np.int64)
        woken = []
        for d in range(8):
            side = gives[frontier, d] & (main[frontier] != d)
            amount = (a[side] * shares[frontier[side], d]) >> 8
            sent[side] += amount
            np.add.at(acc, rec[frontier[side], d], amount)
        for d in range(8):
            to_main = gives[frontier, d] & (main[frontier] == d)
            np.add.at(acc, rec[frontier[to_main], d], a[to_main] - sent[to_main])
            every = gives[frontier, d]
            np.subtract.at(indeg, rec[frontier[every], d], 1)
            woken.append(rec[frontier[every], d])
        woken = np.unique(np.concatenate(woken))
        frontier = woken[indeg[woken] == 0]
    if done != n:
        raise ValueError(f"MFD words form a cycle: {n - done} cells never resolve")
    return acc.reshape(words.shape)


def accumulate_walk(words, frac_bits=16):
    """The same pull, cell by cell with memoised recursion over Python integers, reading the
    bit fields of the word itself (tiny acyclic grids)."""
    words = np.asarray(words, np.uint64)
    h, w = words.shape
    memo = {}

    def sends(word, amount, toward):
        """What a cell with ``word`` and ``amount`` sends in direction ``toward``."""
        if not word:
            return 0
        m = (word >> 56) & 7
        fields = [(word >> (8 * j)) & 0xFF for j in range(7)]
        if toward != m:
            return (amount * fields[((toward - m) & 7) - 1]) >> 8
        return amount - sum((amount * p) >> 8 for p in fields)

    def names(word, toward):
        m = (word >> 56) & 7
        return bool(word) and (toward == m or ((word >> (8 * (((toward - m) & 7) - 1))) & 0xFF))

    def area(y, x):
        if (y, x) not in memo:
            total = 1 << frac_bits
            for d, (oy, ox) in enumerate(DIRECTIONS):
                ny, nx = y + oy, x + ox                    # the donor in direction d sends back
                if 0 <= ny < h and 0 <= nx < w and names(int(words[ny, nx]), (d + 4) & 7):
                    total += sends(int(words[ny, nx]), area(ny, nx), (d + 4) & 7)
            memo[y, x] = total
        return memo[y, x]

    return np.array([[area(y, x) for x in range(w)] for y in range(h)], np.int64)


def counts_of(words):
    """The stats of the accumulation that do not depend on the schedule."""
    return {"split_cells": int(((words & np.uint64((1 << 56) - 1)) != 0).sum()),
            "terminal_cells": int((words == 0).sum()),
            "invalid": 0, "outside": 0, "unresolved": 0, "tile_h": 64, "tile_w": 64}


def random_acyclic_words(shape, seed):
    """Words over a random priority raster: every receiver lies strictly lower, so no cycle.
    Every cell takes a random subset (1 ... 8, as many as there are) of its lower neighbours
    with random shares; a cell without a lower neighbour stays 0."""
    rng = np.random.default_rng(seed)
    h, w = shape
    p = np.full((h + 2, w + 2), np.iinfo(np.int64).max, np.int64)    # outside: never lower
    p[1:-1, 1:-1] = rng.permutation(h * w).reshape(h, w)
    here = p[1:-1, 1:-1]
    lower = np.stack([p[1 + oy:h + 1 + oy, 1 + ox:w + 1 + ox] < here for oy, ox in DIRECTIONS],
                     axis=-1)
    chosen = lower & (rng.random(shape + (8,)) < rng.random(shape + (1,)))
    first = np.argmax(lower, axis=-1)
    none = ~chosen.any(axis=-1) & lower.any(axis=-1)
    chosen[none, first[none]] = True                        # at least one where there is one
    flow = chosen.any(axis=-1)
    order = rng.random(shape + (8,))
    main = np.argmax(np.where(chosen, order, -1.0), axis=-1)
    cut = rng.integers(0, 37, shape + (8,))                 # 7 x 36 = 252 <= 255
    by_direction = np.where(chosen, cut, 0)
    shares = np.zeros(shape + (7,), np.int64)
    for j in range(1, 8):
        shares[..., j - 1] = np.take_along_axis(by_direction, ((main + j) & 7)[..., None],
                                                axis=-1)[..., 0]
    # a chosen receiver with share 0 is no receiver, unless it is the main one: the word says so
    return mfd.pack(flow, np.where(flow, main, 0), np.where(flow[..., None], shares, 0))


# ---------------------------------------------------------------------------
# the power function
# ---------------------------------------------------------------------------
def test_pw_is_within_1e_9_of_the_real_power():
    """A share is quantised in steps of 2^-9 of the total, so 1e-9 is far more than enough; the
    bound is the issue's, the grid covers t in [2^-64, 1] and e in [0.25, 16]."""
    t = np.concatenate([2.0 ** -np.linspace(0, 64, 1537), np.linspace(2.0 ** -64, 1.0, 1001),
                        [1.0, T_MIN, 0.5, 0.70710678118654746, 0.70710678118654757]])
    worst = 0.0
    for e in (0.25, 0.5, 1.0, 1.1, 2.0, 3.7, 4.0, 8.0, 15.99, 16.0):
        got = pw(t, e)
        want = np.array([math.pow(v, e) for v in t])
        usual = want > 1e-300                               # (the rest is subnormal)
        worst = max(worst, float(np.max(np.abs(got[usual] - want[usual]) / want[usual])))
        assert np.all(np.abs(got[~usual] - want[~usual]) <= 1e-9 * want[~usual] + 5e-324)
        assert pw(np.array([1.0]), e)[0] == 1.0             # exactly
    print(f"pw: worst relative error {worst:.3e}")
    assert worst <= 1e-9
    # exact powers of two at integer exponents
    assert pw(np.array([0.5, 0.25, 2.0 ** -64]), 2.0).tolist() == [0.25, 0.0625, 2.0 ** -128]


# ---------------------------------------------------------------------------
# the definition on written-out answers
# ---------------------------------------------------------------------------
def test_a_plane_tilted_east_at_exponent_1():
    words, slope, stats = direction_ref(plane((6, 7), 1.0, 0.0), (1.0, 1.0, 1.0))
    flow, main, shares = mfd.unpack(words)
    # E is the main receiver; NE and SE get 256 * 0.7071 / 2.4142 = 74.98 -> 75 each
    assert flow[:, :-1].all() and (main[:, :-1] == 0).all()
    assert (shares[1:-1, :-1, 0] == 75).all() and (shares[1:-1, :-1, 6] == 75).all()
    assert not shares[1:-1, :-1, 1:6].any()
    by_direction = mfd.shares_of(words)
    assert (by_direction[1:-1, :-1] == [106, 75, 0, 0, 0, 0, 0, 75]).all()
    # the top row has no NE neighbour: 256 * 0.7071 / 1.7071 = 106.04 -> 106 to SE
    assert (by_direction[0, :-1] == [150, 0, 0, 0, 0, 0, 0, 106]).all()
    assert (by_direction[-1, :-1] == [150, 106, 0, 0, 0, 0, 0, 0]).all()
    # the east column has nowhere to go
    assert not words[:, -1].any() and not slope[:, -1].any() and (slope[:, :-1] == 1).all()
    assert stats == {"no_flow": 6, "fallback_cells": 0, "split_cells": 36}


def test_two_equal_receivers_get_exactly_half_each():
    words, slope, _ = direction_ref(np.array([[0, 1, 0]], F32), (1.0, 1.0, 1.0))
    assert words[0, 0] == 0 and words[0, 2] == 0
    assert mfd.shares_of(words)[0, 1].tolist() == [128, 0, 0, 0, 128, 0, 0, 0]
    flow, main, shares = mfd.unpack(words)
    assert flow[0, 1] and main[0, 1] == 0 and shares[0, 1].tolist() == [0, 0, 0, 128, 0, 0, 0]
    assert slope.tolist() == [[0, 1, 0]]
    for e in (0.25, 1.1, 16.0):                             # pw(1, e) is 1 exactly
        again, _, _ = direction_ref(np.array([[0, 1, 0]], F32), "holmgren", e)
        assert np.array_equal(again, words)
    acc = accumulate_ref(words, frac_bits=0)
    assert acc.tolist() == [[1, 1, 2]]                      # (1 * 128) >> 8 = 0: the main one
    acc = accumulate_ref(words, frac_bits=16)               # takes what is left, here all
    assert acc.tolist() == [[(1 << 16) + (1 << 15), 1 << 16, (1 << 16) + (1 << 15)]]


def test_a_five_by_five_cone():
    rows, cols = np.mgrid[0:5, 0:5]
    z = (-np.hypot(rows - 2, cols - 2)).astype(F32)
    words, slope, stats = direction_ref(z, (1.0, 1.0, 1.0))
    by_direction = mfd.shares_of(words)
    # the summit: eight receivers at the same slope to a float32 rounding, 32 each
    assert by_direction[2, 2].tolist() == [32] * 8 and mfd.unpack(words)[1][2, 2] == 0
    assert slope[2, 2] == F32(float(F32(math.sqrt(2))) / math.sqrt(2))
    # the cone turns with the raster: a quarter turn moves every direction by two
    turned = mfd.shares_of(direction_ref(np.rot90(z).copy(), (1.0, 1.0, 1.0))[0])
    assert np.array_equal(turned, np.roll(np.rot90(by_direction, axes=(0, 1)), 2, axis=-1))
    # the corners are the lowest cells, and only they end a path
    assert (words == 0).sum() == 4 and stats["no_flow"] == 4
    for frac_bits in (0, 16):
        acc = accumulate_ref(words, frac_bits=frac_bits)
        assert np.array_equal(acc, accumulate_walk(words, frac_bits))
        assert int(acc[words == 0].sum()) == 25 << frac_bits
    assert accumulate_ref(words)[2, 2] == 1 << 16
    assert accumulate_ref(words)[2, 3] == (1 << 16) + ((1 << 16) * 32 >> 8)
    # a higher exponent concentrates: east of the summit, E takes more than at exponent 1
    sharp = mfd.shares_of(direction_ref(z, "holmgren", 8.0)[0])
    assert sharp[2, 3, 0] > by_direction[2, 3, 0] and sharp[2, 3].sum() == 256


def test_cells_that_are_not_square():
    dx, dy = 30.0, 20.0
    high = 101.0
    # E 30 lower over 30, N 20 lower over 20: two slopes of 1, half each
    z = np.array([[high, 80, high], [high, 100, 70], [high, high, high]], F32)
    words, slope, _ = direction_ref(z, (1.0, 1.0, 1.0), dx=dx, dy=dy)
    assert mfd.shares_of(words)[1, 1].tolist() == [128, 0, 128, 0, 0, 0, 0, 0] and slope[1, 1] == 1
    # the same elevations on square cells: E is 1.5 times as steep as N, 256 * 20 / 50 = 102.4
    square, slope, _ = direction_ref(z, (1.0, 1.0, 1.0))
    assert mfd.shares_of(square)[1, 1].tolist() == [154, 0, 102, 0, 0, 0, 0, 0] and slope[1, 1] == 30
    # a diagonal neighbour is sqrt(dx^2 + dy^2) away: NE 26 lower is 26 / sqrt(1300) = 0.7211
    z[0, 2] = 74
    words, _, _ = direction_ref(z, (1.0, 1.0, 1.0), dx=dx, dy=dy)
    f_ne = 26 / math.sqrt(1300)
    p_ne, p_n = math.floor(256 * f_ne / (2 + f_ne) + 0.5), math.floor(256 / (2 + f_ne) + 0.5)
    assert (p_ne, p_n) == (68, 94)
    assert mfd.shares_of(words)[1, 1].tolist() == [256 - p_ne - p_n, p_ne, p_n, 0, 0, 0, 0, 0]
    # the quinn preset weighs the cardinal directions 0.5 and the diagonal ones 0.354
    z = np.array([[5, 5, 4], [5, 5, 4], [5, 5, 5]], F32)
    words, _, _ = direction_ref(z, "quinn")
    f_e, f_ne = 0.5 * 1.0, 0.35355339059327373 * (1 / math.sqrt(2))
    assert mfd.shares_of(words)[1, 1].tolist() == \
        [256 - math.floor(256 * f_ne / (f_e + f_ne) + 0.5),
         math.floor(256 * f_ne / (f_e + f_ne) + 0.5), 0, 0, 0, 0, 0, 0]


def test_nodata_the_raster_edge_flats_and_the_fallback():
    z = plane((6, 6), 1.0, 0.0)
    z[2, 3] = np.nan
    z[4, 4] = -np.inf
    words, slope, _ = direction_ref(z, (1.0, 1.0, 1.0))
    assert words[2, 3] == 0 and np.isnan(slope[2, 3])
    # west of the NaN: NE and SE alone, half each, the first of them main
    assert mfd.shares_of(words)[2, 2].tolist() == [0, 128, 0, 0, 0, 0, 0, 128]
    assert mfd.unpack(words)[1][2, 2] == 1 and slope[2, 2] == F32(1 / math.sqrt(2))
    # an infinitely low neighbour takes everything; an infinite cell itself has no outflow
    assert mfd.shares_of(words)[4, 3].tolist() == [256, 0, 0, 0, 0, 0, 0, 0]
    assert np.isinf(slope[4, 3]) and words[4, 4] == 0 and slope[4, 4] == 0
    flat = np.full((4, 5), 7, F32)
    codes = np.zeros((4, 5), np.uint8)
    codes[1, 1:4], codes[2, 1:4] = (1, 128, 64), (2, 4, 8)
    words, slope, stats = direction_ref(flat, fallback=codes)
    assert stats == {"no_flow": 14, "fallback_cells": 6, "split_cells": 0} and not slope.any()
    assert np.array_equal(words, mfd.words_from_d8(codes))
    assert mfd.unpack(words)[1][1:3, 1:4].tolist() == [[0, 1, 2], [7, 6, 5]]
    assert not mfd.unpack(words)[2].any()
    assert not direction_ref(flat)[0].any() and direction_ref(flat)[2]["no_flow"] == 20
    # a cell with a way down keeps it; an invalid byte counts only where it is used
    junk = np.full((5, 5), 3, np.uint8)
    words, _, stats = direction_ref(plane((5, 5), 1.0, 0.0), fallback=np.full((5, 5), 4, np.uint8))
    assert stats["fallback_cells"] == 5 and (mfd.unpack(words)[1][:, :-1] == 0).all()
    with pytest.raises(ValueError, match="invalid D8 code in 5 cells"):
        direction_ref(plane((5, 5), 1.0, 0.0), fallback=junk)


# ---------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (3, 3), (17, 23), (40, 31)])
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_every_unit_arrives_at_a_terminal(shape, frac_bits):
    z = random_dem(shape, seed=shape[0] * 100 + shape[1], nan=0.02)
    words, _, stats = direction_ref(z)
    assert not mfd.invalid(words).any()
    acc = accumulate_ref(words, frac_bits=frac_bits)
    assert int(acc[words == 0].sum()) == z.size << frac_bits
    assert acc.min() >= 1 << frac_bits
    if z.size <= 400:
        assert np.array_equal(acc, accumulate_walk(words, frac_bits))
    assert counts_of(words)["split_cells"] == stats["split_cells"]
    assert shape[0] < 17 or stats["split_cells"] > 0.5 * z.size
    # and on words that no direction made: 1 ... 8 receivers with random shares
    words = random_acyclic_words(shape, seed=shape[1])
    acc = accumulate_ref(words, frac_bits=frac_bits)
    assert int(acc[words == 0].sum()) == z.size << frac_bits
    if z.size <= 400:
        assert np.array_equal(acc, accumulate_walk(words, frac_bits))


def test_weighted_accumulation_conserves_the_quantised_weights():
    rng = np.random.default_rng(5)
    words = random_acyclic_words((23, 31), seed=8)
    for weights, frac_bits in ((rng.random((23, 31)).astype(F32) * 9, 20),
                               (rng.integers(0, 2 ** 14, (23, 31)).astype(np.uint32), 16),
                               (rng.integers(0, 256, (23, 31)).astype(np.uint8), 3)):
        acc = accumulate_ref(words, weights, frac_bits)
        assert int(acc[words == 0].sum()) == int(dinf.quantise(weights, frac_bits).sum())
    ones = np.ones((23, 31), np.uint8)
    assert np.array_equal(accumulate_ref(words, ones, 16), accumulate_ref(words, None, 16))
    nan = np.full((23, 31), np.nan, F32)
    assert not accumulate_ref(words, nan, 16).any()
    for bad in (-1.0, np.inf, 2.0 ** 16):
        weights = np.ones((23, 31), F32)
        weights[3, 3] = bad
        with pytest.raises(ValueError, match="weights out of range in 1 cells"):
            accumulate_ref(words, weights, 16)


@pytest.mark.parametrize("shape,ramp", [((1, 1), False), ((9, 14), False), ((40, 70), True)])
def test_canonical_words_reproduce_d8(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=3, ramp=ramp)
    # the D8 reference lets a code point outside; a word may not
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    words = mfd.words_from_d8(codes)
    for frac_bits in (0, 5, 16):
        assert np.array_equal(accumulate_ref(words, frac_bits=frac_bits),
                              acc_kahn(codes) << frac_bits)
    assert np.array_equal(words != 0, codes != 0) and counts_of(words)["split_cells"] == 0
    # the main directions are those of the canonical D-infinity words
    facet, q = dinf.unpack(dinf.words_from_d8(codes))
    eighths = np.where(q == 0, 2 * ((facet >> 1) & 3), 2 * ((facet.astype(int) - 1) >> 1) + 1)
    assert np.array_equal(mfd.unpack(words)[1][codes != 0], eighths[codes != 0])


def test_multiplying_the_dem_by_four_changes_no_word():
    z = random_dem((40, 31), seed=6, nan=0.02)
    for method, exponent in (("freeman", None), ("quinn", None), ("holmgren", 4.0)):
        words, slope, _ = direction_ref(z, method, exponent)
        again, steeper, _ = direction_ref(z * F32(4), method, exponent)
        assert np.array_equal(words, again)
        assert np.array_equal(steeper, slope * F32(4), equal_nan=True)


def test_a_high_exponent_concentrates_the_flow():
    """The issue proposed "exponent 16 leaves >= 90 % of the split cells of ``random_dem`` with a
    main share >= 200 / 256" and asked for the property the reference does meet if it does not
    meet that one.  It does not: ``random_dem`` is white noise on a gentle ramp, many cells have
    two lower neighbours at nearly the same slope, and the reference leaves 71.7 % of the 615
    split cells (84.0 % of the 1090 cells with outflow) at 200 / 256 or more.  What it meets, and
    what is asserted: >= 90 % of the split cells keep at least half (128 / 256) with their main
    receiver (97.7 % here, against 28.6 % at exponent 1), and no cell's main share falls when
    the exponent rises from 1 to 16 by more than the quantisation allows -- the exact share
    1 / F of the steepest receiver grows with the exponent, and seven roundings of at most 1 / 2
    on either side can hide 7 units of it."""
    z = random_dem((40, 31), seed=6)
    words, _, _ = direction_ref(z, "holmgren", 16.0)
    split = (words & np.uint64((1 << 56) - 1)) != 0
    by_direction = mfd.shares_of(words)
    main_share = np.take_along_axis(by_direction, mfd.unpack(words)[1][..., None].astype(int),
                                    axis=-1)[..., 0]
    print(f"exponent 16: {int(split.sum())} split cells, "
          f"{float((main_share[split] >= 200).mean()):.3f} with main >= 200 / 256, "
          f"{float((main_share[split] >= 128).mean()):.3f} with main >= 128 / 256")
    assert split.sum() > 100 and float((main_share[split] >= 128).mean()) >= 0.9
    # and every cell with outflow sums to one
    assert (by_direction.sum(axis=-1)[words != 0] == 256).all()
    linear = mfd.shares_of(direction_ref(z, "holmgren", 1.0)[0])
    assert (main_share - linear.max(axis=-1)).min() >= -7
    assert float((linear.max(axis=-1)[split] >= 128).mean()) < 0.5
    mild = mfd.shares_of(direction_ref(z, "holmgren", 0.25)[0])
    assert mild.max(axis=-1)[split].mean() < main_share[split].mean()


def test_pack_and_unpack_round_trip():
    rng = np.random.default_rng(1)
    flow = rng.random((30, 40)) < 0.8
    main = np.where(flow, rng.integers(0, 8, (30, 40)), 0)
    shares = np.where(flow[..., None], rng.integers(0, 37, (30, 40, 7)), 0)
    words = mfd.pack(flow, main, shares)
    assert words.dtype == np.uint64 and not (words >> np.uint64(60)).any()
    got_flow, got_main, got_shares = mfd.unpack(words)
    assert np.array_equal(got_flow, flow) and np.array_equal(got_main, main)
    assert np.array_equal(got_shares, shares) and not mfd.invalid(words).any()
    assert mfd.shares_of(words).sum(axis=-1)[flow].tolist() == [256] * int(flow.sum())
    assert mfd.pack(True, 7, [255, 0, 0, 0, 0, 0, 0]) == HAS_FLOW | (7 << 56) | 255
    assert mfd.shares_of(mfd.pack(True, 7, [255, 0, 0, 0, 0, 0, 0])).tolist() == \
        [255, 0, 0, 0, 0, 0, 0, 1]
    for bad in ((True, 8, [0] * 7), (True, -1, [0] * 7), (True, 0, [256] + [0] * 6),
                (True, 0, [128, 128] + [0] * 5), (False, 1, [0] * 7), (False, 0, [1] + [0] * 6),
                (True, 0, [0] * 6)):
        with pytest.raises(ValueError):
            mfd.pack(*bad)
    with pytest.raises(ValueError, match="uint64"):
        mfd.unpack(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        mfd.words_from_d8(np.array([[3, 1, 255]], np.uint8))
    # each clause of "valid"
    assert mfd.invalid(np.array([0, HAS_FLOW, 1, 1 << 56, HAS_FLOW | (1 << 60), 1 << 63,
                                 HAS_FLOW | 0x8080, HAS_FLOW | 0x807F], np.uint64)).tolist() == \
        [False, False, True, True, True, True, True, False]


def test_presets_and_methods():
    assert mfd.PRESETS == {"freeman": (1.1, 1.0, 1.0),
                           "quinn": (1.0, 0.5, 0.35355339059327373),
                           "holmgren": (None, 1.0, 1.0)}
    assert mfd.method_of() == (1.1, 1.0, 1.0)
    assert mfd.method_of("quinn") == (1.0, 0.5, 0.5 / math.sqrt(2)) or \
        abs(mfd.method_of("quinn")[2] - 0.5 / math.sqrt(2)) < 1e-16
    assert mfd.method_of("holmgren", 4) == (4.0, 1.0, 1.0)
    assert mfd.method_of((2, 1, 0.5)) == (2.0, 1.0, 0.5)


def test_the_reference_refuses_what_the_operator_refuses():
    ok = mfd.pack([[False, True, False]], [[0, 0, 0]], np.zeros((1, 3, 7), int))
    assert accumulate_ref(ok).tolist() == [[1 << 16, 1 << 16, 2 << 16]]
    for word in (1, 1 << 56, HAS_FLOW | (1 << 60), 1 << 63, HAS_FLOW | 0x8080):
        bad = ok.copy()
        bad[0, 0] = word
        with pytest.raises(ValueError, match="invalid MFD word in 1 cells"):
            accumulate_ref(bad)
    with pytest.raises(ValueError, match="outside the raster in 1 cells"):
        accumulate_ref(mfd.pack([[False, False, True]], [[0, 0, 0]], np.zeros((1, 3, 7), int)))
    shares = np.zeros((1, 3, 7), int)
    shares[0, 0, 0] = 9                                     # E main, NE with a share: outside
    with pytest.raises(ValueError, match="outside the raster in 1 cells"):
        accumulate_ref(mfd.pack([[True, False, False]], [[0, 0, 0]], shares))
    loop = mfd.pack([[True, True, False]], [[0, 4, 0]], np.zeros((1, 3, 7), int))
    with pytest.raises(ValueError, match="2 cells never resolve"):
        accumulate_ref(loop)


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    from hydrodem_amd.filters import custom_filters
    for name in ("MFDFlowDirection", "MFDFlowAccumulation", "DemToMFDArea"):
        assert getattr(hd, name) is getattr(custom_filters, name)
        assert issubclass(getattr(hd, name), hd.Filter)
        assert f"``{name}``" in custom_filters.__doc__
    f = hd.MFDFlowDirection()
    assert f.stats == {} and f.slope is None and f.method == "freeman" and f.exponent is None
    assert f.keep_partial_results is False and f.fallback is None and f.cellsize == 1.0
    a = hd.MFDFlowAccumulation()
    assert a.frac_bits == 16 and a.output == "value" and a.dtype == np.float32
    assert a.weights is None and hd.MFDFlowAccumulation(output="sum").dtype == np.int64
    chain = hd.DemToMFDArea()
    assert chain.flats == "keep" and chain.words is None and chain.stats == {}
    assert [type(m).__name__ for m in chain.filters] == [
        "SinkFill", "D8FlowDirection", "MFDFlowDirection", "MFDFlowAccumulation"]
    assert chain.filters[0].epsilon == 1e-3
    # the calls live in hydrodem_amd.mfd: the binding module lists no device twin of theirs
    assert not [n for n in dir(backend) if "mfd" in n.lower() and n.endswith("_dev")]
    assert not [n for n in backend.SIGNATURES if "mfd" in n and n.endswith("_dev")]


def test_every_refusal_comes_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    z = np.zeros((4, 5), F32)
    words = np.zeros((4, 5), np.uint64)

    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    # the direction
    assert said(lambda: hd.MFDFlowDirection().apply(z.astype(np.float64))) == \
        "MFD flow direction takes a float32 DEM, got float64"
    assert said(lambda: hd.MFDFlowDirection().apply(np.zeros((2, 4, 5), F32))) == \
        "MFD flow direction takes a 2-D raster, got 3 dimensions"
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.MFDFlowDirection().apply([[0.0]])
    assert said(lambda: hd.MFDFlowDirection(method="tarboton")) == \
        "method is one of ['freeman', 'quinn', 'holmgren'] or an (exponent, w_card, w_diag) " \
        "triple, got 'tarboton'"
    assert said(lambda: hd.MFDFlowDirection(method="holmgren")) == \
        "method 'holmgren' needs an exponent"
    assert said(lambda: hd.MFDFlowDirection(method="quinn", exponent=2)) == \
        "method 'quinn' has the exponent 1.0: leave exponent out, or choose 'holmgren'"
    for bad in (0.2, 16.5, float("nan"), float("inf")):
        assert said(lambda: hd.MFDFlowDirection("holmgren", bad)) == \
            f"the exponent is 0.25 ... 16, got {float(bad)}"
    assert said(lambda: hd.MFDFlowDirection("holmgren", "steep")) == \
        "the exponent is a number, got 'steep'"
    assert said(lambda: hd.MFDFlowDirection((1.0, 0.0, 1.0))) == \
        "w_card must be finite and positive, got 0.0"
    assert said(lambda: hd.MFDFlowDirection((1.0, 1.0, float("inf")))) == \
        "w_diag must be finite and positive, got inf"
    assert said(lambda: hd.MFDFlowDirection((1.0, 1.0))) == \
        "method is one of ['freeman', 'quinn', 'holmgren'] or an (exponent, w_card, w_diag) " \
        "triple, got (1.0, 1.0)"
    assert said(lambda: hd.MFDFlowDirection(cellsize=0)) == \
        "cellsize must be finite and positive, got 0.0"
    assert said(lambda: hd.MFDFlowDirection(cellsize=(1, 2, 3))) == \
        "cellsize is a number or a (dx, dy) pair, got (1, 2, 3)"
    assert said(lambda: hd.MFDFlowDirection(fallback=np.zeros((4, 5), np.uint32))) == \
        "fallback has dtype uint8, got uint32"
    assert said(lambda: hd.MFDFlowDirection(fallback=np.zeros((3, 5), np.uint8)).apply(z)) == \
        "the fallback is (3, 5), the dem (4, 5)"
    assert said(lambda: mfd.mfd(z, want=("angle",))) == \
        "unknown MFD outputs ['angle']: choose among ['slope']"
    assert said(lambda: mfd.mfd(None)) == "MFD flow direction needs the dem it is derived from"
    # the accumulation
    assert said(lambda: hd.MFDFlowAccumulation().apply(words.astype(np.uint32))) == \
        "MFD flow accumulation takes uint64 MFD words, got uint32"
    assert said(lambda: hd.MFDFlowAccumulation().apply(np.zeros((2, 4, 5), np.uint64))) == \
        "MFD flow accumulation takes a 2-D raster, got 3 dimensions"
    for bad in (-1, 17, 1.5, True, None):
        assert said(lambda: hd.MFDFlowAccumulation(frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 16, got {bad!r}"
        assert said(lambda: hd.DemToMFDArea(frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 16, got {bad!r}"
    assert said(lambda: hd.MFDFlowAccumulation(frac_bits=31, weights=z)) == \
        "frac_bits is an integer in 0 ... 30 for float32 weights, got 31"
    assert said(lambda: hd.MFDFlowAccumulation(frac_bits=17, weights=z.astype(np.uint8))) == \
        "frac_bits is an integer in 0 ... 16 for uint8 weights, got 17"
    assert said(lambda: hd.MFDFlowAccumulation(weights=z.astype(np.float64))) == \
        "weights has dtype uint8 or uint32 or float32, got float64"
    assert said(lambda: hd.MFDFlowAccumulation(weights=np.zeros((3, 5), F32)).apply(words)) == \
        "the weights are (3, 5), the words (4, 5)"
    assert said(lambda: mfd.mfdacc(words, np.zeros((4, 5), np.int32))) == \
        "the weights are float32, uint32 or uint8, got int32"
    assert said(lambda: hd.MFDFlowAccumulation(output="mask")) == \
        "output is one of ['sum', 'value'], got 'mask'"
    assert said(lambda: mfd.mfdacc(words, want=())) == \
        "no output wanted: choose among ['sum', 'value']"
    assert said(lambda: mfd.mfdacc(words, want=("area",))) == \
        "unknown MFD accumulation outputs ['area']: choose among ['sum', 'value']"
    assert said(lambda: mfd.mfdacc([[0]])) == "words is a NumPy array, got <class 'list'>"
    assert said(lambda: mfd.mfdacc_args(None)) == \
        "MFD flow accumulation needs the words it routes along"
    # the chain
    assert said(lambda: hd.DemToMFDArea(flats="fill")) == \
        "flats is 'keep' or 'resolve', got 'fill'"
    assert said(lambda: hd.DemToMFDArea(output="mask")) == \
        "output is one of ['sum', 'value'], got 'mask'"
    assert said(lambda: hd.DemToMFDArea(method="holmgren")) == \
        "method 'holmgren' needs an exponent"
    assert said(lambda: hd.DemToMFDArea(cellsize=-1)) == \
        "cellsize must be finite and positive, got -1.0"
    assert said(lambda: hd.DemToMFDArea().apply(z.astype(np.float64))) == \
        "DemToMFDArea takes a float32 DEM, got float64"
    assert said(lambda: hd.DemToMFDArea().apply(np.zeros((2, 4, 5), F32))) == \
        "DemToMFDArea takes a 2-D raster, got 3 dimensions"


def test_the_header_declares_both_blocks_and_the_binding_mirrors_them(built):
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "A24  MFDFlowDirection.apply" in header and "A25  MFDFlowAccumulation.apply" in header
    for name, count in (("hdem_mfd_f32", 14), ("hdem_mfdacc_u64", 11)):
        declared = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(declared.split(",")) == count
        assert len(backend.SIGNATURES[name]) == count
        assert name + "_dev" not in backend.SIGNATURES and f"{name}_dev(" not in header
    flag = re.search(r"#define\s+HDEM_ON_DEVICE\s+(0x[0-9a-fA-F]+)", header)
    assert int(flag.group(1), 16) == mfd.ON_DEVICE
    assert ctypes.sizeof(backend._MFDStats) == 32           # pylint: disable=protected-access
    assert ctypes.sizeof(backend._MFDAccStats) == 104       # pylint: disable=protected-access
    assert "} hdem_mfd_stats;            /* sizeof == 32 */" in header
    assert "typedef hdem_dinfsum_stats hdem_mfdacc_stats;" in header
    # the power function is written out in the header's text, and the 8-bit resolution is stated
    for line in ("(m, k) = frexp(t)", "if m < 0.7071067811865476:  m = m * 2.0, k = k - 1",
                 "l2 = (double)k + ((2.0 * s) * r) * 1.4426950408889634",
                 "pw = ldexp(p, (int)n)", "a share below 1 / 512 is lost to the main"):
        assert line in header, line
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "hdem_mfd.hip" in makefile
    # a null context is BAD_ARG, whatever else is passed, with and without the device flag
    lib = backend.load_library()
    for name in ("hdem_mfd_f32", "hdem_mfdacc_u64"):
        args = [t() for t in backend.SIGNATURES[name]]
        assert getattr(lib, name)(*args) == backend.BAD_ARG
        assert lib.hdem_last_error() == b"ctx is null"
        args[-2] = ctypes.c_int(mfd.ON_DEVICE)
        assert getattr(lib, name)(*args) == backend.BAD_ARG
        assert lib.hdem_last_error() == b"ctx is null"
