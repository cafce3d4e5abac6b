"""
Weighted D-infinity accumulation and the terrain attributes of a float32 area
(``WeightedDInfFlowAccumulation``, ``AreaWetnessIndex``, ``DemToDInfWetness``,
``hdem_dinfsum_u32``, ``hdem_terrain_area_f32``): the CPU half.

The host references live here and are used by the GPU tests.  They transcribe blocks A22 and A23
of include/hydrodem_hip.h:
  ``quantise_ref``             q(w) one weight at a time in exact rational arithmetic;
  ``accumulate_weighted_ref``  Kahn's order on ``receivers`` of tests/test_dinf.py, int64;
  ``accumulate_weighted_walk`` the same pull by plain recursion -- tiny grids;
  ``area_reference``           the float32 formulas of A23 from the functions of
                               tests/test_terrain_attributes.py: a float32 area goes through
                               ``area_f32`` as it is (``astype(float32)`` of a float32 is itself).
No GPU here.
"""
import ctypes
import fractions
import math
import os
import re

import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend, dinf
from hydrodem_amd import terrain as T
from hydrodem_amd.dinf import FACETS, Q_ONE
from test_device_ownership import StandIn
from test_dinf import accumulate_ref, direction_ref, random_dem, receivers
from test_flowacc import random_acyclic_codes, terminal_mask
from test_flowsum import wsum_kahn
from test_terrain_attributes import (floored, gradient_f32, spi_f32, twi_f64)
from test_terrain_calls import Recorder, call_operands, device_form, stand_in_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
Q_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def quantise_ref(weights, frac_bits):
    """(q int64, NaN weights, bad weights) of block A22, one weight at a time: the product with
    2^frac_bits exactly, one rounding to nearest even; a refused weight counts 0."""
    weights = np.asarray(weights)
    q = np.zeros(weights.shape, np.int64)
    nan = bad = 0
    for at, w in np.ndenumerate(weights):
        if weights.dtype.kind == "f":
            if np.isnan(w):
                nan += 1
                continue
            if np.isinf(w) or w < 0:
                bad += 1
                continue
            value = round(fractions.Fraction(float(w)) * 2 ** frac_bits)     # ties to even
        else:
            value = int(w) << frac_bits
        if value > Q_MAX:
            bad += 1
            continue
        q[at] = value
    return q, nan, bad


def accumulate_weighted_ref(words, q):
    """int64 ``A`` of block A22 in Kahn's order; ValueError "N cells never resolve" on a cycle."""
    words = np.asarray(words, np.uint32)
    card, diag, share = receivers(words)
    n = words.size
    indeg = np.bincount(card[card >= 0], minlength=n) + np.bincount(diag[diag >= 0], minlength=n)
    acc = np.asarray(q, np.int64).ravel().copy()
    assert acc.size == n
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        to_diag = (acc[frontier] * share[frontier]) >> 15
        to_card = acc[frontier] - to_diag
        woken = []
        for rec, part in ((diag[frontier], to_diag), (card[frontier], to_card)):
            has = rec >= 0
            np.add.at(acc, rec[has], part[has])
            np.subtract.at(indeg, rec[has], 1)
            woken.append(rec[has])
        woken = np.unique(np.concatenate(woken))
        frontier = woken[indeg[woken] == 0]
    if done != n:
        raise ValueError(f"D-infinity words form a cycle: {n - done} cells never resolve")
    return acc.reshape(words.shape)


def accumulate_weighted_walk(words, q):
    """The same pull, cell by cell with memoised recursion (tiny acyclic grids)."""
    words = np.asarray(words, np.uint32)
    h, w = words.shape
    memo = {}

    def area(y, x):
        if (y, x) not in memo:
            total = int(q[y, x])
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if (dy or dx) and 0 <= ny < h and 0 <= nx < w and words[ny, nx] >> 16:
                        facet, share = int(words[ny, nx] >> 16), int(words[ny, nx] & 0xFFFF)
                        e1, e2, _, _ = FACETS[facet]
                        if e2 == (-dy, -dx) and share:
                            total += (area(ny, nx) * share) >> 15
                        if e1 == (-dy, -dx) and share != Q_ONE:
                            total += area(ny, nx) - ((area(ny, nx) * share) >> 15)
            memo[y, x] = total
        return memo[y, x]

    return np.array([[area(y, x) for x in range(w)] for y in range(h)], np.int64)


def random_weights(shape, seed, dtype, nan=0.0):
    """Weights of ``dtype`` whose quantised values stay in range at every frac_bits a test uses:
    float32 below 1.9 (q < 2^31 at frac_bits 30), integers below 2^15 (q < 2^31 at 16)."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        w = (rng.random(shape) * 1.9).astype(F32)
        w[rng.random(shape) < 0.1] = 0.0
        if nan:
            w[rng.random(shape) < nan] = np.nan
        return w
    high = 256 if np.dtype(dtype) == np.uint8 else 2 ** 15
    return rng.integers(0, high, shape).astype(dtype)


def area_reference(dem, area, dx, dy, z_factor, min_slope, given=None):
    """``twi`` (float64, of the reference's own float32 operands), ``spi`` (float32) and the
    stats of block A23; ``t`` is ``given`` as it is (NaN where the dem is), else Horn's tangent."""
    dzdx, dzdy, _, tangent = gradient_f32(dem, dx, dy, z_factor)
    t = tangent if given is None else np.where(np.isnan(dem), F32(np.nan), given).astype(F32)
    with np.errstate(invalid="ignore"):
        nonpositive = int((area <= 0).sum())
    return {"twi": twi_f64(area, t, dx, dy, min_slope), "spi": spi_f32(area, t, dx, dy),
            "stats": {"nan_cells": int(np.isnan(dem).sum()),
                      "flat_cells": int(((dzdx == 0) & (dzdy == 0)).sum()),
                      "floored_cells": int(floored(t, min_slope).sum()), "invalid_codes": 0,
                      "nonpositive_area": nonpositive}}


# ---------------------------------------------------------------------------
# the quantiser
# ---------------------------------------------------------------------------
def test_the_quantiser_on_written_out_values():
    w = np.array([0.5, 1.5, 2.5, -0.0, np.nan, 0.25, 0.75], F32)
    assert dinf.quantise(w, 0).tolist() == [0, 2, 2, 0, 0, 0, 1]          # ties to even
    assert dinf.quantise(w, 1).tolist() == [1, 3, 5, 0, 0, 0, 2]
    assert dinf.quantise(w, 2).tolist() == [2, 6, 10, 0, 0, 1, 3]
    assert quantise_ref(w, 0)[1:] == (1, 0)
    assert np.array_equal(quantise_ref(w, 0)[0], dinf.quantise(w, 0))
    # 2^31 - 1 is taken, 2^31 is not; float32 cannot hold 2^31 - 1, so at frac_bits 30
    just = np.array([np.nextafter(F32(2), F32(0)), 2.0], F32)
    q = dinf.quantise(just, 30)
    assert q.tolist() == [2 ** 31 - 128, 2 ** 31]
    assert quantise_ref(just, 30)[2] == 1 and quantise_ref(just, 30)[0].tolist() == [2 ** 31 - 128, 0]
    whole = np.array([Q_MAX, Q_MAX + 1], np.uint32)
    assert dinf.quantise(whole, 0).tolist() == [Q_MAX, Q_MAX + 1]
    assert quantise_ref(whole, 0)[2] == 1
    # integer weights are shifted: a deliberate difference from the D8 operator
    assert dinf.quantise(np.array([0, 1, 255], np.uint8), 16).tolist() == [0, 65536, 255 << 16]
    assert dinf.quantise(np.array([32767, 32768], np.uint32), 16).tolist() == \
        [32767 << 16, 1 << 31]
    assert quantise_ref(np.array([32767, 32768], np.uint32), 16)[2] == 1
    bad = np.array([-1.0, np.inf, -np.inf, -1e-30, 3e9], F32)
    assert quantise_ref(bad, 0)[1:] == (0, 5)


@pytest.mark.parametrize("dtype,frac_bits", [(np.float32, 0), (np.float32, 10), (np.float32, 30),
                                             (np.uint8, 0), (np.uint8, 16), (np.uint32, 16)])
def test_the_two_quantisers_agree(dtype, frac_bits):
    w = random_weights((13, 17), 5, dtype, nan=0.05)
    q, nan, bad = quantise_ref(w, frac_bits)
    assert np.array_equal(q, dinf.quantise(w, frac_bits)) and bad == 0
    assert nan == (int(np.isnan(w).sum()) if dtype == np.float32 else 0)
    assert 0 <= q.min() and q.max() <= Q_MAX


# ---------------------------------------------------------------------------
# the accumulation references against each other and against the unweighted ones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (3, 3), (17, 23), (40, 31)])
def test_the_references_agree_and_every_unit_arrives(shape):
    words, _, _, _ = direction_ref(random_dem(shape, seed=shape[0] * 100 + shape[1], nan=0.02))
    q = dinf.quantise(random_weights(shape, 3, F32, nan=0.05), 16)
    acc = accumulate_weighted_ref(words, q)
    assert acc.dtype == np.int64
    assert int(acc[words >> 16 == 0].sum()) == int(q.sum())          # conservation: total
    assert (acc >= q).all()
    if words.size <= 400:
        assert np.array_equal(acc, accumulate_weighted_walk(words, q))
    for frac_bits in (0, 16):
        unit = np.full(shape, 1 << frac_bits, np.int64)
        assert np.array_equal(accumulate_weighted_ref(words, unit), accumulate_ref(words, frac_bits))
        assert np.array_equal(dinf.quantise(np.ones(shape, np.uint8), frac_bits), unit)


@pytest.mark.parametrize("shape,ramp", [((1, 1), False), ((9, 14), False), ((40, 70), True)])
def test_canonical_words_reproduce_the_weighted_d8_sum(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=3, ramp=ramp)
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    q = np.random.default_rng(9).integers(0, 2 ** 31, shape, dtype=np.int64)
    assert np.array_equal(accumulate_weighted_ref(dinf.words_from_d8(codes), q),
                          wsum_kahn(codes, q))


def test_a_cycle_is_refused_by_the_reference():
    loop = dinf.pack(np.array([[1, 4, 0]]), np.array([[0, 0, 0]]))
    with pytest.raises(ValueError, match="2 cells never resolve"):
        accumulate_weighted_ref(loop, np.ones((1, 3), np.int64))


# ---------------------------------------------------------------------------
# the terrain reference of an area
# ---------------------------------------------------------------------------
def test_the_area_reference_floor_nan_and_given_slope():
    dem = np.array([[3, 2, 1], [3, 2, 1], [3, 2, 1]], F32)
    area = np.array([[1, 2.5, 0], [np.nan, 4, -1], [7, 8, 9]], F32)
    ref = area_reference(dem, area, 10.0, 30.0, 1.0, 1e-3)
    cell = F32(math.sqrt(300.0))
    # Horn: the plane drops 1 per 10 eastwards in the middle column, half that at the edges
    assert ref["spi"][1, 1] == F32(4) * cell * F32(0.1)
    assert ref["twi"][1, 1] == math.log(float(F32(4) * cell) / float(F32(0.1)))
    assert np.isnan(ref["twi"][1, 0]) and np.isnan(ref["spi"][1, 0])       # a NaN area
    assert ref["twi"][0, 2] == -np.inf and np.isnan(ref["twi"][1, 2])      # zero, negative
    assert ref["stats"]["nonpositive_area"] == 2 and ref["stats"]["floored_cells"] == 0
    given = np.array([[0.5, 0, -1], [1e-4, np.nan, 2], [1e-3, 1, 1]], F32)
    ref = area_reference(dem, area, 10.0, 30.0, 1.0, 1e-3, given)
    assert ref["stats"]["floored_cells"] == 3                              # 0, -1, 1e-4
    assert ref["twi"][0, 1] == math.log(float(F32(2.5) * cell) / float(F32(1e-3)))
    assert ref["twi"][2, 0] == math.log(float(F32(7) * cell) / float(F32(1e-3)))   # not below
    assert ref["spi"][0, 2] == F32(0) * F32(-1) and ref["spi"][1, 2] == F32(-1) * cell * F32(2)
    assert np.isnan(ref["twi"][1, 1]) and np.isnan(ref["spi"][1, 1])       # a NaN t stays NaN
    # an integer-valued area is the accumulation it came from
    acc = np.array([[1, 2, 3], [0, 5, 16777215], [7, 8, 9]], np.uint32)
    t = gradient_f32(dem, 10.0, 30.0)[3]
    assert np.array_equal(twi_f64(acc.astype(F32), t, 10.0, 30.0), twi_f64(acc, t, 10.0, 30.0))
    assert np.array_equal(spi_f32(acc.astype(F32), t, 10.0, 30.0), spi_f32(acc, t, 10.0, 30.0))


# ---------------------------------------------------------------------------
# refusals, before the device is touched
# ---------------------------------------------------------------------------
def test_every_refusal_comes_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    z = np.zeros((4, 5), F32)
    words = np.zeros((4, 5), np.uint32)
    ones = np.ones((4, 5), F32)

    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    # the weighted accumulation
    assert said(lambda: hd.WeightedDInfFlowAccumulation(None)) == \
        "WeightedDInfFlowAccumulation needs the weights it sums"
    assert said(lambda: hd.WeightedDInfFlowAccumulation(ones.astype(np.float64))) == \
        "weights has dtype uint8 or uint32 or float32, got float64"
    assert said(lambda: dinf.dinfsum(words, ones.astype(np.float64))) == \
        "the weights are float32, uint32 or uint8, got float64"
    assert said(lambda: dinf.dinfsum(words, None)) == \
        "weights is a NumPy array, got <class 'NoneType'>"
    assert said(lambda: hd.WeightedDInfFlowAccumulation([[1.0]])) == \
        "weights is a NumPy array or a DeviceRaster, got <class 'list'>"
    assert said(lambda: hd.WeightedDInfFlowAccumulation(ones).apply(words.astype(np.uint8))) == \
        "weighted D-infinity flow accumulation takes uint32 D-infinity words, got uint8"
    assert said(lambda: hd.WeightedDInfFlowAccumulation(ones).apply(np.zeros((2, 4, 5), np.uint32))) \
        == "weighted D-infinity flow accumulation takes a 2-D raster, got 3 dimensions"
    assert said(lambda: hd.WeightedDInfFlowAccumulation(np.ones((4, 6), F32)).apply(words)) == \
        "the weights are (4, 6), the words (4, 5)"
    for bad in (-1, 31, 1.5, True, None):
        assert said(lambda: hd.WeightedDInfFlowAccumulation(ones, frac_bits=bad)) == \
            f"frac_bits is an integer in 0 ... 30 for float32 weights, got {bad!r}"
    for dtype in (np.uint8, np.uint32):
        assert said(lambda: hd.WeightedDInfFlowAccumulation(ones.astype(dtype), frac_bits=17)) == \
            f"frac_bits is an integer in 0 ... 16 for {np.dtype(dtype)} weights, got 17"
        hd.WeightedDInfFlowAccumulation(ones.astype(dtype), frac_bits=16)
    assert said(lambda: hd.WeightedDInfFlowAccumulation(ones, output="mask")) == \
        "output is one of ['sum', 'value'], got 'mask'"
    assert said(lambda: dinf.dinfsum(words, ones, want=())) == \
        "no output wanted: choose among ['sum', 'value']"
    assert said(lambda: dinf.dinfsum(words, ones, want=("area",))) == \
        "unknown D-infinity accumulation outputs ['area']: choose among ['sum', 'value']"
    with pytest.raises(hd.NumpyArrayExpectedError):
        hd.WeightedDInfFlowAccumulation(ones).apply([[0]])
    # the terrain attributes of an area
    assert said(lambda: T.terrain_area(z.astype(np.float64), area=ones)) == \
        "terrain attributes take a float32 DEM, got float64"
    assert said(lambda: T.terrain_area(z)) == "twi needs the float32 area raster"
    assert said(lambda: T.terrain_area(z, "spi")) == "spi needs the float32 area raster"
    assert said(lambda: T.terrain_area(z, area=ones.astype(np.uint32))) == \
        "the area is float32, got uint32"
    assert said(lambda: T.terrain_area(z, area=np.ones((4, 6), F32))) == \
        "the area is (4, 6), the dem (4, 5)"
    assert said(lambda: T.terrain_area(z, area=ones, given_slope=ones.astype(np.float64),
                                       slope="given")) == "the given slope is float32, got float64"
    assert said(lambda: T.terrain_area(z, area=ones, slope="given")) == \
        "slope='given' needs the float32 given slope raster"
    assert said(lambda: T.terrain_area(z, area=ones, given_slope=ones)) == \
        "a given slope raster goes with slope='given', got 'horn'"
    assert said(lambda: T.terrain_area(z, area=ones, slope="dinf")) == \
        "slope is 'horn', 'given' or 'd8', got 'dinf'"
    assert said(lambda: T.terrain_area(z, area=ones, slope="d8")) == \
        "slope='d8' needs the uint8 D8 codes"
    assert said(lambda: T.terrain_area(z, "aspect", min_slope=0)) == \
        "min_slope must be finite and positive, got 0.0"
    assert said(lambda: hd.AreaWetnessIndex(ones.astype(np.uint32))) == \
        "area has dtype float32, got uint32"
    assert said(lambda: hd.AreaWetnessIndex(None)) == "twi needs the float32 area raster"
    assert said(lambda: hd.AreaWetnessIndex(ones, given_slope=[[1.0]])) == \
        "given_slope is a NumPy array or a DeviceRaster, got <class 'list'>"
    assert said(lambda: hd.AreaWetnessIndex(ones, cellsize=0)) == \
        "cellsize must be finite and positive, got 0.0"
    assert said(lambda: hd.AreaWetnessIndex(np.ones((4, 6), F32)).apply(z)) == \
        "the area is (4, 6), the dem (4, 5)"
    assert said(lambda: hd.AreaWetnessIndex(ones, given_slope=np.ones((3, 5), F32)).apply(z)) == \
        "the given slope is (3, 5), the dem (4, 5)"
    # the chain
    assert said(lambda: hd.DemToDInfWetness(flats="fill")) == \
        "flats is 'keep' or 'resolve', got 'fill'"
    assert said(lambda: hd.DemToDInfWetness(slope="d8")) == "slope is 'dinf' or 'horn', got 'd8'"
    assert said(lambda: hd.DemToDInfWetness(frac_bits=17)) == \
        "frac_bits is an integer in 0 ... 16, got 17"
    assert said(lambda: hd.DemToDInfWetness(frac_bits=31, weights=ones)) == \
        "frac_bits is an integer in 0 ... 30 for float32 weights, got 31"
    assert said(lambda: hd.DemToDInfWetness(weights=ones.astype(np.float64))) == \
        "weights has dtype uint8 or uint32 or float32, got float64"
    assert said(lambda: hd.DemToDInfWetness(min_slope=-1)) == \
        "min_slope must be finite and positive, got -1.0"
    assert said(lambda: hd.DemToDInfWetness(cellsize=(1, 2, 3))) == \
        "cellsize is a number or a (dx, dy) pair, got (1, 2, 3)"
    assert said(lambda: hd.DemToDInfWetness().apply(z.astype(np.float64))) == \
        "DemToDInfWetness takes a float32 DEM, got float64"
    assert said(lambda: hd.DemToDInfWetness(weights=np.ones((4, 6), F32)).apply(z)) == \
        "the weights are (4, 6), the words (4, 5)"


# ---------------------------------------------------------------------------
# exports, the header and the binding
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package_and_the_drop_in():
    import subprocess
    import sys
    from hydrodem_amd.filters import custom_filters
    names = ("WeightedDInfFlowAccumulation", "AreaWetnessIndex", "DemToDInfWetness")
    for name in names:
        assert getattr(hd, name) is getattr(custom_filters, name)
        assert issubclass(getattr(hd, name), hd.Filter)
    ones = np.ones((2, 2), F32)
    f = hd.WeightedDInfFlowAccumulation(ones)
    assert f.frac_bits == 16 and f.output == "value" and f.dtype == np.float32
    assert f.auto_device is False and f.stats == {}
    assert hd.WeightedDInfFlowAccumulation(ones, output="sum").dtype == np.int64
    a = hd.AreaWetnessIndex(ones)
    assert a.slope == "horn" and a.want == ("twi",) and a.min_slope == 1e-3 and a.twi is None
    assert hd.AreaWetnessIndex(ones, ones).slope == "given"
    chain = hd.DemToDInfWetness()
    assert chain.flats == "keep" and chain.slope == "dinf" and chain.weights is None
    assert chain.filled is chain.codes is chain.words is chain.area is None and chain.stats == {}
    assert [type(m).__name__ for m in chain.filters] == [
        "SinkFill", "D8FlowDirection", "DInfFlowDirection"]
    assert chain.filters[0].epsilon == 1e-3
    assert T.AREA_SLOPES == ("horn", "given")
    assert not [n for n in backend.__all__ if "dinf" in n.lower() or "terrain" in n.lower()]
    # the reference's flat import resolves them
    code = ("import sys; sys.path.insert(0, sys.argv[1]); "
            "from filters.custom_filters import " + ", ".join(names))
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "hydrodem_amd", "dropin")],
                   check=True, cwd=ROOT, env={**os.environ, "PYTHONPATH": ROOT})


def test_the_header_declares_both_pairs_and_the_binding_mirrors_them(built):
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h"), encoding="utf-8").read()
    assert "A22  WeightedDInfFlowAccumulation.apply" in header
    assert "A23  AreaWetnessIndex.apply" in header
    for name, count in (("hdem_dinfsum_u32", 11), ("hdem_terrain_area_f32", 21)):
        host = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        dev = re.search(rf"int {name}_dev\((.*?)\);", header, re.S).group(1)
        assert " ".join(host.split()) == " ".join(dev.split())
        assert len(host.split(",")) == count
        assert len(backend.SIGNATURES[name]) == count
        assert backend.SIGNATURES[name] == backend.SIGNATURES[name + "_dev"]
    # pylint: disable=protected-access
    assert ctypes.sizeof(backend._DInfSumStats) == 104
    assert ctypes.sizeof(backend._TerrainAreaStats) == 48
    assert "hdem_dinfsum_stats;        /* sizeof == 104 */" in header
    assert "hdem_terrain_area_stats;    /* sizeof == 48 */" in header
    assert "#define HDEM_TERRAIN_TWI_GIVEN 2" in header and T.TWI_GIVEN == 2
    # the weighted stats open with the unweighted ones, the area's with the terrain's
    assert backend._DInfSumStats._fields_[:len(backend._DInfAccStats._fields_)] == \
        backend._DInfAccStats._fields_
    assert [n for n, _ in backend._DInfSumStats._fields_[-3:]] == \
        ["nan_weights", "bad_weights", "total"]
    assert backend._DInfSumStats.nan_weights.offset == ctypes.sizeof(backend._DInfAccStats)
    assert backend._TerrainAreaStats.nonpositive_area.offset == \
        ctypes.sizeof(backend._TerrainStats)
    lib = backend.load_library()
    for name in ("hdem_dinfsum_u32", "hdem_dinfsum_u32_dev", "hdem_terrain_area_f32",
                 "hdem_terrain_area_f32_dev"):
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"


# ---------------------------------------------------------------------------
# the C calls and ownership, on the stand-in library
# ---------------------------------------------------------------------------
RASTER, BYTES = 70 * 90 * 4, 70 * 90
FILL = ("hdem_sinkfill_d8_f32_dev", "ptr", 70, 90, 0.001, 0, 0, "ptr", "ptr", "stats")


def _recorded(call):
    lib = Recorder()
    _on_stand_in(lib, call)
    return lib.record()


def _on_stand_in(lib, run):
    ctx = stand_in_context(lib)
    real, backend.context = backend.context, lambda device=None: ctx
    try:
        return run(call_operands(), device_form(ctx))
    finally:
        backend.context = real


def _area_call(name, area, given, outputs, flags, cell=(1.0, 1.0)):
    wanted = tuple("ptr" if n in outputs else "null" for n in T.TERRAIN_OUTPUTS)
    return (name, "ptr", 70, 90, area, given, "null", cell[0], cell[1], 1.0, 0.001, *wanted, flags,
            "stats")


def test_the_c_calls_of_the_classes():
    weights = lambda o: o.dem                            # noqa: E731  (any float32 raster)
    assert _recorded(lambda o, dev: hd.WeightedDInfFlowAccumulation(weights(o), 10).apply(o.acc)) \
        == ([("hdem_dinfsum_u32", "ptr", 70, 90, "ptr", 1, 10, "null", "ptr", 0, "stats")], {})
    assert _recorded(lambda o, dev: hd.WeightedDInfFlowAccumulation(
        o.codes, 16, "sum").apply_device(dev(o.acc))) == (
            [("hdem_dinfsum_u32_dev", "ptr", 70, 90, "ptr", 3, 16, "ptr", "null", 0, "stats")],
            {"hdem_malloc": [BYTES, RASTER * 2], "hdem_memcpy_h2d": [BYTES]})
    assert _recorded(lambda o, dev: hd.AreaWetnessIndex(o.dem, cellsize=(30.0, 10.0))
                     .apply(o.dem)) == (
        [_area_call("hdem_terrain_area_f32", "ptr", "null", ("twi",), 0, (10.0, 30.0))], {})
    assert _recorded(lambda o, dev: hd.AreaWetnessIndex(
        dev(o.dem), o.dem, want=("spi", "twi"), keep_partial_results=True)
        .apply_device(dev(o.dem))) == (
            [_area_call("hdem_terrain_area_f32_dev", "ptr", "ptr", ("twi", "spi"), 2)],
            {"hdem_malloc": [RASTER] * 3, "hdem_memcpy_h2d": [RASTER]})
    dinf_call = ("hdem_dinf_f32_dev", "ptr", 70, 90, "ptr", 30.0, 10.0, "ptr", "null", "ptr", 0,
                 "stats")
    assert _recorded(lambda o, dev: hd.DemToDInfWetness(cellsize=(30.0, 10.0))
                     .apply_device(dev(o.dem))) == (
        [FILL, dinf_call,
         ("hdem_dinfacc_u32_dev", "ptr", 70, 90, 16, "null", "ptr", 0, "stats"),
         _area_call("hdem_terrain_area_f32_dev", "ptr", "ptr", ("twi",), 2, (30.0, 10.0))],
        {"hdem_malloc": [BYTES] + [RASTER] * 5})
    assert _recorded(lambda o, dev: hd.DemToDInfWetness(slope="horn", weights=o.codes, frac_bits=8)
                     .apply_device(dev(o.dem))) == (
        [FILL, ("hdem_dinf_f32_dev", "ptr", 70, 90, "ptr", 1.0, 1.0, "ptr", "null", "null", 0,
                "stats"),
         ("hdem_dinfsum_u32_dev", "ptr", 70, 90, "ptr", 3, 8, "null", "ptr", 0, "stats"),
         _area_call("hdem_terrain_area_f32_dev", "ptr", "null", ("twi",), 0)],
        {"hdem_malloc": [BYTES, BYTES] + [RASTER] * 4, "hdem_memcpy_h2d": [BYTES]})


def _device_rasters(*holders):
    found = []
    for holder in holders:
        values = list(vars(holder).values()) if hasattr(holder, "__dict__") else [holder]
        found += [v for v in values if isinstance(v, backend.DeviceRaster)]
    return found


OWNERSHIP = {
    "WeightedDInfFlowAccumulation": (lambda o, dev: hd.WeightedDInfFlowAccumulation(o.dem),
                                     lambda o: o.acc),
    "AreaWetnessIndex": (lambda o, dev: hd.AreaWetnessIndex(
        o.dem, dev(o.dem), want=("twi", "spi"), keep_partial_results=True), lambda o: o.dem),
    "DemToDInfWetness": (lambda o, dev: hd.DemToDInfWetness(), lambda o: o.dem),
    "DemToDInfWetness[keep]": (lambda o, dev: hd.DemToDInfWetness(keep_partial_results=True),
                               lambda o: o.dem),
    "DemToDInfWetness[keep, horn, weights]": (lambda o, dev: hd.DemToDInfWetness(
        slope="horn", weights=o.dem, keep_partial_results=True), lambda o: o.dem),
}
FAILS = ("hdem_malloc", "hdem_sinkfill_d8_f32_dev", "hdem_dinf_f32_dev", "hdem_dinfacc_u32_dev",
         "hdem_dinfsum_u32_dev", "hdem_terrain_area_f32_dev", "hdem_dinfsum_u32",
         "hdem_terrain_area_f32")


@pytest.mark.parametrize("name", list(OWNERSHIP))
def test_apply_device_leaves_only_what_it_hands_over(name):
    lib = Recorder()
    held = []
    make, operand = OWNERSHIP[name]

    def run(o, dev):
        f = make(o, dev)
        out = f.apply_device(dev(operand(o)))
        held.extend(_device_rasters(f) + [out])
    _on_stand_in(lib, run)
    ours = {r.ptr for r in held if r._owner}            # pylint: disable=protected-access
    assert lib.live == ours and len(ours) >= 1
    if name.startswith("DemToDInfWetness[keep"):
        assert len(ours) == (5 if "horn" in name else 6)
    for raster in held:
        raster.free()
    assert not lib.live


def _entry_points(name, form):
    """The entry points the call reaches when nothing fails."""
    lib = StandIn()
    make, operand = OWNERSHIP[name]

    def run(o, dev):
        f = make(o, dev)
        out = getattr(f, form)(operand(o) if form == "apply" else dev(operand(o)))
        for raster in _device_rasters(f) + [out]:
            if isinstance(raster, backend.DeviceRaster):
                raster.free()
    _on_stand_in(lib, run)
    return set(lib.log)


@pytest.mark.parametrize("fail", FAILS)
@pytest.mark.parametrize("name", list(OWNERSHIP))
def test_a_failing_c_call_leaves_nothing_allocated(name, fail):
    make, operand = OWNERSHIP[name]
    reached = 0
    for form in ("apply", "apply_device"):
        if fail not in _entry_points(name, form):
            continue
        reached += 1
        lib = StandIn(fail=fail)

        def run(o, dev, form=form):
            f = make(o, dev)
            return getattr(f, form)(operand(o) if form == "apply" else dev(operand(o))), f
        with pytest.raises((ValueError, MemoryError)):
            _on_stand_in(lib, run)
        assert fail in lib.log and not lib.live, (name, form)
    if fail == "hdem_malloc":
        assert reached >= 1
