"""
The CPU references in every elevation regime of tests/elevation_regimes.py, and the D8 tie
rasters: what tests/test_gpu_elevation_regimes.py rests on.  No GPU here.

Per regime, on the "rough" and the integer-metre "srtm" variant: the C priority flood equals
the Jacobi definition bit for bit with and without a gradient, its result is a fixed point of
one more sweep, the C D8 equals the NumPy one, and the two flat-resolution and the two flow-
trace references agree on the fills.  At +8000 m one ulp is 4.9e-4: epsilon = 1e-4 is absorbed
by every addition and gives the surface of epsilon = 0, epsilon = 1e-3 still drains every cell.

The tie rasters: the two drops of every pattern are equal in float32 and unequal in float64,
the oracle takes the first in window order, the strip form is its own fill, and two D8
restatements that break the arithmetic contract (float64 drop; division by 1.4142135f) are
caught by the tie raster and by no cell of the synthetic DEM -- the input every earlier D8
test used.
"""
import numpy as np
import pytest

import oracle
from oracle import c_oracle
from oracle.hdem_oracle_np import D8_OFFSETS
import elevation_regimes as er
from test_flats import resolve_flats_bfs, resolve_flats_walk
from test_flowtrace import trace_doubling, trace_walk

SMALL, WIDE = (96, 140), (200, 333)
CASES = [(name, variant) for name in er.REGIMES for variant in er.VARIANTS]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    c_oracle.build()


def test_the_regimes_reach_what_they_are_named_for():
    z = {name: er.regime_raster(name, WIDE) for name in er.REGIMES}
    assert all(r.dtype == np.float32 and np.isfinite(r).all() for r in z.values())
    assert (z["below_sea"] < 0).all()
    zero = z["zero_cross"] == 0
    assert (z["zero_cross"] < 0).any() and (z["zero_cross"] > 0).any()
    assert (np.signbit(z["zero_cross"]) & zero).any() and (~np.signbit(z["zero_cross"]) & zero).any()
    assert np.spacing(z["high_8000"]).min() > 1e-4 and np.spacing(z["high_8000"]).max() < 1e-3
    assert np.ptp(z["milli"]) < 0.05
    tiny = np.abs(z["tiny"][z["tiny"] != 0])
    assert tiny.min() >= np.finfo(np.float32).tiny and tiny.max() < 1e-28
    assert np.spacing(z["huge_1e30"]).min() > 1e20
    assert (z["near_max"] >= er.HUB_BIG).any() and (z["near_max"] < er.HUB_BIG).any()
    ladder = z["ulp_ladder"].view(np.int32).astype(np.int64) - np.float32(1000.0).view(np.int32)
    assert ladder.min() == 0 and 100 < ladder.max() < 4000
    assert float(z["ulp_ladder"].max()) < 1024.0                      # one binade
    assert er.ulps_from(-300.0, 1) == np.nextafter(np.float32(-300.0), np.float32(0.0))
    assert er.ulps_from(8000.0, -2) == np.float32(8000.0) - np.float32(2 ** -10)


def test_the_basin_raster_overflows_the_span_of_the_coarse_start():
    """What tests/test_gpu_elevation_regimes.py needs of ``near_max_basin``: block maxima under
    the wall whose double is not a float32, in a raster the references agree on."""
    z = er.regime_raster("near_max_basin", WIDE, "rough", True)
    h, w = -(-z.shape[0] // 16) * 16, -(-z.shape[1] // 16) * 16
    pad = np.full((h, w), -np.inf, np.float32)
    pad[:z.shape[0], :z.shape[1]] = np.where(np.isnan(z), np.finfo(np.float32).max, z)
    top = pad.reshape(h // 16, 16, w // 16, 16).max(axis=(1, 3))
    top = top[top < er.HUB_BIG].max()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(2.0) * top)
    for eps in (1e-3, 1e-4):
        _, filled, codes = er.regime_fill("near_max_basin", WIDE, "rough", True, eps)
        assert oracle.sinkfill_is_fixed_point(z, filled, eps)
        assert np.array_equal(codes, oracle.d8_flow_direction(filled))
    # and in the regime itself no block lies under the wall: the coarse raster is all walls
    z = er.regime_raster("near_max", WIDE, "rough", True)
    pad[:z.shape[0], :z.shape[1]] = np.where(np.isnan(z), np.finfo(np.float32).max, z)
    assert (pad.reshape(h // 16, 16, w // 16, 16).max(axis=(1, 3)) >= er.HUB_BIG).all()


@pytest.mark.parametrize("name,variant", CASES)
def test_the_flood_equals_the_jacobi_definition(name, variant):
    z = er.regime_raster(name, SMALL, variant)
    for eps in (0.0, 1e-3, 1e-4):
        want, _ = oracle.sinkfill_jacobi(z, eps)
        assert np.array_equal(er.regime_fill(name, SMALL, variant, False, eps)[1], want), eps


@pytest.mark.parametrize("name,variant", CASES)
def test_the_fill_is_a_fixed_point_and_the_two_d8_agree(name, variant):
    for nodata in (False, True):
        for eps in (0.0, 1e-3):
            z, filled, codes = er.regime_fill(name, WIDE, variant, nodata, eps)
            assert oracle.sinkfill_is_fixed_point(z, filled, eps)
            assert np.array_equal(codes, oracle.d8_flow_direction(filled))
        assert np.array_equal(c_oracle.d8(z), oracle.d8_flow_direction(z))


@pytest.mark.parametrize("name,variant", CASES)
def test_the_flat_references_agree_on_the_exact_fill(name, variant):
    _, filled, codes = er.regime_fill(name, SMALL, variant)
    out, dist = resolve_flats_bfs(filled, codes)
    out_walk, dist_walk = resolve_flats_walk(filled, codes)
    assert np.array_equal(out, out_walk) and np.array_equal(dist, dist_walk)


@pytest.mark.parametrize("name,variant", CASES)
def test_the_trace_references_agree_on_the_gradient_fill(name, variant):
    _, _, codes = er.regime_fill(name, SMALL, variant, False, 1e-3)
    streams = np.zeros(codes.shape, bool)
    streams[::7, ::5] = True
    for mask in (None, streams):
        for a, b in zip(trace_walk(codes, mask), trace_doubling(codes, mask)):
            assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b)


@pytest.mark.parametrize("variant", er.VARIANTS)
def test_at_8000_m_a_small_gradient_is_absorbed_and_a_larger_one_drains(variant):
    z, exact, codes = er.regime_fill("high_8000", WIDE, variant)
    _, absorbed, codes_absorbed = er.regime_fill("high_8000", WIDE, variant, False, 1e-4)
    assert np.array_equal(absorbed, exact) and np.array_equal(codes_absorbed, codes)
    assert (exact > z).any()                                         # something was raised
    assert (codes[1:-1, 1:-1] == 0).any()                             # and flats were left
    _, _, draining = er.regime_fill("high_8000", WIDE, variant, False, 1e-3)
    assert (draining[1:-1, 1:-1] != 0).all()


# ---------------------------------------------------------------------------
# D8 ties
# ---------------------------------------------------------------------------
def _two_drops(z, rows, cols, dtype):
    """(cardinal, diagonal) drop of every centre's two low neighbours, evaluated in ``dtype``
    with the float32 weight."""
    z = z.astype(dtype)
    weight = dtype(np.float32(0.70710678))
    card, diag = [], []
    for y, x in zip(rows, cols):
        low = [(z[y, x] - z[y + dy, x + dx], dy != 0 and dx != 0)
               for dy, dx in D8_OFFSETS if z[y + dy, x + dx] < z[y, x]]
        assert sorted(d for _, d in low) == [False, True]
        card.append(next(drop for drop, d in low if not d))
        diag.append(next(drop for drop, d in low if d) * weight)
    return np.array(card, dtype), np.array(diag, dtype)


@pytest.mark.parametrize("base", er.TIE_BASES)
@pytest.mark.parametrize("form", [er.d8_tie_raster, er.d8_tie_strip])
def test_the_tie_patterns_tie_in_float32_only_and_the_first_in_window_order_wins(form, base):
    z, rows, cols, expected = form(base)
    assert len(expected) == 48 and len(set(zip(rows.tolist(), cols.tolist()))) == 48
    assert z[rows, cols].tolist() == [base] * 48
    card, diag = _two_drops(z, rows, cols, np.float32)
    assert card.dtype == np.float32 and np.array_equal(card, diag)
    card, diag = _two_drops(z, rows, cols, np.float64)
    assert (card != diag).all()
    assert np.abs(card - diag).max() < 1e-3 * np.spacing(np.float32(abs(base)))
    for raster, r, c in ((z, rows, cols), er.shifted_right(z, rows, cols, base)):
        for d8 in (c_oracle.d8, oracle.d8_flow_direction):
            assert np.array_equal(d8(raster)[r, c], expected)
    # both orders occur: the tie goes to the cardinal neighbour in some patterns, to the
    # diagonal one in others (every code but SE, the last of the window)
    assert set(expected.tolist()) == {32, 64, 128, 16, 1, 8, 4}


@pytest.mark.parametrize("base", er.TIE_BASES)
def test_the_tie_strip_is_its_own_fill(base):
    z, rows, cols, _ = er.d8_tie_strip(base)
    assert z.shape == (3, 193)
    for raster in (z, er.shifted_right(z, rows, cols, base)[0]):
        for eps in (0.0, 1e-3):
            assert np.array_equal(c_oracle.sinkfill_pflood(raster, eps=eps), raster)
            assert np.array_equal(oracle.sinkfill_jacobi(raster, eps)[0], raster)


@pytest.mark.parametrize("wrong", [er.d8_drop_in_float64, er.d8_divided_by_sqrt2])
def test_a_d8_that_breaks_the_arithmetic_contract_is_caught_by_the_ties_alone(wrong):
    plain = oracle.synth_dem(60, 80)
    assert np.array_equal(wrong(plain), c_oracle.d8(plain))          # the old input is blind
    for base in er.TIE_BASES:
        for z, rows, cols, expected in (er.d8_tie_raster(base), er.d8_tie_strip(base)):
            got = wrong(z)[rows, cols]
            assert (got != expected).sum() >= 1, base
            assert np.array_equal(c_oracle.d8(z)[rows, cols], expected)
