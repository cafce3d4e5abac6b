"""
The CPU references of the filter branch in every regime of tests/filter_regimes.py: what
tests/test_gpu_filter_regimes.py rests on.  No GPU here.

  * the mirrored launch decisions: 90 rows pin the streaming kernel's strip height to 96 at
    every CU count, and the parent commit's offset cells are where the module says;
  * the bar 1e-6 * max|z| is one the reference alone meets: the bit-faithful restatement
    ``c_oracle.quadratic_ref`` stays within it of ``quadratic_exact64`` for every regime, shape
    and window the GPU file uses (measured: at most 6.9e-7 * max|z|, base raster at window 9), and ``near_max``, which
    is left out there, overflows the reference's own float32 sums;
  * groves x 3: with the tolerance at the bar and the band at max(1e-3, 64 ulp) the
    restatement meets the issue's rule as it stands, with no excused cell, in 52 cases and
    with one in two more; in the two cases of ``SURROUNDINGS_OF_A_FLIP`` it meets it with the
    bounded exception for the window of the one flipped cell, and not without; the band is
    small, and in ``milli`` and ``tiny`` no highlight reaches the threshold;
  * the premise of the outlier tests: the window-local reference gives the same bits, with
    and without one unlike cell, at every cell whose window does not hold it;
  * ``c_oracle.boxmean3`` equals SciPy / NumPy on the bit patterns, signs of zero included,
    and the integer rasters do have ties and results that round to -0.0;
  * the Fourier destripe oracle on the raster cast to float64: one mask in every regime, the
    final |.| folds ``zero_cross``, the float32 oracle within the bar of it;
  * the lagoon oracle commutes with exact power-of-two scalings of the non-void cells.
"""
import numpy as np
import pytest

import oracle
from oracle import c_oracle
import filter_regimes as fr


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    c_oracle.build()


# ---------------------------------------------------------------------------
# mirrored constants
# ---------------------------------------------------------------------------
def test_ninety_rows_are_one_strip_of_96_at_every_cu_count():
    for cus in fr.CUS:
        for ws in (15, 9):
            assert fr.strip_rows((90, 300), ws, cus) == 96
            assert fr.stream_offset_cells((90, 300), ws, cus) == [(48, 128), (48, 299)]
    assert fr.strip_rows((16384, 16384), 15, 256) == 171          # two full rounds
    tiles = fr.tiled_offset_cells((70, 150))
    assert len(tiles) == 9 and tiles[0] == (16, 32) and tiles[-1] == (69, 149)
    assert (48, 96) in tiles and (69, 32) in tiles


def test_the_regimes_are_what_they_are_named_for():
    z = {n: fr.dem(n, (90, 300)) for n in fr.QUADRATIC_REGIMES}
    assert all(np.isfinite(r).all() for r in z.values())
    assert np.ptp(z["steep_x30"][:, :256]) > 300.0                 # inside one strip
    assert (z["below_sea"] < 0).all() and (z["zero_cross"] < 0).any()
    assert np.spacing(z["high_8000"]).min() > 1e-4


# ---------------------------------------------------------------------------
# A3: the bar is one the reference alone meets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ws", fr.QUADRATIC_WINDOWS)
@pytest.mark.parametrize("shape", fr.QUADRATIC_SHAPES)
@pytest.mark.parametrize("name", fr.QUADRATIC_REGIMES + ("base",))
def test_the_restatement_meets_the_bar_against_exact_math(name, shape, ws):
    z, exact, ref = fr.quadratic_case(name, shape, ws)
    err = np.abs(ref.astype(np.float64) - exact).max()
    print(f"{name} {shape} ws {ws}: {err / np.abs(z).max():.2e} of max|z|")
    assert np.isfinite(ref).all() and np.isfinite(exact).all()
    assert err <= fr.bar(z)
    p = ws // 2
    ring = ~fr.far_from(shape, [], 0)
    ring[:p], ring[-p:], ring[:, :p], ring[:, -p:] = True, True, True, True
    assert np.array_equal(fr.bits(ref)[ring], fr.bits(z)[ring])


def test_near_max_overflows_the_reference_itself():
    """Why A3/A4 leave ``near_max`` out: s1 = sum w over 225 cells of 3e38 is past FLT_MAX."""
    for ws in fr.QUADRATIC_WINDOWS:
        z, _, ref = fr.quadratic_case("near_max", (90, 300), ws)
        assert np.isfinite(z).all()
        p = ws // 2
        assert not np.isfinite(ref[p:-p, p:-p]).all()


# ---------------------------------------------------------------------------
# A4: groves x 3
# ---------------------------------------------------------------------------
# cases with one band cell at which groves_ref and groves_exact64 end on different sides of
# the threshold and differ by more than the bar (in every other case: none)
REFERENCES_FLIP = {("high_8000", (128, 203), 21): 1, ("steep_x30", (90, 300), 9): 1,
                   ("steep_x30", (128, 203), 21): 1, ("steep_x30", (90, 300), 21): 1}


@pytest.mark.parametrize("ws", fr.QUADRATIC_WINDOWS)
@pytest.mark.parametrize("shape", fr.QUADRATIC_SHAPES)
@pytest.mark.parametrize("name", fr.QUADRATIC_REGIMES)
def test_the_groves_restatement_has_no_bad_cell_and_a_small_band(name, shape, ws):
    img, groves, want, exact, highlights, masks = fr.groves_case(name, shape, ws)
    delta = fr.groves_delta(img)
    # the reference is up to 6.3 ulp from exact math and the highlight is a difference of two
    # such numbers; 64 ulp is ten times that
    surroundings = fr.surroundings_of_a_flip(name, shape, ws)
    bad_in_band, band = fr.groves_compare(want, exact, highlights, fr.bar(img), delta,
                                          surroundings=surroundings)
    print(f"{name} {shape} ws {ws}: band {band} of {img.size} cells, delta {delta:.3g}")
    # measured: the two references flip no band cell against each other, except in the cases
    # of REFERENCES_FLIP (where the coarse ulp puts real highlights inside 6 ulp of 1.5)
    assert bad_in_band == REFERENCES_FLIP.get((name, shape, ws), 0)
    # ... and every such cell is one at which the two references correct in different passes
    differ, first = fr.references_decide_differently(name, shape, ws)
    bad = np.abs(want - exact) > fr.bar(img)
    assert bad_in_band == int((bad & differ).sum())
    if surroundings is None:
        assert not (bad & ~differ).any()              # the issue's rule as it stands
    else:
        # the exception is needed, is small, and its bound is of the size of what it excuses:
        # without it the rule fails on 1 (window 9) and 5 (window 21) cells around the flip
        cells, bound = surroundings
        excused = bad & ~differ
        assert differ.sum() == 1 and first[differ][0] == 1
        assert excused.sum() == (1 if ws == 9 else 5) and (excused & ~cells).sum() == 0
        assert cells.sum() == ws * ws - 1
        worst = np.abs(want - exact)[excused].max()
        assert 0.5 * bound[cells].max() < worst <= bound[cells].max() < 7e-2
        with pytest.raises(AssertionError):
            fr.groves_compare(want, exact, highlights, fr.bar(img), delta)
    if name != "huge_1e30":
        # measured: at most 53 of 27 000 cells at window 15 (steep_x30; high_8000: 21), 70 of
        # 25 984 over all windows and shapes
        assert band <= (53 if (shape, ws) == ((90, 300), 15) else 3 * img.size // 1000)
    else:
        # every corrected cell has a highlight of a few ulps in the next pass, and nearly every
        # grove cell above its surroundings is corrected: the band is up to 30 % of the raster
        # and the check on the GPU rests on the cap on excused cells alone
        assert band > img.size // 20
    if name in fr.QUIET_REGIMES:
        assert not any(m.any() for m in masks)
        assert max(float(h.max()) for h in highlights) < fr.THRESHOLD - delta
        assert np.abs(want - img).max() <= fr.bar(img)
    else:
        assert masks[0].sum() > 20                                # something is corrected


# ---------------------------------------------------------------------------
# one unlike cell: the reference is window-local
# ---------------------------------------------------------------------------
def _planted(z, cells, value):
    out = z.copy()
    for y, x in cells:
        out[y, x] = value
    return out


@pytest.mark.parametrize("shape,ws", fr.OUTLIER_CASES)
def test_the_reference_does_not_see_an_outlier_outside_its_window(shape, ws):
    z, _, ref = fr.quadratic_case("base", shape, ws)
    cells = fr.offset_cells(shape, ws)
    assert cells
    for cell in cells:
        for value in fr.OUTLIERS + (np.nan, np.inf):
            with np.errstate(all="ignore"):
                got = c_oracle.quadratic_ref(_planted(z, [cell], value), ws)
            far = fr.far_from(shape, [cell], ws // 2)
            assert far.sum() > shape[0] * shape[1] // 2
            assert np.array_equal(fr.bits(got)[far], fr.bits(ref)[far])
    for cell in fr.lattice(shape)[::7]:
        got = c_oracle.quadratic_ref(_planted(z, [cell], -32768.0), ws)
        far = fr.far_from(shape, [cell], ws // 2)
        assert np.array_equal(fr.bits(got)[far], fr.bits(ref)[far])
    block = fr.block_3x4(cells[0], shape)
    assert len(block) == 12 or cells[0][0] in (0, shape[0] - 1) or cells[0][1] >= shape[1] - 2
    got = c_oracle.quadratic_ref(_planted(z, block, -32768.0), ws)
    far = fr.far_from(shape, block, ws // 2)
    assert np.array_equal(fr.bits(got)[far], fr.bits(ref)[far])


@pytest.mark.parametrize("shape,ws", fr.OUTLIER_CASES)
def test_three_groves_passes_reach_three_half_windows(shape, ws):
    img, groves, want, _, _, _ = fr.groves_case("base", shape, ws)
    cell = fr.offset_cells(shape, ws)[0]
    for value in fr.OUTLIERS:
        got = c_oracle.groves_ref(_planted(img, [cell], value), groves, 3, ws)
        far = fr.far_from(shape, [cell], 3 * (ws // 2))
        assert far.any()
        assert np.array_equal(got[far], want[far])


# ---------------------------------------------------------------------------
# A5: the box mean oracle against SciPy / NumPy, on the bit patterns
# ---------------------------------------------------------------------------
def _box_cases():
    for name in fr.BOX_REGIMES:
        yield name, False
    for name in fr.BOX_INTEGER:
        yield name, True


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", fr.BOX_SHAPES)
@pytest.mark.parametrize("name,integer", list(_box_cases()))
def test_the_box_mean_oracle_equals_scipy_on_the_bits(name, integer, shape, dtype):
    from scipy.ndimage import convolve
    x = fr.box_raster(name, shape, dtype, integer)
    with np.errstate(all="ignore"):
        mean = convolve(x, weights=np.ones((3, 3))) / 9
        assert mean.dtype == dtype
        assert np.array_equal(fr.bits(c_oracle.boxmean3(x, False)), fr.bits(mean))
        assert np.array_equal(fr.bits(c_oracle.boxmean3(x, True)), fr.bits(np.around(mean)))
        assert np.array_equal(fr.bits(oracle.boxmean3_round(x)), fr.bits(np.around(mean)))
    if name == "near_max" and dtype == np.float32:
        assert np.isinf(mean).any()                               # the sum of nine overflows
    else:
        assert np.isfinite(mean).all()
    if integer:
        rounded = np.around(mean)
        if name == "zero_cross":
            assert ((mean < 0) & (rounded == 0) & np.signbit(rounded)).any()  # -0.0
        # (a sum of nine integers over 9 is never k + 0.5: the ties are Around's, on halves)
        halves = fr.halves(x)
        assert ((halves < 0) & (halves - np.trunc(halves) == -0.5)).any()
        if name == "zero_cross":
            assert (np.signbit(np.around(halves)) & (np.around(halves) == 0)
                    & (halves != 0)).any()                        # -0.5 -> -0.0


# ---------------------------------------------------------------------------
# Fourier destripe: the float64 oracle in every regime, and float32 against it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fr.FOURIER_SHAPES)
@pytest.mark.parametrize("name", fr.FOURIER_REGIMES)
def test_the_float64_destripe_oracle_in_every_regime(name, shape):
    from oracle import hdem_oracle_fourier as F
    dem, want, mask, borderline = fr.fourier_case(name, shape)
    _, _, base_mask, _ = fr.fourier_case("base", shape)
    print(f"{name} {shape}: mask {int(mask.sum())} cells, {borderline} borderline")
    assert np.isfinite(want).all() and mask.sum() > 500
    # the detection is relative (4 x the hollow mean), a shift moves the zero frequency only
    assert np.array_equal(mask, base_mask)
    assert (want >= 0).all()                                      # the reference returns |elevation|
    if name == "below_sea":
        assert (dem < 0).all()
    if name == "zero_cross":
        folded = (dem < -1.0) & (want > 0.5)
        assert folded.sum() > 1000
    with np.errstate(over="ignore"):
        want32, mask32, _ = F.detect_apply_fourier(dem)
    agree = mask32 == mask
    err = np.abs(want32 - want).max()
    print(f"   float32 oracle: {err:.3e} = {err / np.abs(dem).max():.2e} of max|z|, "
          f"{int((~agree).sum())} mask cells differ")
    assert agree.all()                                            # measured: in every regime
    assert err <= fr.bar(dem)
    assert err <= 5.5e-7 * float(np.abs(dem).max())               # measured: at most 5.46e-7
    # the issue's figures at 256 x 300 (256 x 256: 2 378 cells, 1 borderline margin)
    assert (int(mask.sum()), borderline) == ((2346, 2) if shape == (256, 300) else (2378, 1))


# ---------------------------------------------------------------------------
# lagoon branch: the oracle commutes with exact scalings
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("power", fr.LAGOON_POWERS[1:])
def test_the_lagoon_oracle_commutes_with_powers_of_two(power):
    (hs0, mask0), stages0 = fr.lagoon_case(0)
    (hs, mask), stages = fr.lagoon_case(power)
    assert np.array_equal(mask, mask0) and mask0.sum() > 20
    assert np.array_equal(hs < 0, hs0 < 0)
    for key, base in stages0.items():
        scaled = np.ldexp(base, power)
        if key in ("CorrectNANValues", "GreyDilationInput", "GreyDilation"):   # voids stay as coded
            scaled = np.where(base < 0, base, scaled)
        assert np.array_equal(fr.bits(stages[key]), fr.bits(scaled.astype(base.dtype))), key


def test_the_lagoon_specials_are_what_they_are_named_for():
    hs, fixed, major, grey = fr.lagoon_specials()
    assert np.isinf(major).any() and np.isinf(grey).any()
    zero_lake = major[75:95, 95:120]
    assert (zero_lake == 0).all()
