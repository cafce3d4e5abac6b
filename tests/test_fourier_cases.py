"""
tests/fourier_cases.py without a device: every predicate that tests/test_gpu_fourier_regimes.py
rests on, asserted on the CPU oracle alone.  The launch geometry on figures worked out by hand;
no case has a cell that rounding may decide, so the GPU tests may ask for the oracle's mask
bit for bit; the hits of the two passes are the pairs that were placed; the skip rule of the
second pass is sound on every case, and each of the two smaller rules loses one named pair of
the 300 x 1930 raster; both wide rasters have a FULL block that is skipped and one that finds a
second-pass peak; the 2 M-cell rasters sum every second cell, and a level of half the mean
misses their bar by a factor of five in the CPU's own complex64 chain.
"""
import numpy as np
import pytest

import filter_regimes as fr
import fourier_cases as fc


def by_shape(shape):
    return f"{shape[0]}x{shape[1]}"


def all_cases():
    for name in fc.ORACLE_CASES:
        yield name, fc.oracle_case(name)
    for shape in fc.STATE_SHAPES:
        yield f"state {by_shape(shape)}", fc.state_case(shape)
    for shape in fc.LEVEL_SHAPES:
        for level in fc.LEVELS:
            yield f"{by_shape(shape)}@{level:g}", fc.level_case(shape, level)


# ---------------------------------------------------------------------------
# the geometry, on figures worked out by hand
# ---------------------------------------------------------------------------
def test_the_geometry_on_the_thresholds_themselves():
    assert (fc.WINDOW, fc.R, fc.H4W, fc.OUTW, fc.OCC) == (55, 27, 512, 458, 32)
    assert fc.quadrant((300, 1930)) == (140, 955) and fc.quadrant((131, 131)) == (55, 55)
    assert [fc.block_columns(w) for w in (55, 458, 459, 955, 1990)] == [1, 1, 2, 3, 5]
    assert [fc.first_column(b) for b in range(3)] == [-27, 431, 889]
    # the FULL form needs a block column wholly inside the quadrant: 431 + 512 = 943 columns,
    # a raster 1 906 wide
    assert not fc.is_full(1, 942) and fc.is_full(1, 943) and not fc.is_full(0, 943)
    assert fc.quadrant((300, 1905))[1] == 942 and fc.quadrant((300, 1906))[1] == 943
    assert [fc.is_full(b, 955) for b in range(3)] == [False, True, False]
    assert [fc.is_full(b, 1990) for b in range(5)] == [False, True, True, True, False]
    assert fc.grid((140, 955)) == (3, 5) and fc.grid((55, 1990)) == (5, 2)
    assert fc.grid((1990, 55)) == (1, 63)
    # 8182^2, the raster of the kernel's own notes: 9 x 128 blocks of 32 rows are fewer than
    # 4 096; at 32768^2, 36 x 128 blocks of 128 rows reach it
    assert fc.segment_rows(fc.quadrant((8182, 8182))) == 32
    assert fc.segment_rows(fc.quadrant((32768, 32768))) == 128
    assert [fc.level_step(s) for s in ((1024, 1024), (1447, 1449), (1024, 2048), (1031, 2039),
                                       (2048, 2048))] == [1, 1, 2, 2, 4]


def test_every_case_walks_segments_of_32_rows():
    for name, case in all_cases():
        assert fc.segment_rows(case.q) == 32, name


def test_the_skip_rules_on_one_cell():
    """One first-pass peak at (60, 300) of the 140 x 955 quadrant, occupancy cell (1, 9)."""
    q = (140, 955)
    hits = np.zeros(q, bool)
    hits[60, 300] = True
    occ = fc.occupancy(hits)
    assert occ.shape == (5, 30) and occ.sum() == 1 and occ[1, 9]
    # block column 0 (columns 0 ... 484) sees it from the segments whose rows +- 27 touch rows
    # 32 ... 63: 0 (rows 0 ... 58), 1 and 2 (rows 37 ... 122); no other block column does
    assert fc.visits(occ, q).tolist() == [[True, True, True, False, False], [False] * 5, [False] * 5]
    assert fc.visits(occ, q, fc.visited_without_rows)[0].tolist() == [False, True, False, False, False]
    assert np.array_equal(fc.visits(occ, q, fc.visited_without_context), fc.visits(occ, q))
    # a peak at column 440, occupancy column 13, is context of block column 1 (columns 431 ...
    # 942) and left of its outputs (458 ... 915, occupancy columns 14 ... 28)
    hits[:] = False
    hits[60, 440] = True
    occ = fc.occupancy(hits)
    assert fc.visits(occ, q)[:, 1].tolist() == [True, True, False]
    assert fc.visits(occ, q, fc.visited_without_context)[:, 1].tolist() == [True, False, False]


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def test_no_case_has_a_borderline_cell():
    for name, case in all_cases():
        assert case.dem.dtype == np.float32 and not case.dem.flags.writeable, name
        assert case.borderline() == 0, name
        assert case.mask.dtype == np.uint8 and case.mask.any(), name


@pytest.mark.parametrize("name", list(fc.NOISE_CASES))
def test_the_two_passes_find_the_pairs_that_were_placed(name):
    """The first pass finds the strong pairs and not the weak ones, the second the weak ones;
    whatever else either finds is a lone noise cell that IsolatedPoints removes; the second
    quadrant holds noise alone."""
    case = fc.noise_case(name)
    strong, weak = case.pair_cells(fc.A), case.pair_cells(fc.B)
    assert strong.sum() == weak.sum() == len(case.pairs) and not (strong & weak).any()
    assert (case.first[0] & strong).sum() == strong.sum() and not (case.first[0] & weak).any()
    assert (case.second[0] & weak).sum() == weak.sum()
    assert np.array_equal(case.kept[0], strong | weak)
    assert not case.kept[1].any()
    # the seeds were chosen among those without a borderline cell for having no lone cell either
    assert np.array_equal(case.first[0], strong) and np.array_equal(case.second[0], weak)
    assert not case.first[1].any() and not case.second[1].any()
    # the lines stand where the magnitudes say: amp * H * W / 2, the noise sqrt(H * W)
    n = case.shape[0] * case.shape[1]
    assert case.scale == pytest.approx(fc.A * n / 2, rel=1e-3)


@pytest.mark.parametrize("shape", fc.STATE_SHAPES, ids=by_shape)
def test_the_state_cases_find_their_pairs_and_two_share_a_cell_count(shape):
    case = fc.state_case(shape)
    assert np.array_equal(case.first[0], case.pair_cells(fc.A))
    assert np.array_equal(case.second[0], case.pair_cells(fc.B))
    assert not case.first[1].any() and not case.second[1].any()
    cells = [s[0] * s[1] for s in fc.STATE_SHAPES]
    assert cells[1] == cells[2] != cells[0] and fc.STATE_SHAPES[1] == fc.STATE_SHAPES[2][::-1]


@pytest.mark.parametrize("shape", fc.LEVEL_SHAPES, ids=by_shape)
@pytest.mark.parametrize("level", fc.LEVELS)
def test_the_level_cases_find_their_pairs_and_sum_every_second_cell(level, shape):
    case = fc.level_case(shape, level)
    assert shape[0] * shape[1] >> 20 == 2 and fc.level_step(shape) == 2
    # (at amplitude 5 the weak pair is not hidden from the first pass, which is fine here)
    placed = case.pair_cells(5.0) | case.pair_cells(fc.B)
    assert placed.sum() == 4
    assert np.array_equal(case.kept[0], placed) and not case.kept[1].any()
    assert float(case.dem.mean()) == pytest.approx(level, abs=0.01)


@pytest.mark.parametrize("name", list(fc.SMALL_CASES))
def test_the_smallest_rasters_have_quadrants_of_the_window(name):
    case = fc.small_case(name)
    assert case.q == (fc.WINDOW, fc.WINDOW) and fc.grid(case.q) == (1, 2)
    # one row or column fewer is refused (tests/test_gpu_windows.py: 128 x 130)
    assert min(fc.quadrant((129, 130))) < fc.WINDOW and min(fc.quadrant((130, 129))) < fc.WINDOW
    assert 3 <= case.first[0].sum() <= 13 and 21 <= case.first[1].sum() <= 34
    assert case.second[1].any() and case.kept[0].any() and case.kept[1].any()


def test_the_skip_rule_visits_every_block_with_a_second_pass_hit():
    """The soundness of the rule itself: wherever the oracle's second pass finds a cell, the
    first pass found one in the occupancy cells that the cell's block looks at."""
    seen = 0
    for name, case in all_cases():
        for first, second in zip(case.first, case.second):
            occ = fc.occupancy(first)
            for y, x in np.argwhere(second):
                assert fc.visited(occ, case.q, *fc.block_of(case.q, y, x)), (name, y, x)
                seen += 1
    assert seen >= 4 + 4 + 2 + 4 * 6


def test_each_smaller_rule_loses_one_pair_of_the_300_x_1930_raster():
    case = fc.noise_case("wide_300x1930")
    q, occ = case.q, fc.occupancy(case.first[0])
    # 7 of the 15 blocks of the first quadrant are skipped, all 15 of the second
    assert fc.visits(occ, q).shape == (3, 5) and (~fc.visits(occ, q)).sum() == 7
    assert not fc.visits(fc.occupancy(case.first[1]), q).any()
    upper, right = fc.block_of(q, 70, 305), fc.block_of(q, 112, 462)
    assert upper == (0, 2) and right == (1, 3)
    assert case.second[0][70, 305:307].all() and case.second[0][112, 462:464].all()
    # the first-pass peaks near (70, 305) lie in the 32 rows above its segment ...
    assert not fc.visited_without_rows(occ, q, *upper)
    assert fc.visited_without_context(occ, q, *upper)
    # ... and those near (112, 462) in occupancy column 13, left of its block's output columns
    assert not fc.visited_without_context(occ, q, *right)
    assert fc.visited_without_rows(occ, q, *right)
    assert fc.is_full(right[0], q[1]) and not fc.is_full(upper[0], q[1])


@pytest.mark.parametrize("name", ["wide_300x1930", "wide_130x4000"])
def test_the_wide_rasters_skip_a_full_block_and_find_a_peak_in_another(name):
    case = fc.noise_case(name)
    q = case.q
    table = fc.visits(fc.occupancy(case.first[0]), q)
    full = [bx for bx in range(table.shape[0]) if fc.is_full(bx, q[1])]
    assert len(full) == {"wide_300x1930": 1, "wide_130x4000": 3}[name]
    assert any(not table[bx, by] for bx in full for by in range(table.shape[1]))
    with_hit = {fc.block_of(q, y, x) for y, x in np.argwhere(case.second[0])}
    assert any(bx in full and table[bx, by] for bx, by in with_hit)


def test_the_tall_raster_is_one_block_column_of_63_segments():
    case = fc.noise_case("tall_4000x130")
    assert case.q == (1990, 55) and fc.grid(case.q) == (1, 63)
    table = fc.visits(fc.occupancy(case.first[0]), case.q)[0]
    # the strong pair at row 1020, occupancy row 31, is seen from the segments whose rows +- 27
    # touch rows 992 ... 1023; the weak one at row 1030 lies in the last of them
    assert np.flatnonzero(table).tolist() == [30, 31, 32]


# ---------------------------------------------------------------------------
# the bar of the level test
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fc.LEVEL_SHAPES, ids=by_shape)
def test_the_level_bar_tells_the_mean_from_half_the_mean(shape):
    """The bar at 8 000 m is half an ulp of the output plus 4 x e32.  e32 is far below that
    half ulp, so the bar is the output's rounding; the same complex64 chain on dem - mean / 2
    -- what sum_final_kernel would make of the full count at step 2 -- misses it fivefold."""
    high = fc.LEVELS[0]
    case = fc.level_case(shape, high)
    half_ulp = 0.5 * fr.ulp_of_max(case.dem)
    assert half_ulp == 2.0 ** -12
    e32 = fc.complex64_error(shape, high)
    bar = half_ulp + 4.0 * e32
    halved = fc.complex64_error(shape, high, 0.5)
    print(f"{by_shape(shape)}: e32 {e32:.3e} m, bar {bar:.3e} m, at half the level {halved:.3e} m")
    assert 0.0 < e32 < half_ulp / 4.0
    assert halved > 5.0 * bar
    # at 100 m the bar of tests/filter_regimes.py holds the same chain with room to spare
    assert fc.complex64_error(shape, fc.LEVELS[1]) < 0.5 * fr.bar(fc.level_case(shape, 100.0).dem)
