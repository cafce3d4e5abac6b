"""
D-infinity distance up to the ridge on the MI355X (``DInfDistanceUp``, ``DemToDInfDistanceUp``,
``hdem_dinfdistup_u32``).

The definition and the host reference are those of tests/test_dinfdistup.py.  Every comparison is
byte equality: a cell's value is a fixed sequence of float64 operations on its counted donors'
final values, taken in the order of their position, so the NumPy transcription gives the bits
the kernels give, whatever the schedule.  The words come from the *reference* direction, from
``random_acyclic_words`` or from written-out paths, so the direction kernel cannot reach these
tests.

The operator is one C symbol that takes host or device pointers by a flag, so the table of
tests/device_cases.py does not list it; this file supplies that coverage itself: both forms,
poisoned scratch and output memory, and a caller's stream behind an unfinished producer, on a
second context (with the machinery of tests/test_gpu_scribble.py and tests/test_gpu_streams.py).
"""
import ctypes
import math

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
import size_regimes as sr
from hydrodem_amd import backend, dinf
from hydrodem_amd.backend import DeviceRaster
from hydrodem_amd.dinf import Q_ONE
from test_dinf import direction_ref, random_dem
from test_dinfdist import KINDS, STATISTICS, same_bits, ulps_apart
from test_dinfdistup import SHARES, counts_up_of, distance_up_ref
from test_gpu_dinf import loop_cells, random_acyclic_words
from test_gpu_flowacc import path_codes, spiral
from test_gpu_scribble import Case, assert_same_bytes, execute
from test_gpu_streams import Delay, on_a_callers_stream

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(130, 197), (1, 200), (65, 1), (64, 128), (200, 70)]
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731
FREE = ("ridge_cells", "counted_links", "ignored_links", "merge_cells", "nan_cells", "invalid",
        "outside", "unresolved", "tile_h", "tile_w")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def schedule_free(stats):
    return {k: stats[k] for k in FREE}


def assert_distance(words, dem=None, kind="horizontal", statistic="average", cellsize=1.0,
                    min_share=16384, want=None):
    """The host form against the reference: the bytes and the counts that no schedule changes."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    dx, dy = dinf.cellsizes(cellsize)
    if want is None:
        want = distance_up_ref(words, dem, kind, statistic, dx, dy, min_share)
    got, stats = dinf.dinfdistup(words, dem, cellsize, kind, statistic, min_share=min_share)
    assert got.dtype == F32 and got.shape == words.shape
    differ = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(differ), [(tuple(c), got[tuple(c)], want[tuple(c)]) for c in differ[:5]]
    assert schedule_free(stats) == counts_up_of(words, min_share, want)
    assert stats["rounds"] >= 1 and stats["tile_visits"] >= sr.tiles_of(words.shape)
    return got, stats


def rough_elevations(shape, seed):
    """Elevations that have nothing to do with the words, some NaN, some infinite."""
    rng = np.random.default_rng(seed)
    z = (rng.random(shape) * 100).astype(F32)
    z[rng.random(shape) < 0.01] = np.nan
    z[rng.random(shape) < 0.005] = np.inf
    z[rng.random(shape) < 0.005] = -np.inf
    return z


# ---------------------------------------------------------------------------
# the reference's own direction, and random acyclic words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_distance_on_the_reference_direction(shape, kind):
    cellsize = (30.0, 20.0) if kind != "vertical" else 1.0
    z = random_dem(shape, seed=shape[0] * 7 + shape[1], nan=0.01)
    words = direction_ref(z, *dinf.cellsizes(cellsize))[0]
    dem = None if kind == "horizontal" else z
    merges = []
    for statistic in STATISTICS:
        for min_share in (16384, 1):
            _, stats = assert_distance(words, dem, kind, statistic, cellsize, min_share)
            merges.append(stats["merge_cells"])
    if min(shape) > 2:
        assert merges[1] > merges[0] > 0                   # both branches of the statistic ran


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_distance_on_random_acyclic_words(shape):
    words = random_acyclic_words(shape, seed=shape[0] * 3 + shape[1])
    z = (np.random.default_rng(shape[0]).random(shape) * 100).astype(F32)
    for min_share in SHARES:
        for statistic in STATISTICS:
            assert_distance(words, None, "horizontal", statistic, 1.0, min_share)
            assert_distance(words, z, "surface", statistic, (2.0, 3.0), min_share)
        assert_distance(words, z, "vertical", "average", 1.0, min_share)
    if min(shape) > 1:
        low, whole = (counts_up_of(words, s, np.zeros(shape, F32)) for s in (1, 32768))
        assert low["merge_cells"] > whole["merge_cells"] > 0
        assert whole["ignored_links"] > 0.2 * words.size and low["ignored_links"] == 0


# ---------------------------------------------------------------------------
# long dependency chains
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles_with_its_ridge_cell_at_the_far_end(upright):
    n = 4097
    cells = [(2, x) for x in range(n)]
    want = np.zeros((5, n), F32)
    want[2] = np.arange(n, dtype=F32)
    shape = (5, n)
    if upright:
        cells, want, shape = [(x, y) for y, x in cells], np.ascontiguousarray(want.T), (n, 5)
    words = dinf.words_from_d8(path_codes(shape, cells))
    # the last cell waits for 4096 cells in 65 tiles: a seam per round at the least
    for statistic in ("average", "maximum"):
        _, stats = assert_distance(words, None, "horizontal", statistic, want=want)
        assert stats["rounds"] >= 64
        assert stats["ridge_cells"] == 4 * n + 1 and stats["counted_links"] == n - 1
    z = np.zeros(shape, F32)
    for k, c in enumerate(cells):
        z[c] = 200.0 - k * 2.0 ** -6
    rise, stats = assert_distance(words, z, "vertical", min_share=32768)
    assert rise[cells[-1]] == F32((n - 1) * 2.0 ** -6) and stats["rounds"] >= 64


def test_a_zigzag_of_1000_diagonal_steps_along_a_tile_seam():
    cells = [(k, 63 + k % 2) for k in range(1001)]         # crosses column 63 | 64 every step
    words = dinf.words_from_d8(path_codes((1001, 128), cells))
    got, stats = assert_distance(words)
    assert stats["rounds"] > 1
    # 1000 sequential float64 additions of sqrt 2 stay within one float32 step of the product
    assert ulps_apart(got[1000:1001, 63], np.array([1000 * math.sqrt(2.0)], F32)).max() <= 1
    assert_distance(words, None, "horizontal", "minimum", (3.0, 0.25), 32768)


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    words = dinf.words_from_d8(path_codes(shape, cells))
    want = np.zeros(shape, F32)
    for k, c in enumerate(cells):
        want[c] = k                                        # all steps are cardinal
    assert_distance(words, want=want)
    z = np.random.default_rng(offset).random(shape).astype(F32)
    for kind in ("vertical", "surface"):
        assert_distance(words, z, kind, "maximum")


def test_a_cone_where_nearly_every_cell_merges_two_donors():
    rows, cols = np.mgrid[0:200, 0:200]
    z = (-np.hypot(rows - 99.5, cols - 99.5)).astype(F32)
    words = direction_ref(z)[0]
    for kind in KINDS:
        for statistic in STATISTICS:
            got, stats = assert_distance(words, None if kind == "horizontal" else z, kind,
                                         statistic, 1.0, 1)
            assert np.isfinite(got).all() and stats["merge_cells"] > 0.9 * 198 * 198
    assert_distance(words, None, "horizontal", "average", 1.0, 16384)


def test_a_pit_whose_centre_waits_for_the_whole_raster():
    rows, cols = np.mgrid[0:199, 0:199]
    z = np.hypot(rows - 99, cols - 99).astype(F32)
    words = direction_ref(z)[0]
    assert words[99, 99] == 0
    for kind in KINDS:
        for statistic in STATISTICS:
            got, _ = assert_distance(words, None if kind == "horizontal" else z, kind, statistic,
                                     1.0, 1)
            assert np.isfinite(got).all()
    far, _ = assert_distance(words, None, "horizontal", "maximum", 1.0, 1)
    assert far[99, 99] == far.max() >= 98 * math.sqrt(2.0)
    assert_distance(words, z, "surface", "average", (2.0, 0.5), 16384)


def test_a_strip_whose_schedule_kernel_spans_two_workgroups():
    shape = sr.DINF_SHAPES[1]
    assert sr.schedule_blocks(shape) >= 2 and sr.tiles_of(shape) > 256
    words = random_acyclic_words(shape, seed=sr.DINF_SEED)
    _, stats = assert_distance(words, None, "horizontal", "minimum", 1.0, 1)
    assert stats["rounds"] >= 2
    assert_distance(words)


# ---------------------------------------------------------------------------
# the threshold, where the donor lies in the halo
# ---------------------------------------------------------------------------
def test_a_link_across_a_seam_counts_at_min_share_and_not_one_below():
    share = 12345
    words = np.zeros((130, 130), np.uint32)
    for y in (10, 20):                                     # two runs east, up to column 62
        words[y, 50:63] = dinf.pack(1, 0)
    for x in (10, 30):                                     # two runs south, up to row 62
        words[50:63, x] = dinf.pack(6, 0)
    words[10, 63] = dinf.pack(1, Q_ONE - share)            # east across the seam: `share`
    words[20, 63] = dinf.pack(1, Q_ONE - share + 1)        # one unit less
    words[63, 10] = dinf.pack(6, Q_ONE - share)            # south across the seam
    words[63, 30] = dinf.pack(6, Q_ONE - share + 1)
    for k in range(1, 24):                                 # two diagonals into the corner where
        words[63 - k, 63 - k] = dinf.pack(7, Q_ONE)        # four tiles meet: south-east ...
        words[64 + k, 63 - k] = dinf.pack(1, Q_ONE)        # ... and north-east
    words[63, 63] = dinf.pack(7, share)                    # south-east across the corner: `share`
    words[64, 63] = dinf.pack(1, share - 1)                # north-east across it: one unit less
    for kind in KINDS:
        z = None if kind == "horizontal" else random_dem(words.shape, seed=1)
        for statistic in STATISTICS:
            got, stats = assert_distance(words, z, kind, statistic, 1.0, share)
            assert stats["ignored_links"] == 3
    got, _ = assert_distance(words, None, "horizontal", "maximum", 1.0, share)
    r2 = math.sqrt(2.0)
    diagonal = np.cumsum(np.full(24, r2))                  # summed step by step, as the operator does
    assert got[10, 63] == 13 and got[10, 64] == 14 and got[9, 64] == F32(13 + r2)
    assert got[20, 63] == 13 and got[20, 64] == 0 and got[19, 64] == F32(13 + r2)
    assert got[63, 10] == 13 and got[64, 10] == 14 and got[64, 30] == 0
    assert got[63, 63] == F32(diagonal[22]) and diagonal[23] < diagonal[22] + 1 + 1
    assert got[64, 63] == F32(diagonal[22] + 1)            # from (63, 63); from (65, 62) it is less
    assert got[64, 64] == F32(diagonal[22] + 1 + 1)        # by way of (64, 63), not straight
    assert got[63, 64] == 0                                # what (64, 63) sends north-east
    # one unit more and the three links at the threshold go, too
    _, stats = assert_distance(words, min_share=share + 1)
    assert stats["ignored_links"] == 6


def test_nan_and_infinite_elevations_leave_one_nan_bit_pattern():
    words = random_acyclic_words((130, 197), seed=12)
    z = rough_elevations(words.shape, seed=12)
    nans = {}
    for kind in ("vertical", "surface"):
        for statistic in STATISTICS:
            got, stats = assert_distance(words, z, kind, statistic, (2.0, 3.0), 1)
            assert set(got.view(np.uint32)[np.isnan(got)].tolist()) == {0x7FC00000}
            assert np.isinf(got).any()
            nans[kind, statistic] = stats["nan_cells"]
        assert nans[kind, "average"] >= nans[kind, "maximum"] > nans[kind, "minimum"] > 0


# ---------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------
def test_two_runs_and_both_forms_give_identical_bytes():
    words = random_acyclic_words((257, 130), seed=21)
    z = (np.random.default_rng(21).random(words.shape) * 50).astype(F32)
    for kind, dem in (("horizontal", None), ("surface", z)):
        a, stats_a = dinf.dinfdistup(words, dem, 1.0, kind, min_share=1)
        b, _ = dinf.dinfdistup(words, dem, 1.0, kind, min_share=1)
        with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
                backend.on_device(dem, dtype=F32) as dz, \
                DeviceRaster.empty(words.shape, F32, dw.ctx) as mine:
            dev, stats_c = dinf.dinfdistup_dev(dw, dz, 1.0, kind, min_share=1)
            with dev:
                c = dev.to_host()
            same, _ = dinf.dinfdistup_dev(dw, dz, 1.0, kind, min_share=1, out=mine)
            assert same is mine and mine.to_host().tobytes() == a.tobytes()
            op = hd.DInfDistanceUp(kind, dem=dz, min_share=1)
            with op.apply_device(dw) as one:
                assert one.dtype == F32 and one.to_host().tobytes() == a.tobytes()
            assert op.apply(words).tobytes() == a.tobytes()
            assert schedule_free(op.stats) == schedule_free(stats_a)
        assert a.tobytes() == b.tobytes() == c.tobytes()
        assert schedule_free(stats_a) == schedule_free(stats_c)
        assert same_bits(a, distance_up_ref(words, dem, kind, min_share=1))
    # the proportion is the share's ceiling
    half, _ = dinf.dinfdistup(words, min_proportion=0.5)
    assert same_bits(half, distance_up_ref(words, min_share=16384))
    assert same_bits(hd.DInfDistanceUp().apply(words), half)
    assert same_bits(hd.DInfDistanceUp(min_proportion=0.3).apply(words),
                     distance_up_ref(words, min_share=9831))


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    words = random_acyclic_words((300, 300), seed=9)
    ctx = backend.context()
    op = hd.DInfDistanceUp()
    op.apply(words)
    assert op.stats["ms_classify"] == 0 and op.stats["ms_relax"] == 0 and op.stats["ms_final"] == 0
    ctx.profile(True)
    try:
        op.apply(words)
    finally:
        ctx.profile(False)
    assert op.stats["ms_classify"] > 0 and op.stats["ms_relax"] > 0 and op.stats["ms_final"] > 0
    assert "struct_size" not in op.stats and "reserved" not in op.stats


# ---------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_300_500():
    z = hdem_synth.synth_dem(300, 500)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("flats,epsilon", [("keep", 1e-3), ("resolve", 0.0)])
def test_the_chain_against_the_reference_on_its_own_stages(synth_300_500, flats, epsilon):
    chain = hd.DemToDInfDistanceUp(epsilon=epsilon, flats=flats, keep_partial_results=True)
    got = chain.apply(synth_300_500)
    assert chain.filled.dtype == F32 and chain.codes.dtype == np.uint8
    want_words, _, _, taken = direction_ref(chain.filled, fallback=chain.codes)
    assert np.array_equal(chain.words, want_words)
    want = distance_up_ref(want_words)
    counts = counts_up_of(want_words, 16384, want)
    cells = want.size
    print(f"{flats}: ridge {counts['ridge_cells'] / cells:.4f}, merge "
          f"{counts['merge_cells'] / cells:.4f}, ignored links {counts['ignored_links']}, "
          f"longest {want.max():.1f}")
    # both branches of the statistic and of the threshold are exercised, by the reference's own
    # account
    assert counts["merge_cells"] >= 0.05 * cells and counts["ignored_links"] >= 0.02 * cells
    assert 0.1 * cells <= counts["ridge_cells"] <= 0.9 * cells and want.max() >= 3
    assert same_bits(got, want)
    assert chain.stats["DInfFlowDirection"]["fallback_cells"] == taken
    assert schedule_free(chain.stats["DInfDistanceUp"]) == counts
    assert ("ResolveFlats" in chain.stats) == (flats == "resolve")
    assert set(chain.stats) - {"ResolveFlats"} == {"SinkFill", "DInfFlowDirection",
                                                  "DInfDistanceUp"}
    # without the stages kept, on the device; the rise on the filled DEM; the surface minimum
    plain = hd.DemToDInfDistanceUp(epsilon=epsilon, flats=flats)
    with DeviceRaster.from_host(synth_300_500, dtype=F32) as dz, plain.apply_device(dz) as up:
        assert up.dtype == F32 and same_bits(up.to_host(), want)
    assert plain.filled is None and plain.codes is None and plain.words is None
    rise = hd.DemToDInfDistanceUp(kind="vertical", statistic="maximum", min_share=1,
                                  epsilon=epsilon, flats=flats)
    assert same_bits(rise.apply(synth_300_500),
                     distance_up_ref(want_words, chain.filled, "vertical", "maximum", min_share=1))
    along = hd.DemToDInfDistanceUp(kind="surface", statistic="minimum", min_proportion=0.25,
                                   cellsize=(30.0, 20.0), epsilon=epsilon, flats=flats,
                                   keep_partial_results=True)
    got = along.apply(synth_300_500)
    assert same_bits(got, distance_up_ref(along.words, along.filled, "surface", "minimum", 30.0,
                                          20.0, 8192))


# ---------------------------------------------------------------------------
# refusals: argument errors that the library returns; the context stays usable
# ---------------------------------------------------------------------------
def test_invalid_words_are_refused_with_their_count():
    words = random_acyclic_words((70, 90), seed=2)
    kinds = {"facet > 8": 9 << 16, "q > 32768": (3 << 16) | (Q_ONE + 1), "facet 0 with q": 7,
             "stray bit 20": (2 << 16) | (1 << 20), "stray bit 31": 1 << 31}
    for n, (kind, word) in enumerate(kinds.items(), 1):
        bad = words.copy()
        bad[5:5 + n, 66] = word
        with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells: the facet"):
            hd.DInfDistanceUp().apply(bad)
        with DeviceRaster.from_host(bad, dtype=np.uint32) as dw:
            with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells"):
                hd.DInfDistanceUp(min_share=1).apply_device(dw)
        with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells"):
            distance_up_ref(bad)
        assert kind
    assert_distance(words)


def test_a_receiver_outside_the_raster_is_refused():
    words = np.zeros((66, 70), np.uint32)
    words[0, 3] = dinf.pack(2, 0)                         # north of the first row
    words[65, 69] = dinf.pack(8, 100)                     # east is outside, south-east too
    words[30, 69] = dinf.pack(1, Q_ONE)                   # north-east only, outside
    words[30, 0] = dinf.pack(1, Q_ONE)                    # north-east only, inside
    with pytest.raises(ValueError, match="send flow outside the raster in 3 cells"):
        hd.DInfDistanceUp().apply(words)
    with pytest.raises(ValueError, match="outside the raster in 3 cells"):
        distance_up_ref(words)


def test_a_cycle_of_counted_links_is_refused_in_bounded_time_and_an_ignored_link_cuts_it():
    words = np.zeros((40, 130), np.uint32)
    words[7, 7:9] = dinf.pack(np.array([1, 4]), np.array([0, 0]))     # E then W: a 2-cycle
    with pytest.raises(ValueError, match="cycle of counted links: 2 cells never resolve"):
        hd.DInfDistanceUp().apply(words)
    cells = loop_cells(10, 59, 11)                        # across the seam at column 64
    assert len(cells) == 40
    words = dinf.words_from_d8(path_codes((40, 130), cells + cells[:1]))
    words[3, 3] = dinf.pack(7, 1000)                      # a cell that does resolve
    words[9, 58] = dinf.pack(7, Q_ONE)                    # one that drains into the loop: a ridge
    assert cells[20] == (20, 69) and words[20, 69] == dinf.pack(4, 0)
    words[20, 69] = dinf.pack(5, 9000)                    # 23768 W along the loop, 9000 SW out
    words[21, 11:69] = dinf.pack(4, 0)                    # of it, and west across the seam
    waits = len(cells) + 58 + 1                           # the run, and the cell it ends in
    for min_share in (1, 9000):                           # the loop, and the run that waits on it
        with pytest.raises(ValueError, match=f"{waits} cells never resolve"):
            hd.DInfDistanceUp(min_share=min_share).apply(words)
        with pytest.raises(ValueError, match=f"{waits} cells never resolve"):
            distance_up_ref(words, min_share=min_share)
    with pytest.raises(ValueError, match="40 cells never resolve"):
        hd.DInfDistanceUp(min_share=9001).apply(words)    # the run starts from a ridge cell now
    # the same cycle with one link below min_share is an open path
    for min_share in (23769, Q_ONE):
        for statistic in STATISTICS:
            got, stats = assert_distance(words, None, "horizontal", statistic, 1.0, min_share)
            assert stats["unresolved"] == 0
            assert stats["ignored_links"] == 3 + (min_share == Q_ONE)     # (3, 3) sends 31768 S
            assert got[cells[21]] == 0 and got[9, 58] == 0 and got[21, 68] == 0
            if statistic == "maximum":                     # (10, 59) also hears from (9, 58)
                assert got[cells[20]] == 39
    z = np.random.default_rng(5).random((40, 130)).astype(F32)
    assert_distance(words, z, "vertical", "average", 1.0, 23769)


def test_an_output_of_the_wrong_dtype_is_refused_and_the_c_entry_point_checks_its_arguments():
    words = random_acyclic_words((20, 30), seed=4)
    z = random_dem((20, 30), seed=4)
    ctx = backend.context()
    dev = dinf.ON_DEVICE
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.from_host(z, dtype=F32) as dz, \
            DeviceRaster.empty(words.shape, np.uint32, ctx) as wrong, \
            DeviceRaster.empty((20, 31), F32, ctx) as wide, \
            DeviceRaster.empty(words.shape, F32, ctx) as right:
        with pytest.raises(ValueError, match="out is float32, got uint32"):
            dinf.dinfdistup_dev(dw, out=wrong)
        with pytest.raises(ValueError, match=r"out is \(20, 31\), the words \(20, 30\)"):
            dinf.dinfdistup_dev(dw, out=wide)
        got, _ = dinf.dinfdistup_dev(dw, out=right)
        assert got is right and same_bits(right.to_host(), distance_up_ref(words))

        fn = ctx.lib.hdem_dinfdistup_u32

        def call(words=dw.ptr, dem=None, dx=1.0, dy=1.0, what=0, statistic=0, min_share=16384,
                 out=right.ptr, flags=dev, stats=None):
            return fn(ctx.handle, words, 20, 30, dem, dx, dy, what, statistic, min_share, out,
                      flags, stats)

        def refused(text, **kw):
            assert call(**kw) == backend.BAD_ARG
            assert text in ctx.lib.hdem_last_error(), ctx.lib.hdem_last_error()

        assert call() == backend.OK
        refused(b"null raster pointer", words=None)
        refused(b"null raster pointer", out=None)
        refused(b"need the dem", what=1)
        refused(b"need the dem", what=2)
        refused(b"takes no dem", dem=dz.ptr)
        refused(b"unknown distance kind 3", what=3)
        refused(b"unknown distance kind -1", what=-1)
        refused(b"unknown distance statistic 3", statistic=3)
        refused(b"unknown distance statistic -1", statistic=-1)
        for bad in (0, Q_ONE + 1, 0xFFFFFFFF):
            refused(b"min_share is 1 ... 32768", min_share=bad)
        assert call(min_share=1) == call(min_share=Q_ONE) == backend.OK
        for flags in (1, dev | 2, -1):
            refused(b"unknown flags", flags=flags)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(b"dx and dy must be finite and positive", dx=bad)
            refused(b"dx and dy must be finite and positive", dy=bad)
        # an output that overlaps an input, by one cell at either end
        refused(b"distance overlaps words", out=dw.ptr)
        refused(b"distance overlaps words", out=dw.ptr + 4 * (20 * 30 - 1))
        refused(b"distance overlaps words", words=right.ptr + 4 * (20 * 30 - 1))
        refused(b"distance overlaps dem", what=1, dem=dz.ptr, out=dz.ptr)
        refused(b"distance overlaps dem", what=2, dem=right.ptr + 4)
        st = backend._DInfDistUpStats()                    # pylint: disable=protected-access
        st.struct_size = 0
        refused(b"struct_size", stats=ctypes.byref(st))
        st = backend._DInfDistUpStats()                    # pylint: disable=protected-access
        st.struct_size = 24                                # a shorter struct
        st.counted_links, st.tile_h = -5, -7
        assert call(stats=ctypes.byref(st)) == backend.OK
        assert st.struct_size == 24
        assert st.ridge_cells == counts_up_of(words, 16384, np.zeros((20, 30), F32))["ridge_cells"]
        assert st.counted_links == -5 and st.tile_h == -7    # nothing beyond it is written
        fake = ctypes.c_void_p(256)                        # never dereferenced
        for flags in (0, dev):
            assert fn(ctx.handle, fake, 65536, 65536, None, 1.0, 1.0, 0, 0, 16384, fake, flags,
                      None) == backend.BAD_ARG
            assert b"2^32" in ctx.lib.hdem_last_error()
        assert fn(None, dw.ptr, 20, 30, None, 1.0, 1.0, 0, 0, 16384, right.ptr, dev,
                  None) == backend.BAD_ARG
        assert ctx.lib.hdem_last_error() == b"ctx is null"
    # the context is as usable as before
    assert_distance(words)


# ---------------------------------------------------------------------------
# poisoned scratch and output memory, and a caller's stream
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=33):
    words = direction_ref(random_dem(shape, seed=seed, nan=0.01))[0]
    return {"words": words, "z": rough_elevations(shape, seed)}


def poison_run(call, inp):
    """The horizontal average at a half, the surface maximum and the vertical minimum over
    every link."""
    dw, dz = call.up(inp["words"]), call.up(inp["z"])
    host, stats = {}, {}
    for name, args in (("horizontal", (None, 1.0, "horizontal", "average", 0.5)),
                       ("surface", (dz, (2.0, 3.0), "surface", "maximum", 2.0 ** -15)),
                       ("vertical", (dz, 1.0, "vertical", "minimum", 2.0 ** -15))):
        out = call.out(dw.shape, F32)
        got, st = dinf.dinfdistup_dev(dw, *args, out=out)
        assert not call.own or got is out
        host[name] = call.host(got)
        stats.update({f"{name}_{k}": v for k, v in schedule_free(st).items()})
    return host, stats


def poison_check(inp, got):
    words, z = inp["words"], inp["z"]
    assert same_bits(got["horizontal"], distance_up_ref(words))
    assert same_bits(got["surface"], distance_up_ref(words, z, "surface", "maximum", 2.0, 3.0, 1))
    assert same_bits(got["vertical"], distance_up_ref(words, z, "vertical", "minimum",
                                                      min_share=1))


POISON_CASE = Case("dinfdistup", ((130, 197),), poison_inputs, poison_run, poison_check, True,
                   frozenset())


@pytest.fixture(scope="module")
def clean_runs():
    """Inputs and the run on a fresh context's own stream, once per ``own``."""
    runs = {}

    def run(own):
        if own not in runs:
            inputs = POISON_CASE.build((130, 197))
            got, stats = execute(POISON_CASE, inputs, None, own)
            POISON_CASE.check(inputs, got)
            runs[own] = (inputs, got, stats)
        return runs[own]
    return run


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
def test_poisoned_memory_changes_no_byte(clean_runs, own):
    inputs, clean, clean_stats = clean_runs(own)
    for byte in (0x00, 0xA5, 0xFF):
        got, stats = execute(POISON_CASE, inputs, byte, own)
        assert stats == clean_stats
        assert_same_bytes(got, clean, f"dinfdistup under {byte:#04x}")


@pytest.fixture(scope="module")
def delay():
    return Delay()


def test_a_callers_stream_behind_an_unfinished_producer_changes_no_byte(clean_runs, delay):
    inputs, want, want_stats = clean_runs(False)
    got, stats = on_a_callers_stream(POISON_CASE, inputs, want, False)
    assert_same_bytes(got, want, "dinfdistup on an idle stream of the caller's")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"dinfdistup behind the delay, out= {whose}"
        got, stats = on_a_callers_stream(POISON_CASE, inputs, want, own, delay)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
