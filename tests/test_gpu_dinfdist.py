"""
D-infinity distance down and HAND on the MI355X (``DInfDistanceDown``,
``DInfHeightAboveDrainage``, ``DemToDInfHAND``, ``hdem_dinfdist_u32``).

The definition and the host reference are those of tests/test_dinfdist.py.  Every comparison is
byte equality: a cell's value is a fixed sequence of float64 operations on its receivers' final
values, so the NumPy transcription gives the bits the kernels give, whatever the schedule.  The
words come from the *reference* direction or from ``random_acyclic_words``, so the direction
kernel cannot reach these tests.

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
from test_dinfdist import (KINDS, STATISTICS, counts_of, d8_case, distance_ref, same_bits,
                           stops_of, ulps_apart)
from test_flowacc import acc_kahn
from test_gpu_dinf import loop_cells, random_acyclic_words
from test_gpu_flowacc import path_codes, spiral
from test_gpu_scribble import Case, assert_same_bytes, execute
from test_gpu_streams import Delay, on_a_callers_stream

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(130, 197), (1, 200), (65, 1), (64, 128), (200, 70)]
IDS = lambda s: f"{s[0]}x{s[1]}"                           # noqa: E731
FREE = ("split_cells", "terminal_cells", "stop_cells", "unreached_cells", "invalid", "outside",
        "unresolved", "tile_h", "tile_w")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def split_cells(words):
    q = words & 0xFFFF
    return int(((q != 0) & (q != Q_ONE)).sum())


def schedule_free(stats):
    return {k: stats[k] for k in FREE}


def assert_distance(words, streams=None, threshold=None, dem=None, kind="horizontal",
                    statistic="average", cellsize=1.0, want=None):
    """The host form against the reference: the bytes and the counts that no schedule changes."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    dx, dy = dinf.cellsizes(cellsize)
    stops = stops_of(words, streams, threshold)
    if want is None:
        want = distance_ref(words, stops, dem, kind, statistic, dx, dy)
    got, stats = dinf.dinfdist(words, streams, threshold, dem, cellsize, kind, statistic)
    assert got.dtype == F32 and got.shape == words.shape
    differ = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(differ), [(tuple(c), got[tuple(c)], want[tuple(c)]) for c in differ[:5]]
    assert schedule_free(stats) == counts_of(words, stops, want)
    assert stats["rounds"] >= 1 and stats["tile_visits"] >= sr.tiles_of(words.shape)
    return got, stats


def stream_forms(words, seed):
    """(streams, threshold) twice: a mask that holds most of the cells without outflow and one
    cell in twenty of the rest, and a uint32 raster that is a stop where it is >= 40."""
    rng = np.random.default_rng(seed)
    shape = words.shape
    mask = (rng.random(shape) < 0.05) | ((words >> 16 == 0) & (rng.random(shape) < 0.8))
    acc = np.where(mask, rng.integers(40, 1000, shape), rng.integers(0, 40, shape))
    return (mask, None), (acc.astype(np.uint32), 40)


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
    nans = []
    for streams, threshold in stream_forms(words, shape[1]):
        for statistic in STATISTICS:
            got, _ = assert_distance(words, streams, threshold, dem, kind, statistic, cellsize)
            nans.append(int(np.isnan(got).sum()))
    assert nans[:3] == nans[3:]                            # the two forms name the same set
    if min(shape) > 1:
        assert nans[0] == nans[2] > nans[1] > 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_distance_on_random_acyclic_words(shape):
    words = random_acyclic_words(shape, seed=shape[0] * 3 + shape[1])
    assert min(shape) == 1 or split_cells(words) > 0.05 * words.size
    rng = np.random.default_rng(shape[0])
    z = (rng.random(shape) * 100).astype(F32)
    for share in (0.02, 0.3):
        mask = rng.random(shape) < share
        for statistic in STATISTICS:
            assert_distance(words, mask, None, None, "horizontal", statistic)
            assert_distance(words, mask, None, z, "surface", statistic, (2.0, 3.0))
        assert_distance(words, mask, None, z, "vertical")
    assert_distance(words)                                 # to the cells without outflow
    # an empty stop set: everything is NaN, and nothing hangs
    got, stats = assert_distance(words, np.zeros(shape, bool))
    assert np.isnan(got).all() and stats["stop_cells"] == 0
    assert stats["unreached_cells"] == words.size


# ---------------------------------------------------------------------------
# long dependency chains
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_65_tiles_with_the_stop_at_the_far_end(upright):
    n = 4097
    cells = [(2, x) for x in range(n)]
    want = np.full((5, n), np.nan, F32)
    want[2] = np.arange(n - 1, -1, -1, dtype=F32)
    shape = (5, n)
    if upright:
        cells, want, shape = [(x, y) for y, x in cells], np.ascontiguousarray(want.T), (n, 5)
    words = dinf.words_from_d8(path_codes(shape, cells))
    stop = np.zeros(shape, bool)
    stop[cells[-1]] = True
    want.view(np.uint32)[np.isnan(want)] = 0x7FC00000
    _, stats = assert_distance(words, stop, want=want)
    # (a tile hop per round, unless a tile happens to see its neighbour's cells of the same round)
    assert stats["rounds"] > 1 and stats["unreached_cells"] == 4 * n
    z = np.zeros(shape, F32)
    for k, c in enumerate(cells):
        z[c] = 200.0 - k * 2.0 ** -6
    drop, _ = assert_distance(words, stop, None, z, "vertical")
    assert drop[cells[0]] == F32((n - 1) * 2.0 ** -6)


def test_a_zigzag_of_1000_diagonal_steps_along_a_tile_seam():
    cells = [(k, 63 + k % 2) for k in range(1001)]         # crosses column 63 | 64 every step
    words = dinf.words_from_d8(path_codes((1001, 128), cells))
    got, stats = assert_distance(words)                    # to the path's end, and 0 off the path
    assert stats["rounds"] > 1                             # the worst case: about one per step
    # 1000 sequential float64 additions of sqrt 2 stay within one float32 step of the product
    assert ulps_apart(got[0:1, 63], np.array([1000 * math.sqrt(2.0)], F32)).max() <= 1
    assert_distance(words, None, None, None, "horizontal", "average", (3.0, 0.25))


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    words = dinf.words_from_d8(path_codes(shape, cells))
    want = np.zeros(shape, F32)
    for k, c in enumerate(cells):
        want[c] = len(cells) - 1 - k                        # all steps are cardinal
    assert_distance(words, want=want)
    z = np.random.default_rng(offset).random(shape).astype(F32)
    for kind in ("vertical", "surface"):
        assert_distance(words, None, None, z, kind)


def test_a_cone_where_nearly_every_cell_splits():
    rows, cols = np.mgrid[0:200, 0:200]
    z = (-np.hypot(rows - 99.5, cols - 99.5)).astype(F32)
    words = direction_ref(z)[0]
    assert split_cells(words) > 0.9 * 198 * 198
    for kind in KINDS:
        for statistic in STATISTICS:
            got, _ = assert_distance(words, None, None, None if kind == "horizontal" else z, kind,
                                     statistic)
            assert np.isfinite(got).all()


def test_a_strip_whose_schedule_kernel_spans_two_workgroups():
    shape = sr.DINF_SHAPES[1]
    assert sr.schedule_blocks(shape) >= 2 and sr.tiles_of(shape) > 256
    words = random_acyclic_words(shape, seed=sr.DINF_SEED)
    mask = np.random.default_rng(1).random(shape) < 0.001
    _, stats = assert_distance(words, mask, None, None, "horizontal", "minimum")
    assert stats["rounds"] >= 2
    assert_distance(words, mask)


# ---------------------------------------------------------------------------
# canonical D8 words against the D8 operators
# ---------------------------------------------------------------------------
def test_canonical_words_give_the_d8_hand_and_flow_distance():
    codes, z, streams = d8_case((150, 210), seed=5)
    words = dinf.words_from_d8(codes)
    hand = hd.HeightAboveDrainage(dem=z, streams=streams).apply(codes)
    length = hd.FlowDistance(streams).apply(codes)
    hand.view(np.uint32)[np.isnan(hand)] = 0x7FC00000
    for statistic in STATISTICS:
        op = hd.DInfDistanceDown("vertical", statistic, streams, dem=z)
        assert same_bits(op.apply(words), hand)
        got = hd.DInfDistanceDown("horizontal", statistic, streams).apply(words)
        reached = ~np.isnan(length)
        assert np.array_equal(np.isnan(got), ~reached) and reached.mean() > 0.3
        assert ulps_apart(got[reached], length[reached]).max() <= 1
    assert same_bits(hd.DInfHeightAboveDrainage(dem=z, streams=streams).apply(words), hand)
    # an accumulation with a threshold is the same stop set
    acc = acc_kahn(codes).astype(np.uint32)
    assert same_bits(hd.DInfHeightAboveDrainage(dem=z, streams=acc, threshold=8).apply(words), hand)
    # to the outlet
    out = hd.FlowDistance().apply(codes)
    got = hd.DInfDistanceDown().apply(words)
    assert not np.isnan(got).any() and ulps_apart(got, out).max() <= 1


# ---------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------
def test_two_runs_and_both_forms_give_identical_bytes():
    words = random_acyclic_words((257, 130), seed=21)
    rng = np.random.default_rng(21)
    mask, z = rng.random(words.shape) < 0.1, (rng.random(words.shape) * 50).astype(F32)
    for kind, dem in (("horizontal", None), ("surface", z)):
        a, stats_a = dinf.dinfdist(words, mask, None, dem, 1.0, kind)
        b, _ = dinf.dinfdist(words, mask, None, dem, 1.0, kind)
        with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
                DeviceRaster.from_host(mask.view(np.uint8), dtype=np.uint8) as dm, \
                backend.on_device(dem, dtype=F32) as dz, \
                DeviceRaster.empty(words.shape, F32, dw.ctx) as mine:
            dev, stats_c = dinf.dinfdist_dev(dw, dm, None, dz, 1.0, kind)
            with dev:
                c = dev.to_host()
            same, _ = dinf.dinfdist_dev(dw, dm, None, dz, 1.0, kind, out=mine)
            assert same is mine and mine.to_host().tobytes() == a.tobytes()
            op = hd.DInfDistanceDown(kind, streams=dm, dem=dz)
            with op.apply_device(dw) as one:
                assert one.dtype == F32 and one.to_host().tobytes() == a.tobytes()
            assert op.apply(words).tobytes() == a.tobytes()
        assert a.tobytes() == b.tobytes() == c.tobytes()
        assert schedule_free(stats_a) == schedule_free(stats_c)
        assert same_bits(a, distance_ref(words, mask, dem, kind))


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    words = random_acyclic_words((300, 300), seed=9)
    ctx = backend.context()
    op = hd.DInfDistanceDown()
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
    threshold = 30
    chain = hd.DemToDInfHAND(threshold=threshold, epsilon=epsilon, flats=flats,
                             keep_partial_results=True)
    got = chain.apply(synth_300_500)
    assert chain.filled.dtype == F32 and chain.codes.dtype == np.uint8
    assert np.array_equal(chain.accumulation, acc_kahn(chain.codes))
    want_words, _, _, taken = direction_ref(chain.filled, fallback=chain.codes)
    assert np.array_equal(chain.words, want_words)
    stops = chain.accumulation >= threshold
    want = distance_ref(want_words, stops, chain.filled, "vertical", "average")
    low = distance_ref(want_words, stops, chain.filled, "vertical", "minimum")
    # both branches of the statistic are exercised, by the reference's own account
    cells = want.size
    split = counts_of(want_words, stops, want)["split_cells"]
    print(f"{flats}: finite {np.isfinite(want).mean():.4f}, NaN {np.isnan(want).mean():.4f}, "
          f"split {split / cells:.4f}, finite under minimum {np.isfinite(low).mean():.4f}")
    assert np.isfinite(want).sum() >= 0.5 * cells
    assert np.isnan(want).sum() >= 0.01 * cells
    assert split >= 0.05 * cells
    assert np.isfinite(low).sum() > np.isfinite(want).sum()
    assert same_bits(got, want)
    assert chain.stats["DInfFlowDirection"]["fallback_cells"] == taken
    assert schedule_free(chain.stats["DInfDistanceDown"]) == counts_of(want_words, stops, want)
    assert ("ResolveFlats" in chain.stats) == (flats == "resolve")
    assert set(chain.stats) - {"ResolveFlats"} == {"SinkFill", "FlowAccumulation",
                                                  "DInfFlowDirection", "DInfDistanceDown"}
    # without the stages kept, on the device; and the minimum
    plain = hd.DemToDInfHAND(threshold=threshold, epsilon=epsilon, flats=flats)
    with DeviceRaster.from_host(synth_300_500, dtype=F32) as dz, plain.apply_device(dz) as hand:
        assert hand.dtype == F32 and same_bits(hand.to_host(), want)
    assert plain.filled is None and plain.codes is None and plain.words is None
    assert plain.accumulation is None
    lowest = hd.DemToDInfHAND(threshold=threshold, epsilon=epsilon, flats=flats,
                              statistic="minimum")
    assert same_bits(lowest.apply(synth_300_500), low)


# ---------------------------------------------------------------------------
# refusals: argument errors that the library returns; the context stays usable
# ---------------------------------------------------------------------------
def test_invalid_words_are_refused_with_their_count():
    words = random_acyclic_words((70, 90), seed=2)
    stop = np.zeros((70, 90), bool)
    stop[5:8, 66] = True                                   # a stop cell's word is validated too
    kinds = {"facet > 8": 9 << 16, "q > 32768": (3 << 16) | (Q_ONE + 1), "facet 0 with q": 7,
             "stray bit 20": (2 << 16) | (1 << 20), "stray bit 31": 1 << 31}
    for n, (kind, word) in enumerate(kinds.items(), 1):
        bad = words.copy()
        bad[5:5 + n, 66] = word
        with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells: the facet"):
            hd.DInfDistanceDown(streams=stop).apply(bad)
        with DeviceRaster.from_host(bad, dtype=np.uint32) as dw:
            with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells"):
                hd.DInfDistanceDown().apply_device(dw)
        with pytest.raises(ValueError, match=f"invalid D-infinity word in {n} cells"):
            distance_ref(bad, stop)
        assert kind
    assert_distance(words, stop)


def test_a_receiver_outside_the_raster_is_refused():
    words = np.zeros((66, 70), np.uint32)
    words[0, 3] = dinf.pack(2, 0)                         # north of the first row
    words[65, 69] = dinf.pack(8, 100)                     # east is outside, south-east too
    words[30, 69] = dinf.pack(1, Q_ONE)                   # north-east only, outside
    words[30, 0] = dinf.pack(1, Q_ONE)                    # north-east only, inside
    stop = np.zeros((66, 70), bool)
    stop[0, 3] = True                                     # a stop cell's word is checked too
    with pytest.raises(ValueError, match="send flow outside the raster in 3 cells"):
        hd.DInfDistanceDown(streams=stop).apply(words)
    with pytest.raises(ValueError, match="outside the raster in 3 cells"):
        distance_ref(words, stop)


def test_a_cycle_without_a_stop_is_refused_in_bounded_time_and_one_with_a_stop_is_cut():
    words = np.zeros((40, 130), np.uint32)
    words[7, 7:9] = dinf.pack(np.array([1, 4]), np.array([0, 0]))     # E then W: a 2-cycle
    with pytest.raises(ValueError, match="without a stop cell: 2 cells never resolve"):
        hd.DInfDistanceDown().apply(words)
    cells = loop_cells(10, 59, 11)                        # across the seam at column 64
    assert len(cells) == 40
    words = dinf.words_from_d8(path_codes((40, 130), cells + cells[:1]))
    words[3, 3] = dinf.pack(7, 1000)                      # and a cell that does resolve
    words[9, 58] = dinf.pack(7, 1000)                     # and one that drains into the loop
    with pytest.raises(ValueError, match="41 cells never resolve"):
        hd.DInfDistanceDown().apply(words)
    with pytest.raises(ValueError, match="41 cells never resolve"):
        distance_ref(words, stops_of(words))
    # the same cycle with one stop cell in it
    stop = np.zeros((40, 130), bool)
    stop[cells[17]] = True
    for statistic in STATISTICS:
        got, stats = assert_distance(words, stop, None, None, "horizontal", statistic)
        assert stats["unresolved"] == 0 and got[cells[18]] == 39 and got[cells[16]] == 1
    z = np.random.default_rng(5).random((40, 130)).astype(F32)
    assert_distance(words, stop, None, z, "vertical")


def test_an_output_of_the_wrong_dtype_is_refused_and_the_c_entry_point_checks_its_arguments():
    words = random_acyclic_words((20, 30), seed=4)
    z = random_dem((20, 30), seed=4)
    ctx = backend.context()
    dev = dinf.ON_DEVICE
    acc_kind, mask_kind = backend.FT_STREAMS_ACC_U32, backend.FT_STREAMS_MASK_U8
    with DeviceRaster.from_host(words, dtype=np.uint32) as dw, \
            DeviceRaster.from_host(z, dtype=F32) as dz, \
            DeviceRaster.empty(words.shape, np.uint32, ctx) as wrong, \
            DeviceRaster.empty((20, 31), F32, ctx) as wide, \
            DeviceRaster.empty(words.shape, F32, ctx) as right:
        with pytest.raises(ValueError, match="out is float32, got uint32"):
            dinf.dinfdist_dev(dw, out=wrong)
        with pytest.raises(ValueError, match=r"out is \(20, 31\), the words \(20, 30\)"):
            dinf.dinfdist_dev(dw, out=wide)
        got, _ = dinf.dinfdist_dev(dw, out=right)
        assert got is right and same_bits(right.to_host(), distance_ref(words, stops_of(words)))

        fn = ctx.lib.hdem_dinfdist_u32

        def call(words=dw.ptr, streams=None, kind=0, threshold=0, dem=None, dx=1.0, dy=1.0,
                 what=0, statistic=0, out=right.ptr, flags=dev, stats=None):
            return fn(ctx.handle, words, 20, 30, streams, kind, threshold, dem, dx, dy, what,
                      statistic, out, flags, stats)

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
        refused(b"unknown stream kind 3", kind=3)
        refused(b"must be null and 0", threshold=5)            # a threshold without a raster
        refused(b"takes no threshold", streams=dw.ptr, kind=mask_kind, threshold=5)
        refused(b"needs a threshold", streams=dw.ptr, kind=acc_kind)
        refused(b"stream raster is null", kind=acc_kind, threshold=5)
        for flags in (1, dev | 2, -1):
            refused(b"unknown flags", flags=flags)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(b"dx and dy must be finite and positive", dx=bad)
            refused(b"dx and dy must be finite and positive", dy=bad)
        st = backend._DInfDistStats()                      # pylint: disable=protected-access
        st.struct_size = 0
        refused(b"struct_size", stats=ctypes.byref(st))
        st = backend._DInfDistStats()                      # pylint: disable=protected-access
        st.struct_size = 24                                # a shorter struct
        st.terminal_cells, st.tile_h = -5, -7
        assert call(stats=ctypes.byref(st)) == backend.OK
        assert st.struct_size == 24
        assert st.split_cells == split_cells(words)
        assert st.terminal_cells == -5 and st.tile_h == -7   # nothing beyond it is written
        fake = ctypes.c_void_p(256)                        # never dereferenced
        for flags in (0, dev):
            assert fn(ctx.handle, fake, 65536, 65536, None, 0, 0, None, 1.0, 1.0, 0, 0, fake,
                      flags, None) == backend.BAD_ARG
            assert b"2^32" in ctx.lib.hdem_last_error()
    # the context is as usable as before
    assert_distance(words)


# ---------------------------------------------------------------------------
# poisoned scratch and output memory, and a caller's stream
# ---------------------------------------------------------------------------
def poison_inputs(shape, seed=33):
    words = direction_ref(random_dem(shape, seed=seed, nan=0.01))[0]
    rng = np.random.default_rng(seed)
    (mask, _), (acc, _) = stream_forms(words, seed)
    return {"words": words, "mask": mask.view(np.uint8), "acc": acc,
            "z": (rng.random(shape) * 100).astype(F32)}


def poison_run(call, inp):
    """The horizontal average to a mask, the surface maximum to an accumulation's threshold, and
    the vertical minimum to the outlets."""
    dw, dm, da, dz = (call.up(inp[name]) for name in ("words", "mask", "acc", "z"))
    host, stats = {}, {}
    for name, args in (("horizontal", (dm, None, None, 1.0, "horizontal", "average")),
                       ("surface", (da, 40, dz, (2.0, 3.0), "surface", "maximum")),
                       ("vertical", (None, None, dz, 1.0, "vertical", "minimum"))):
        out = call.out(dw.shape, F32)
        got, st = dinf.dinfdist_dev(dw, *args, out=out)
        assert not call.own or got is out
        host[name] = call.host(got)
        stats.update({f"{name}_{k}": v for k, v in schedule_free(st).items()})
    return host, stats


def poison_check(inp, got):
    words, z = inp["words"], inp["z"]
    assert same_bits(got["horizontal"], distance_ref(words, inp["mask"] != 0))
    assert same_bits(got["surface"], distance_ref(words, inp["acc"] >= 40, z, "surface",
                                                  "maximum", 2.0, 3.0))
    assert same_bits(got["vertical"], distance_ref(words, stops_of(words), z, "vertical",
                                                   "minimum"))


POISON_CASE = Case("dinfdist", ((130, 197),), poison_inputs, poison_run, poison_check, True,
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
        assert_same_bytes(got, clean, f"dinfdist under {byte:#04x}")


@pytest.fixture(scope="module")
def delay():
    return Delay()


def test_a_callers_stream_behind_an_unfinished_producer_changes_no_byte(clean_runs, delay):
    inputs, want, want_stats = clean_runs(False)
    got, stats = on_a_callers_stream(POISON_CASE, inputs, want, False)
    assert_same_bytes(got, want, "dinfdist on an idle stream of the caller's")
    for own in (False, True):
        whose = "the caller's" if own else "the library's"
        what = f"dinfdist behind the delay, out= {whose}"
        got, stats = on_a_callers_stream(POISON_CASE, inputs, want, own, delay)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what
