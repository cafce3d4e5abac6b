"""
Downstream D8 path sums and extremes on the MI355X (``FlowPathSum``, ``FlowPathExtreme``,
``hdem_flowpath_u8[_dev]``).  Every comparison is ``np.array_equal`` (``equal_nan`` or the bits
for the float rasters): closed forms on a row and a column, every field of the scheme filled
(the in-tile sum on a 64 x 64 spiral, the forest sum on a 512^2 snake, both with every cost
2^31 - 1), agreement with the doubling references of tests/test_flowpath.py on random acyclic
codes for every stream kind and weight type, with ``FlowDistance``'s own counts and with
``HeightAboveDrainage`` on a filled DEM, the local proof at 2048^2, poisoned scratch and output
memory, host / device / chain equality and the refusals.

Value-only mutants of the kernels that were run against this file (all but the two synthetic
DEMs: 69 tests), with the tests each fails:
  a crossing step's cost not added to the exit node -> 22 tests, the first
      test_a_row_and_a_column_hold_the_suffix_sums_of_their_positions: every test with a sum
      whose path leaves a tile; the 27 tests of the extremes alone all pass
  the in-tile sum cut to 32 bits -> 15 tests: test_the_in_tile_sum_fills_its_field, both cases,
      test_the_forest_sum_fills_its_field, test_random_acyclic_codes_match_the_sum_reference
      in 11 of its larger cases (its uint32 weights reach 2^31 - 1) and the legal loop of
      test_invalid_bytes_and_cycles_are_refused_with_their_counts; nothing else
  the forest sum cut to 48 bits -> test_the_forest_sum_fills_its_field, and nothing else
  the final pass reading the other of the two node arrays -> 39 tests, the first
      test_a_row_and_a_column_hold_the_suffix_sums_of_their_positions: every test whose paths
      leave a tile, sums and extremes alike
  a stop excluded from the extreme (a cell that points at a stop or an exit keeps its own
      word) -> 32 tests, the first test_random_acyclic_codes_match_the_extreme_reference[f32-3x3];
      among them test_the_stop_at_the_end_of_a_spiral_holds_the_extreme, all four cases, and
      test_a_path_whose_only_value_is_the_stops_and_a_path_without_any; all the sums pass
B done in place (one node array for source and destination) was not run: a torn node can hold
a stop's index where a slot number is expected, which is an out-of-bounds read and not a
value-only mutant.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from hydrodem_amd import flowpath as fp
from hydrodem_amd.backend import DeviceRaster
from test_flowacc import acc_kahn, random_acyclic_codes, terminal_mask
from test_flowpath import (Q_MAX, extreme_doubling, extreme_holds, sum_doubling, sum_holds,
                           value_of)
from test_gpu_flowacc import path_codes, snake, spiral
from test_gpu_scribble import D8_SHAPES, POISON, Case, execute
from test_gpu_scribble import codes_of as scribble_inputs
from test_gpu_watersheds import RANDOM_SHAPES, rim_codes
from test_watersheds import random_seeds

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
SUM_ALL = ("stop", "sum", "value")
EXT_ALL = ("stop", "extreme", "where")
NOWHERE = 0xFFFFFFFF
QUIET_NAN = 0x7FC00000


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(got, want):
    """Dtype, shape and every bit."""
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(bits(got), bits(want))


def path_sum(codes, weights, streams=None, threshold=None, per="step", step_len=None,
             frac_bits=0, want=SUM_ALL):
    """The host entry point in sum mode, all three outputs unless ``want`` says."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    got, stats = fp.flowpath(codes, weights, "sum", streams, threshold, per, step_len,
                             frac_bits, want)
    assert tuple(got) == tuple(n for n in SUM_ALL if n in want)
    dtypes = {"stop": np.uint32, "sum": np.int64, "value": np.float32}
    for name, raster in got.items():
        assert raster.dtype == dtypes[name] and raster.shape == codes.shape, name
    return got, stats


def path_extreme(codes, values, mode, streams=None, threshold=None, want=EXT_ALL):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    got, stats = fp.flowpath(codes, values, mode, streams, threshold, want=want)
    assert tuple(got) == tuple(n for n in EXT_ALL if n in want)
    dtypes = {"stop": np.uint32, "extreme": values.dtype, "where": np.uint32}
    for name, raster in got.items():
        assert raster.dtype == dtypes[name] and raster.shape == codes.shape, name
    return got, stats


def assert_sum(got, codes, q, mask, frac_bits):
    """The three rasters against the doubling reference; unreached cells NaN and stop 0."""
    stop, total = sum_doubling(codes, q, mask)
    assert np.array_equal(got["stop"], stop), "stop"
    assert np.array_equal(got["sum"], total), "sum"
    assert same(got["value"], value_of(stop, total, frac_bits)), "value"
    assert np.array_equal(np.isnan(got["value"]), got["stop"] == 0)
    return stop, total


def assert_extreme(got, codes, values, mode, mask):
    stop, extreme, where = extreme_doubling(codes, values, mode, mask)
    assert np.array_equal(got["stop"], stop), "stop"
    assert same(got["extreme"], extreme), "extreme"
    assert np.array_equal(got["where"], where), "where"
    return stop, extreme, where


def path_cells_answer(shape, cells, along):
    """The sums of ``path_codes(shape, cells)`` when cell k of the path costs ``along[k]``:
    the suffix sums without the last cell's own cost; every other cell is its own stop."""
    total = np.zeros(shape, np.int64)
    ys, xs = np.array(cells).T
    suffix = np.concatenate([np.cumsum(along[:-1][::-1])[::-1], [0]])
    total[ys, xs] = suffix
    return total


# ---------------------------------------------------------------------------
# constructed paths: exact answers, every field full
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_hold_the_suffix_sums_of_their_positions():
    k = np.arange(10000, dtype=np.int64)
    closed = (9998 * 9999 // 2) - (k - 1) * k // 2       # sum of i for k <= i <= 9998
    closed[-1] = 0
    w = k.astype(np.uint32)
    got, stats = path_sum(np.full((1, 10000), E, np.uint8), w.reshape(1, -1))   # 156 crossings
    assert np.array_equal(got["sum"][0], closed)
    assert np.array_equal(got["stop"][0], np.full(10000, 10000))
    assert np.array_equal(got["value"][0], closed.astype(np.float64).astype(np.float32))
    assert stats["stops"] == 1 and stats["unreached"] == 0 and stats["exits"] == 156
    assert stats["tile_h"] == 64 and stats["tile_w"] == 64 and stats["nan_weights"] == 0
    got, _ = path_sum(np.full((10000, 1), S, np.uint8), w.reshape(-1, 1))
    assert np.array_equal(got["sum"][:, 0], closed)
    assert np.array_equal(got["stop"][:, 0], np.full(10000, 10000))


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_the_in_tile_sum_fills_its_field(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    assert len(cells) == 4096                            # 4095 steps of 2^31 - 1: 43 bits
    w = np.full(shape, Q_MAX, np.uint32)
    got, _ = path_sum(path_codes(shape, cells), w)
    want = path_cells_answer(shape, cells, np.full(4096, Q_MAX, np.int64))
    assert np.array_equal(got["sum"], want)
    head = got["sum"][cells[0]]
    assert head == 4095 * Q_MAX and head > 2 ** 42
    assert got["stop"][cells[0]] == cells[-1][0] * shape[1] + cells[-1][1] + 1
    assert np.array_equal(got["value"], want.astype(np.float64).astype(np.float32))


def test_the_forest_sum_fills_its_field():
    cells = snake(512, 512)
    w = np.full((512, 512), Q_MAX, np.uint32)
    got, stats = path_sum(path_codes((512, 512), cells), w)
    want = path_cells_answer((512, 512), cells, np.full(512 * 512, Q_MAX, np.int64))
    assert np.array_equal(got["sum"], want)
    assert got["sum"][0, 0] == 262143 * Q_MAX and got["sum"][0, 0] > 2 ** 48
    assert np.array_equal(got["stop"], np.full((512, 512), 511 * 512 + 1))
    assert stats["stops"] == 1 and stats["exits"] == 512 * 7 + 7
    assert stats["forest_rounds"] >= 2


# ---------------------------------------------------------------------------
# random acyclic codes against the doubling references
# ---------------------------------------------------------------------------
def stream_kinds(codes):
    """(streams, threshold, the mask they mean) for none, a uint8 mask, an accumulation."""
    shape = codes.shape
    mask = (random_seeds(shape, seed=shape[0] * 3 + shape[1], every=50) != 0).astype(np.uint8)
    acc = acc_kahn(codes).astype(np.uint32)
    return ((None, None, None), (mask * 255, None, mask != 0), (acc, 10, acc >= 10))


def weight_kinds(shape, seed):
    """(weights, per, table, frac_bits): uint8, uint32, float32 at 0 and 16 fractional bits
    per step, none with a geographic table per unit length."""
    rng = np.random.default_rng(seed)
    wf = (rng.random(shape, dtype=np.float32) * np.float32(100.0)).astype(np.float32)
    wf[rng.random(shape) < 0.02] = np.nan
    table = fp.geographic_step_lengths(shape[0], 45.0, 1.0 / 1200, 1.0 / 1200)
    return ((rng.integers(0, 256, shape).astype(np.uint8), "step", None, 0),
            (rng.integers(0, Q_MAX + 1, shape).astype(np.uint32), "step", None, 0),
            (wf, "step", None, 0), (wf, "step", None, 16), (None, "length", table, 16))


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_match_the_sum_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    terminal = terminal_mask(codes)
    for weights, per, table, frac_bits in weight_kinds(shape, seed=shape[0] + shape[1]):
        q = fp.quantise_steps(codes, weights, per, table, frac_bits)
        assert 0 <= q.min() and q.max() <= Q_MAX
        nans = int(np.isnan(weights).sum()) if weights is not None and weights.dtype.kind == "f" \
            else 0
        for streams, threshold, mask in stream_kinds(codes):
            got, stats = path_sum(codes, weights, streams, threshold, per, table, frac_bits)
            stop, _ = assert_sum(got, codes, q, mask, frac_bits)
            assert stats["unreached"] == int((stop == 0).sum())
            assert stats["stops"] == int((terminal if mask is None else terminal | mask).sum())
            assert stats["nan_weights"] == nans and stats["absent"] == 0
            if mask is None:
                assert stats["unreached"] == 0 and not np.isnan(got["value"]).any()


def extreme_values(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "u32":
        return rng.integers(0, 6, shape).astype(np.uint32)          # ties everywhere
    pool = np.array([-np.inf, -3.5, -0.0, 0.0, 1.0, 1.5, 1e30, np.inf, np.nan, np.nan],
                    np.float32)
    return pool[rng.integers(0, pool.size, shape)]                  # ties, +-0.0, 20 % NaN


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["f32", "u32"])
def test_random_acyclic_codes_match_the_extreme_reference(shape, kind):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=True)
    values = extreme_values(kind, shape, seed=shape[0] * 11 + shape[1])
    nans = int(np.isnan(values).sum()) if kind == "f32" else 0
    for mode in ("min", "max"):
        for streams, threshold, mask in stream_kinds(codes):
            got, stats = path_extreme(codes, values, mode, streams, threshold)
            stop, _, where = assert_extreme(got, codes, values, mode, mask)
            assert stats["absent"] == nans and stats["nan_weights"] == 0
            assert stats["unreached"] == int((stop == 0).sum())
            present = where != NOWHERE
            assert same(values.ravel()[where[present]], got["extreme"][present])
            if kind == "f32":
                assert np.all(bits(got["extreme"])[~present] == QUIET_NAN)
            else:
                assert present.all()


def test_ties_take_the_smallest_index_also_from_across_a_tile_seam():
    for mode, low, high in (("min", 5.0, 1.0), ("max", 1.0, 9.0)):
        v = np.full(130, low, np.float32)
        v[60] = v[70] = high                              # tiles end at 63
        x = np.arange(130)
        got, _ = path_extreme(np.full((1, 130), E, np.uint8), v.reshape(1, -1), mode)
        assert np.array_equal(got["where"][0], np.where(x <= 60, 60, np.where(x <= 70, 70, x)))
        assert np.array_equal(got["extreme"][0], np.where(x <= 70, high, low).astype(np.float32))
        # upwards: the holder with the smaller index lies in the tile the path reaches last
        got, _ = path_extreme(np.full((130, 1), N, np.uint8), v.reshape(-1, 1), mode)
        assert np.array_equal(got["where"][:, 0], np.where(x >= 60, 60, 0))
        assert np.array_equal(got["extreme"][:, 0], np.where(x >= 60, high, low).astype(np.float32))
        assert np.array_equal(got["stop"], np.full((130, 1), 1))
    zeros = np.zeros((1, 130), np.float32)
    zeros[0, 100] = -0.0                                  # -0.0 below +0.0, across the seam
    got, _ = path_extreme(np.full((1, 130), E, np.uint8), zeros, "min")
    assert np.array_equal(got["where"][0], np.where(np.arange(130) <= 100, 100, np.arange(130)))
    assert np.array_equal(np.signbit(got["extreme"][0]), np.arange(130) <= 100)
    got, _ = path_extreme(np.full((1, 130), E, np.uint8), zeros, "max")
    assert np.array_equal(got["where"][0], np.where(np.arange(130) == 100, 101, np.arange(130)))


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
@pytest.mark.parametrize("mode", ["min", "max"])
def test_the_stop_at_the_end_of_a_spiral_holds_the_extreme(mode, offset):
    """4095 steps inside a tile take all twelve doubling rounds, and the stop's own value has
    to come all the way up to the head through them.  Every cell's extreme is the last
    cell's."""
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    ys, xs = np.array(cells).T
    along = np.arange(4096, dtype=np.uint32)
    v = np.full(shape, 5000, np.uint32)
    v[ys, xs] = 5000 - along if mode == "min" else along
    last = cells[-1][0] * shape[1] + cells[-1][1]
    for values in (v, v.astype(np.float32)):
        got, _ = path_extreme(path_codes(shape, cells), values, mode)
        assert np.all(got["where"][ys, xs] == last) and np.all(got["stop"][ys, xs] == last + 1)
        assert np.all(got["extreme"][ys, xs] == values[cells[-1]])
        assert_extreme(got, path_codes(shape, cells), values, mode, None)
    # and the first cell's, when that is where it is
    v[ys, xs] = along if mode == "min" else 5000 - along
    got, _ = path_extreme(path_codes(shape, cells), v, mode)
    assert np.array_equal(got["where"][ys, xs], ys * shape[1] + xs)


@pytest.mark.parametrize("mode", ["min", "max"])
def test_a_path_whose_only_value_is_the_stops_and_a_path_without_any(mode):
    row = np.full((1, 200), E, np.uint8)
    v = np.full((1, 200), np.nan, np.float32)
    v[0, 199] = 7.0
    got, stats = path_extreme(row, v, mode)
    assert np.all(got["extreme"] == 7.0) and np.all(got["where"] == 199)
    assert np.all(got["stop"] == 200) and stats["absent"] == 199
    mask = np.zeros((1, 200), np.uint8)
    mask[0, 130] = 1
    v[:] = np.nan
    v[0, 130] = -2.0                                      # a stream cell in the third tile
    got, stats = path_extreme(row, v, mode, mask)
    assert np.array_equal(got["stop"][0], [131] * 131 + [0] * 69)
    assert np.array_equal(got["where"][0], [130] * 131 + [NOWHERE] * 69)
    assert np.all(got["extreme"][0, :131] == -2.0)
    assert np.all(bits(got["extreme"])[0, 131:] == QUIET_NAN)
    assert stats["unreached"] == 69
    v[:] = np.nan                                         # nothing present anywhere
    got, stats = path_extreme(row, v, mode)
    assert np.all(bits(got["extreme"]) == QUIET_NAN) and np.all(got["where"] == NOWHERE)
    assert np.all(got["stop"] == 200) and stats["absent"] == 200
    u = np.arange(200, dtype=np.uint32).reshape(1, 200)   # uint32: every value is present
    u[0, 5] = 0xFFFFFFFF
    got, _ = path_extreme(row, u, mode)
    x = np.arange(200)
    if mode == "min":
        assert np.array_equal(got["where"][0], np.where(x == 5, 6, x))
    else:
        assert np.array_equal(got["where"][0], np.where(x <= 5, 5, 199))
        assert np.all(got["extreme"][0, :6] == 0xFFFFFFFF)


# ---------------------------------------------------------------------------
# against the flow trace's own operators
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_the_uniform_table_gives_the_flow_distance_counts_in_integers(frac_bits):
    cs = 30.0
    codes = random_acyclic_codes(300, 517, seed=9, ramp=True)
    acc = acc_kahn(codes).astype(np.uint32)
    card = int(np.rint(cs * 2.0 ** frac_bits))
    diag = int(np.rint((cs * np.sqrt(2.0)) * 2.0 ** frac_bits))
    for streams, threshold in ((None, None), (acc, 25)):
        trace, _ = backend.flowtrace(codes, streams, threshold, None, cs,
                                     ("stop", "ncard", "ndiag"))
        f = hd.FlowPathSum(per="length", cellsize=cs, frac_bits=frac_bits, streams=streams,
                           threshold=threshold, output="sum", keep_partial_results=True)
        total = f.apply(codes)
        assert total.dtype == np.int64 and np.array_equal(f.stop, trace["stop"])
        assert np.array_equal(total, trace["ncard"].astype(np.int64) * card
                              + trace["ndiag"].astype(np.int64) * diag)
        assert trace["ncard"].any() and trace["ndiag"].any()
        table = fp.step_lengths(codes.shape[0], cs)
        g = hd.FlowPathSum(per="length", step_lengths=table, frac_bits=frac_bits,
                           streams=streams, threshold=threshold, output="sum")
        assert np.array_equal(g.apply(codes), total)


def test_the_minimum_along_the_path_of_a_filled_dem_gives_the_height_above_drainage():
    z = hdem_synth.synth_dem(1024, 1024, variant="rough")
    filled = hd.SinkFill(epsilon=0.0).apply(z)
    codes = hd.D8FlowDirection().apply(filled)
    acc = hd.FlowAccumulation().apply(codes)
    # plain D8 stops in the flats of an exact fill, so accumulations stay small: the streams
    # are the hundredth of the cells with the largest ones
    threshold = max(2, int(np.percentile(acc, 99)))
    hand = hd.HeightAboveDrainage(dem=filled, streams=acc, threshold=threshold).apply(codes)
    f = hd.FlowPathExtreme(filled, "min", streams=acc, threshold=threshold,
                           keep_partial_results=True)
    lowest = f.apply(codes)
    reached = f.stop != 0
    print(f"threshold {threshold}, reached {100.0 * reached.mean():.1f} %")
    assert (reached & (acc < threshold)).any() and np.array_equal(reached, ~np.isnan(hand))
    # elevations do not rise along the D8 paths of a filled DEM: the lowest is the stop's
    assert same((filled - lowest)[reached], hand[reached])
    where = hd.FlowPathExtreme(filled, "min", streams=acc, threshold=threshold,
                               output="where").apply(codes)
    assert extreme_holds(codes, filled, "min", f.stop, lowest, where, streams=acc >= threshold)


def test_2048_holds_the_local_proof():
    threshold, frac_bits = 1000, 16
    z = hdem_synth.synth_dem(2048, 2048, variant="rough")
    rng = np.random.default_rng(2048)
    w = (rng.random(z.shape, dtype=np.float32) * np.float32(10.0)).astype(np.float32)
    with DeviceRaster.from_host(z) as dz:
        filled, dcodes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    with filled, dcodes, DeviceRaster.from_host(w, dtype=np.float32) as dw:
        dacc, _ = backend.flowacc_dev(dcodes)
        with dacc:
            outs, stats = fp.flowpath_dev(dcodes, dw, "sum", dacc, threshold, "step", None,
                                          frac_bits, SUM_ALL)
            acc = dacc.to_host()
        got = {}
        for name, raster in outs.items():
            with raster:
                got[name] = raster.to_host()
        codes = dcodes.to_host()
    stream = acc >= threshold
    q = fp.quantise_steps(codes, w, "step", None, frac_bits)
    assert sum_holds(codes, q, got["stop"], got["sum"], streams=stream)
    assert same(got["value"], value_of(got["stop"], got["sum"], frac_bits))
    unreached = int((got["stop"] == 0).sum())
    assert 0 < unreached < codes.size and stats["unreached"] == unreached
    assert stats["exits"] > 0 and stats["forest_rounds"] >= 2
    assert got["sum"].max() > 2 ** 24                     # beyond what float32 sums keep exact


# ---------------------------------------------------------------------------
# poisoned scratch and output memory
# ---------------------------------------------------------------------------
POISON_TABLE_ROW = (10.0, 0.01, 0.01)                     # geographic_step_lengths past the rows


def poison_table(rows):
    return fp.geographic_step_lengths(rows, *POISON_TABLE_ROW)


def poison_run(call, inp):
    """A sum per unit length to the streams and a minimum to the outlet, all outputs."""
    codes = inp["codes"]
    dtypes = {"stop": np.uint32, "sum": np.int64, "value": np.float32, "extreme": np.float32,
              "where": np.uint32}
    dc, dv, da = call.up(codes), call.up(inp["dem"]), call.up(inp["acc"])

    def out(names):
        return {n: call.out(codes.shape, dtypes[n]) for n in names} if call.own else None
    sums, sum_stats = fp.flowpath_dev(dc, dv, "sum", da, 10, "length", poison_table(codes.shape[0]),
                                      8, SUM_ALL, out=out(SUM_ALL))
    lows, low_stats = fp.flowpath_dev(dc, dv, "min", want=EXT_ALL, out=out(EXT_ALL))
    host = {prefix + name: call.host(raster) for prefix, rasters in (("sum_", sums), ("min_", lows))
            for name, raster in rasters.items()}
    stats = {**{"sum_" + k: n for k, n in sum_stats.items() if not k.startswith("ms_")},
             **{"min_" + k: n for k, n in low_stats.items() if not k.startswith("ms_")}}
    return host, stats


def poison_check(inp, got):
    codes = inp["codes"]
    q = fp.quantise_steps(codes, inp["dem"], "length", poison_table(codes.shape[0]), 8)
    stop, total = sum_doubling(codes, q, inp["acc"] >= 10)
    assert np.array_equal(got["sum_stop"], stop) and np.array_equal(got["sum_sum"], total)
    assert same(got["sum_value"], value_of(stop, total, 8))
    stop, extreme, where = extreme_doubling(codes, inp["dem"], "min")
    assert np.array_equal(got["min_stop"], stop) and same(got["min_extreme"], extreme)
    assert np.array_equal(got["min_where"], where)


# (no schedule set: forest_rounds too is compared, nothing jumps in place)
POISON_CASE = Case("flowpath-sum-and-min", tuple(D8_SHAPES), scribble_inputs, poison_run,
                   poison_check, True, frozenset())


@pytest.mark.parametrize("own", [False, True], ids=["library_out", "callers_out"])
@pytest.mark.parametrize("shape", D8_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_poisoned_memory_changes_no_byte(shape, own):
    inp = POISON_CASE.build(shape, 5)
    clean, clean_stats = execute(POISON_CASE, inp, None, own)
    POISON_CASE.check(inp, clean)
    for byte in POISON:                                   # 0x00 first
        got, stats = execute(POISON_CASE, inp, byte, own)
        assert got.keys() == clean.keys()
        for name in clean:
            assert same(got[name], clean[name]), (name, hex(byte))
        assert stats == clean_stats, hex(byte)            # forest_rounds too: nothing in place


# ---------------------------------------------------------------------------
# host and device forms, the operators, a chain
# ---------------------------------------------------------------------------
def test_host_and_device_forms_and_a_repeat_are_bit_equal():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    acc = acc_kahn(codes).astype(np.uint32)
    rng = np.random.default_rng(8)
    w = (rng.random(codes.shape, dtype=np.float32) * np.float32(50.0)).astype(np.float32)
    w[rng.random(codes.shape) < 0.02] = np.nan
    table = fp.geographic_step_lengths(700, 60.0, 0.001, 0.001)
    q = fp.quantise_steps(codes, w, "length", table, 12)
    a, sa = path_sum(codes, w, acc, 10, "length", table, 12)
    b, sb = path_sum(codes, w, acc, 10, "length", table, 12)
    assert_sum(a, codes, q, acc >= 10, 12)
    la, lsa = path_extreme(codes, w, "max", acc, 10)
    assert_extreme(la, codes, w, "max", acc >= 10)
    with DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            DeviceRaster.from_host(acc, dtype=np.uint32) as dacc, \
            DeviceRaster.from_host(w, dtype=np.float32) as dw:
        outs, sc = fp.flowpath_dev(dc, dw, "sum", dacc, 10, "length", table, 12, SUM_ALL)
        c = {}
        for name, raster in outs.items():
            with raster:
                c[name] = raster.to_host()
        outs, lsc = fp.flowpath_dev(dc, dw, "max", dacc, 10, want=EXT_ALL)
        lc = {}
        for name, raster in outs.items():
            with raster:
                lc[name] = raster.to_host()
        for name in SUM_ALL:
            assert same(a[name], b[name]) and same(a[name], c[name]), name
        for name in EXT_ALL:
            assert same(la[name], lc[name]), name
        assert sa == sb == sc and lsa == lsc              # (no phase times: profiling is off)
        assert sa["nan_weights"] == int(np.isnan(w).sum()) == lsa["absent"]
        # the operators, operands on either side, apply_device against apply
        for weights, streams in ((w, acc), (dw, dacc), (w, dacc)):
            f = hd.FlowPathSum(weights, per="length", step_lengths=table, frac_bits=12,
                               streams=streams, threshold=10, keep_partial_results=True)
            assert same(f.apply(codes), a["value"]) and same(f.stop, a["stop"])
            with f.apply_device(dc) as dev:
                assert same(dev.to_host(), a["value"])
            with f.stop as ds:
                assert same(ds.to_host(), a["stop"])
            assert f.stats["unreached"] == sa["unreached"]
            for output in ("extreme", "where"):
                g = hd.FlowPathExtreme(weights, "max", streams=streams, threshold=10,
                                       output=output)
                assert same(g.apply(codes), la[output]) and g.stop is None
                with g.apply_device(dc) as dev:
                    assert dev.dtype == g.dtype and same(dev.to_host(), la[output])
        f = hd.FlowPathSum(w, frac_bits=12, output="sum")
        with f.apply_device(dc) as dev:
            assert dev.dtype == np.int64
            assert np.array_equal(dev.to_host(),
                                  sum_doubling(codes, fp.quantise_steps(codes, w, "step", None, 12))[1])
    # either output alone holds the bytes of the call for all
    for name in SUM_ALL:
        alone, st = path_sum(codes, w, acc, 10, "length", table, 12, want=(name,))
        assert same(alone[name], a[name]) and st == sa
    for name in EXT_ALL:
        alone, st = path_extreme(codes, w, "max", acc, 10, want=(name,))
        assert same(alone[name], la[name]) and st == lsa


def test_a_chain_from_the_dem_is_device_resident_and_equals_the_host_chain(monkeypatch):
    z = hdem_synth.synth_dem(257, 300, variant="rough")
    w = np.random.default_rng(3).random(z.shape, dtype=np.float32)
    members = [hd.SinkFill(epsilon=1e-3), hd.D8FlowDirection(),
               hd.FlowPathSum(w, frac_bits=16, keep_partial_results=True)]
    codes = members[1].apply(members[0].apply(z))
    host = members[2].apply(codes)
    stop = members[2].stop
    assert same(host, value_of(*sum_doubling(codes, fp.quantise_steps(codes, w, "step", None, 16)),
                               16))
    chain = hd.ComposedFilter()
    chain.filters = members
    with DeviceRaster.from_host(z) as dz, chain.apply_device(dz) as dev:
        assert dev.dtype == np.float32 and same(dev.to_host(), host)
    with members[2].stop as ds:
        assert same(ds.to_host(), stop)

    def host_form(*a, **k):
        raise AssertionError("a member ran on the host")
    for cls in (hd.SinkFill, hd.D8FlowDirection, hd.FlowPathSum):
        assert cls.auto_device is True
        monkeypatch.setattr(cls, "apply", host_form)
    assert same(chain.apply(z), host)                     # through apply_device, member by member
    members[2].stop.free()


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    codes = random_acyclic_codes(300, 300, seed=5, ramp=True)
    w = np.ones(codes.shape, np.uint8)
    ctx = backend.context()
    f = hd.FlowPathSum(w, frac_bits=0)
    f.apply(codes)
    assert f.stats["ms_tile"] == 0 and f.stats["ms_forest"] == 0 and f.stats["ms_final"] == 0
    ctx.profile(True)
    try:
        f.apply(codes)
    finally:
        ctx.profile(False)
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0
    assert "struct_size" not in f.stats and "reserved" not in f.stats


# ---------------------------------------------------------------------------
# refusals: each with its count, the context usable afterwards
# ---------------------------------------------------------------------------
def good_call():
    got, _ = path_sum(np.full((3, 5), S, np.uint8), np.full((3, 5), 2, np.uint8))
    assert np.array_equal(got["sum"][:, 0], [4, 2, 0])
    assert np.array_equal(got["stop"][:, 0], [11, 11, 11])


def test_weights_out_of_range_are_refused_with_their_counts():
    codes = np.full((70, 130), E, np.uint8)
    w = np.ones((70, 130), np.float32)
    w[3, 4] = w[69, 129] = -1.0                           # the second one on a stop
    w[5, 6] = -np.inf
    with pytest.raises(ValueError, match="out of range in 3 cells: 3 negative, 0 infinite, 0 above"):
        path_sum(codes, w, frac_bits=16)
    good_call()
    w[:] = 1.0
    w[60, 100] = np.inf
    w[0, 0] = np.nan                                      # a NaN costs 0 and is no refusal
    with pytest.raises(ValueError, match="1 cells: 0 negative, 1 infinite, 0 above"):
        path_sum(codes, w, frac_bits=16)
    good_call()
    w[60, 100] = 32768.0                                  # 2^31 at 16 fractional bits
    w[60, 101] = 32767.99                                 # just below
    with pytest.raises(ValueError, match=r"1 cells: 0 negative, 0 infinite, 1 above.*frac_bits 16"):
        path_sum(codes, w, frac_bits=16)
    got, stats = path_sum(codes, w, frac_bits=15)
    assert stats["nan_weights"] == 1
    assert got["sum"][60, 100] - got["sum"][60, 101] == 2 ** 30
    u = np.full((70, 130), 7, np.uint32)
    u[1, 1] = 2 ** 31
    u[2, 2] = 2 ** 32 - 1
    with pytest.raises(ValueError, match="2 cells: 0 negative, 0 infinite, 2 above"):
        path_sum(codes, u)
    # per unit length it is the product that counts
    table = fp.step_lengths(70, 1000.0)
    u[1, 1] = u[2, 2] = 7
    u[9, 9] = 2 ** 31 // 1000 + 1
    with pytest.raises(ValueError, match="1 cells: 0 negative, 0 infinite, 1 above"):
        path_sum(codes, u, per="length", step_len=table)
    good_call()


def test_invalid_bytes_and_cycles_are_refused_with_their_counts():
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = 3
    codes[21, 34] = 255
    w = np.ones((50, 70), np.float32)
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        path_sum(codes, w)
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        path_extreme(codes, w, "min", np.ones((50, 70), np.uint8))
    with pytest.raises(ValueError, match="invalid D8 code in 2 cells"):
        path_sum(codes, None, per="length", step_len=fp.step_lengths(50))
    good_call()
    pair = np.array([[E, W_]], np.uint8)
    with pytest.raises(ValueError, match="cycle: 2 cells never resolve"):
        path_sum(pair, np.ones((1, 2), np.uint8))
    with pytest.raises(ValueError, match="cycle: 2 cells never resolve"):
        path_extreme(pair, np.ones((1, 2), np.uint32), "max")
    good_call()
    codes = rim_codes()
    codes[100, 21:100] = W_                               # 79 cells that drain into the loop
    w = np.full(codes.shape, Q_MAX, np.uint32)            # sums that wrap while they double
    with pytest.raises(ValueError, match="cycle: 875 cells never resolve"):
        path_sum(codes, w)
    with pytest.raises(ValueError, match="cycle: 875 cells never resolve"):
        path_extreme(codes, w, "min")
    good_call()
    # a loop that holds a stream cell ends there: legal, and the reference agrees
    mask = np.zeros((256, 256), np.uint8)
    mask[10, 150] = 1
    got, stats = path_sum(codes, w, mask)
    assert_sum(got, codes, w.astype(np.int64), mask, 0)
    assert (got["stop"] != 0).sum() == 875 and got["sum"].max() == 795 * Q_MAX
    got, _ = path_extreme(codes, w, "max", mask)
    assert_extreme(got, codes, w, "max", mask)


def _call(fn, ctx, d8, h, w, streams=None, kind=0, threshold=0, mode=0, values=None,
          value_type=0, per=0, frac_bits=0, step_len=None, outs=(None,) * 5, flags=0, st=None):
    return fn(ctx.handle, d8, h, w, streams, kind, threshold, mode, values, value_type, per,
              frac_bits, step_len, *outs, flags, st)


def test_a_bad_table_entry_is_refused_before_any_launch():
    codes = np.full((6, 9), E, np.uint8)
    for bad in (0.0, -1.0, np.nan, np.inf):
        table = fp.step_lengths(6, 30.0)
        table[4, 2] = table[5, 0] = bad
        with pytest.raises(ValueError, match="2 entries that are not finite and positive"):
            path_sum(codes, None, per="length", step_len=table)
        ctx = backend.context()                           # the C entry points say the same
        with DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
                DeviceRaster.empty((6, 9), np.int64, ctx) as ds:
            host_sum = np.empty((6, 9), np.int64)
            for fn, d8, out in ((ctx.lib.hdem_flowpath_u8_dev, dc.ptr, ds.ptr),
                                (ctx.lib.hdem_flowpath_u8, codes.ctypes.data,
                                 host_sum.ctypes.data)):
                rc = _call(fn, ctx, d8, 6, 9, per=1, step_len=table.ctypes.data,
                           outs=(None, out, None, None, None))
                assert rc == backend.BAD_ARG
                text = ctx.lib.hdem_last_error()
                assert b"step_len has 2 entries" in text and b"row 4" in text, text
    good_call()


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_flowpath_u8_dev, ctx.lib.hdem_flowpath_u8):
        st = backend._FlowPathStats()
        rc = _call(fn, ctx, fake, 65536, 65536, values=fake, value_type=1,
                   outs=(fake, None, None, None, None), st=ctypes.byref(st))
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    good_call()


def test_the_c_entry_points_check_their_arguments_and_struct_size():
    ctx = backend.context()
    table = fp.step_lengths(4, 2.0)
    with DeviceRaster.from_host(np.full((4, 4), E, np.uint8), dtype=np.uint8) as dc, \
            DeviceRaster.from_host(np.ones((4, 4), np.uint32), dtype=np.uint32) as dv, \
            DeviceRaster.from_host(np.ones((4, 4), np.uint32), dtype=np.uint32) as ds, \
            DeviceRaster.empty((4, 4), np.uint32, ctx) as do, \
            DeviceRaster.empty((4, 4), np.uint32, ctx) as dw, \
            DeviceRaster.empty((4, 4), np.int64, ctx) as dsum:
        fn = ctx.lib.hdem_flowpath_u8_dev
        tp = table.ctypes.data
        sum_outs = (do.ptr, dsum.ptr, None, None, None)
        ext_outs = (do.ptr, None, None, dw.ptr, None)

        def call(**kw):
            kw.setdefault("values", dv.ptr)
            kw.setdefault("value_type", 2)
            kw.setdefault("outs", sum_outs if kw.get("mode", 0) == 0 else ext_outs)
            return _call(fn, ctx, dc.ptr, 4, 4, **kw)
        cases = [
            (dict(mode=3), b"unknown mode"),
            (dict(mode=-1), b"unknown mode"),
            (dict(value_type=4), b"unknown value type"),
            (dict(per=2), b"unknown per"),
            (dict(flags=1), b"flags"),
            (dict(kind=3), b"unknown stream kind"),
            (dict(streams=ds.ptr, kind=2, threshold=0), b"threshold >= 1"),
            (dict(streams=ds.ptr, kind=1, threshold=3), b"no threshold"),
            (dict(streams=None, kind=2, threshold=3), b"null"),
            (dict(frac_bits=-1, value_type=1), b"frac_bits is 0 ... 30"),
            (dict(frac_bits=31, value_type=1), b"frac_bits is 0 ... 30"),
            (dict(frac_bits=4), b"integer weights per step take frac_bits 0"),
            (dict(values=None), b"do not go together"),
            (dict(value_type=0), b"do not go together"),
            (dict(values=None, value_type=0), b"needs the weights"),
            (dict(step_len=tp), b"null per step"),
            (dict(per=1), b"needs step_len"),
            (dict(outs=(None,) * 5), b"no output wanted"),
            (dict(outs=ext_outs), b"outputs of the min and max modes"),
            (dict(mode=1, outs=sum_outs), b"outputs of a sum"),
            (dict(mode=1, outs=(None,) * 5), b"no output wanted"),
            (dict(mode=2, value_type=3), b"float32 or uint32"),
            (dict(mode=1, values=None, value_type=0), b"float32 or uint32"),
            (dict(mode=1, per=1), b"belong to a sum"),
            (dict(mode=1, frac_bits=1), b"belong to a sum"),
            (dict(mode=2, step_len=tp), b"belong to a sum"),
            # an output over an input or over another output
            (dict(outs=(dv.ptr, None, None, None, None)), b"stop overlaps weights"),
            (dict(outs=(do.ptr, do.ptr, None, None, None)), b"sum overlaps stop"),
            (dict(outs=(None, dsum.ptr, dsum.ptr + 64, None, None)), b"value overlaps sum"),
            (dict(mode=1, outs=(None, None, None, dv.ptr, None)), b"extreme overlaps values"),
            (dict(mode=2, outs=(do.ptr, None, None, dw.ptr, do.ptr)), b"where overlaps stop"),
            (dict(mode=2, outs=(None, None, None, dw.ptr, dw.ptr)), b"where overlaps extreme"),
            (dict(streams=ds.ptr, kind=1, outs=(None, ds.ptr, None, None, None)),
             b"sum overlaps streams"),
            (dict(outs=(dc.ptr, None, None, None, None)), b"stop overlaps d8"),
        ]
        for kwargs, text in cases:
            assert call(**kwargs) == backend.BAD_ARG, kwargs
            assert text in ctx.lib.hdem_last_error(), (kwargs, ctx.lib.hdem_last_error())
        st = backend._FlowPathStats()
        st.struct_size = 0
        assert call(st=ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend._FlowPathStats()
        st.struct_size = 16                              # a shorter struct
        st.unreached, st.exits, st.tile_h = -3, -5, -7
        assert call(st=ctypes.byref(st)) == backend.OK
        assert st.struct_size == 16 and st.stops == 4 and st.forest_rounds == 1
        assert st.unreached == -3 and st.exits == -5 and st.tile_h == -7   # nothing beyond it
        assert np.array_equal(do.to_host(), np.repeat([[4], [8], [12], [16]], 4, axis=1))
        assert np.array_equal(dsum.to_host(), np.repeat([[3, 2, 1, 0]], 4, axis=0))
        # integer weights per unit length with fractional bits; the table is a host pointer
        assert call(per=1, frac_bits=3, step_len=tp) == backend.OK
        assert np.array_equal(dsum.to_host(), 16 * np.repeat([[3, 2, 1, 0]], 4, axis=0))
        assert call(mode=2) == backend.OK
        assert np.array_equal(dw.to_host(), np.ones((4, 4)))
    good_call()
