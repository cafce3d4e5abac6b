"""
The operators merged after tests/test_gpu_size_regimes.py, past one grid stride and one
schedule workgroup, on the MI355X: WeightedFlowAccumulation (``flowsum_forest_degree_kernel``),
UpstreamExtreme and BreachDepressions (``upext_forest_degree_kernel``), FlowPathSum and
FlowPathExtreme (``flowpath_forest_kernel``) and DInfFlowAccumulation
(``dinfacc_schedule_kernel``), on the inputs of tests/size_regimes.py against the suite's own
references and the closed forms that tests/test_size_regimes.py holds to those references.
Every comparison is ``np.array_equal`` or bit for bit; a test asserts the predicate of the
branch it exists for on its own input first.

  strips of 2 181 tiles (at 256 CUs)       100 whole tiles in the second stride of the three
                                           forest kernels; 9 workgroups of the schedule
  65 x 67 200                              the second stride on random codes; its late tiles
                                           are 19 tiles one cell high
  67 200 x 65 (``tall``)                   the same extent upright: 9 full 64 x 64 tiles and 10
                                           one-column tiles past the first stride, with a trunk
                                           that carries 3.2 M cells into them; also run through
                                           FlowAccumulation, the flow trace, Watersheds and
                                           UpstreamFlowLength, which had no full tile there
  1 x 16 485, 3 x 16 485, 1093 x 1029      two workgroups of the schedule kernel; on the last,
                                           tile 256 is (15, 1) of 18 x 17 and its neighbours lie
                                           on both sides of the workgroup boundary

The tall raster is ``random_acyclic_codes`` with the ramp, as ``wide``, plus a trunk down its
west column: without it no cell of a raster 65 cells wide collects more than about 1 900 cells
and hardly a step enters the last tiles from those before them.

Value-only mutants, after the manner of tests/test_gpu_size_regimes.py: each built once and
run once against this file and the operator's earlier GPU file.  Every failure was a failed
assertion or the operator's own "form a cycle" refusal (an in-degree or a tile that is never
served leaves cells unresolved, which the library counts and reports); no HIP call failed.
  flowsum_forest_degree_kernel skipping ``atomicAdd(&indeg_b[n], 1u)`` when
  ``s >= gridDim.x * NT`` (``next[s]`` still written: the walk follows ``next`` alone, every
  entry a valid slot or -1, and is bounded by ``nslots``) -> 11 tests:
      test_strips_carry_weighted_sums_through_the_second_stride, ``one_path``, row and column
      (in ``segments`` no forest node has a successor: a path of 50 cells ends in the tile it
      enters, so there is no in-degree to lose, and both pass);
      test_weighted_accumulation_past_the_cap_matches_the_kahn_reference, all six cases;
      test_unit_weights_past_the_cap_count_cells, wide and tall;
      test_the_mask_of_the_tall_raster_is_the_threshold_of_the_sum;
      nothing else, and all 130 tests of tests/test_gpu_flowsum.py pass
  upext_forest_degree_kernel with the same change (the same bounds; the words it reduces are
  written to the outputs and never used as an index) -> 9 tests:
      test_strips_carry_upstream_extremes_through_the_second_stride, ``one_path``, row and
      column, min and max (``segments`` pass for the reason above);
      test_upstream_extremes_past_the_cap_match_the_kahn_reference, wide and tall, min and max;
      test_the_tall_raster_is_breached_as_the_reference_carves_it;
      nothing else, and all 83 tests of tests/test_gpu_upextreme.py pass
  dinfacc_schedule_kernel starting with ``if (blockIdx.x) return;`` (tiles 256 and up are
  never listed again; the host reads the list's length back as the next grid, so nothing is
  read or written elsewhere) -> all 11 D-infinity tests of this file:
      test_a_strip_of_258_tiles_takes_the_second_schedule_workgroup, all four cases;
      test_random_words_across_the_schedule_workgroup_boundary, all four cases;
      test_the_big_strips_take_nine_schedule_workgroups, row and column;
      test_canonical_words_of_the_tall_raster_give_its_d8_accumulation;
      nothing else, and all 58 tests of tests/test_gpu_dinf.py pass
The path operators are not run under a mutant that skips the stride (it would leave pointers
unwritten, which is not a value-only change); that their answers depend on the late tiles rests
on the conditions tests/test_size_regimes.py asserts on the tall raster.

``forest_rounds`` is held to 2 everywhere but where one round is inherent.  The last rounds
seen at 256 CUs: 5 on the ``one_path`` strips and on tall without streams, 2 on wide without
streams and on both rasters with the stream mask, 1 on the ``segments`` strips and under
``acc >= 10`` (a path ends within a few cells).  test_both_node_arrays_have_held_the_result
asserts that an odd and an even last round occurred.

Measured on the MI355X (``pytest --durations=0``): the 66 tests take 43 s when the file runs
alone, references included; the slowest calls are UpstreamFlowLength on tall (2.5 s), Watersheds
on tall (1.5 s) and the path extremes (1.2 - 1.4 s each, nearly all of it ``extreme_doubling``),
the weighted sums and upstream extremes 0.4 - 1.1 s, every strip and D-infinity case under
0.4 s (tall: 1 052 rounds in 0.38 s).
"""
import functools

import numpy as np
import pytest

import hydrodem_amd as hd
import size_regimes as sr
from hydrodem_amd import dinf, flowsum, upextreme
from hydrodem_amd import flowpath as fp
from test_flowacc import terminal_mask
from test_flowpath import (extreme_doubling, extreme_holds, sum_doubling, sum_holds, value_of)
from test_flowsum import wsum_kahn
from test_flowtrace import distance_of, trace_doubling
from test_gpu_dinf import assert_accumulation, random_acyclic_words
from test_gpu_flowacc import flowacc
from test_gpu_flowpath import path_extreme, path_sum, same
from test_gpu_flowsum import random_weights, sums
from test_gpu_flowtrace import trace
from test_gpu_upextreme import extremes, random_values
from test_gpu_upstream import up
from test_gpu_watersheds import watersheds
from test_dinf import counts_of
from test_upextreme import NOWHERE, same_bytes, upext_kahn
from test_upstream import upstream_kahn
from test_watersheds import labels_doubling, random_seeds

pytestmark = pytest.mark.gpu

U32 = np.uint32
CELL = 12.5
Q_MAX = 2 ** 31 - 1
RASTERS = ("wide", "tall")
STRIPS = [(strip, segment) for strip in ("row", "column") for segment in (None, sr.SEGMENT)]
STRIP_IDS = [f"{strip}-{'segments' if segment else 'one_path'}" for strip, segment in STRIPS]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


@pytest.fixture(scope="module")
def cus():
    """The compute units of the device: what the library reads from ``hipDeviceProp``."""
    import torch
    count = torch.cuda.get_device_properties(0).multi_processor_count
    assert count > 0
    return count


def by_shape(shape):
    return f"{shape[0]}x{shape[1]}"


def codes_of(raster, cus):
    """The codes of ``wide`` or ``tall``, with the predicates they exist for."""
    codes = sr.wide_codes(cus) if raster == "wide" else sr.tall_codes_2d(cus)
    assert sr.past_the_cap(codes.shape, cus) and sr.late_tiles(codes.shape, cus).size > 0
    assert raster == "wide" or sr.full_late_tiles(codes.shape, cus) >= 8
    return codes


def strip_of(strip, cus):
    shape = sr.strip_shapes(cus)[strip]
    assert sr.past_the_cap(shape, cus)
    assert sr.second_stride_tiles(shape, cus) == sr.SECOND_STRIDE
    return shape


# ---------------------------------------------------------------------------
# WeightedFlowAccumulation: flowsum_forest_degree_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("strip, segment", STRIPS, ids=STRIP_IDS)
def test_strips_carry_weighted_sums_through_the_second_stride(cus, strip, segment):
    shape = strip_of(strip, cus)
    codes = sr.strip_codes(shape, segment)
    w = sr.strip_weights(shape, seed=11)
    assert w.ravel()[0] == Q_MAX and w.max() <= Q_MAX
    want = sr.strip_flowsum(shape, w, segment)
    assert segment or want.max() > 2 ** 44              # the carry across 2 181 tiles
    got, stats = sums(codes, w)
    assert np.array_equal(got, want)
    assert stats["nan_weights"] == 0
    if segment:
        rng = np.random.default_rng(12)
        wf, frac_bits = random_weights("f16n", shape, rng)
        q = flowsum.quantise(wf, frac_bits)
        got, stats = sums(codes, wf, frac_bits)
        assert np.array_equal(got, wsum_kahn(codes, q))
        assert np.array_equal(got, sr.strip_flowsum(shape, q, segment))
        assert stats["nan_weights"] == int(np.isnan(wf).sum()) > 0


@functools.lru_cache(maxsize=None)
def weights_of(raster, kind, cus):
    """(weights, frac_bits, the Kahn reference of their sums), made once."""
    codes = codes_of(raster, cus)
    rng = np.random.default_rng(len(raster) * 100 + len(kind))
    w, frac_bits = random_weights(kind, codes.shape, rng)
    return w, frac_bits, wsum_kahn(codes, flowsum.quantise(w, frac_bits))


@pytest.mark.parametrize("kind", ["u32", "u8", "f16n"])
@pytest.mark.parametrize("raster", RASTERS)
def test_weighted_accumulation_past_the_cap_matches_the_kahn_reference(cus, raster, kind):
    codes = codes_of(raster, cus)
    w, frac_bits, want = weights_of(raster, kind, cus)
    got, stats = sums(codes, w, frac_bits)
    assert np.array_equal(got, want)
    assert stats["nan_weights"] == (int(np.isnan(w).sum()) if kind == "f16n" else 0)


@pytest.mark.parametrize("raster", RASTERS)
def test_unit_weights_past_the_cap_count_cells(cus, raster):
    codes = codes_of(raster, cus)
    got, _ = sums(codes, np.ones(codes.shape, np.uint8))
    assert np.array_equal(got, sr.acc_of(raster, cus))


# (``FlowAccumulation`` takes no weights: ``WeightedFlowAccumulation`` and ``flowsum.flowsum`` are
# the only ways into hdem_flowsum_u8, and both are used here)
def test_the_mask_of_the_tall_raster_is_the_threshold_of_the_sum(cus):
    codes = codes_of("tall", cus)
    w, frac_bits, want = weights_of("tall", "u8", cus)
    threshold = 2000
    outs, _ = flowsum.flowsum(codes, w, frac_bits, ("sum", "mask"), threshold)
    assert np.array_equal(outs["sum"], want)
    want_mask = (want >= threshold).astype(np.uint8)
    late = sr.late_mask(codes.shape, cus)
    assert want_mask[late].any() and not want_mask[late].all()
    assert same_bytes(outs["mask"], want_mask)
    f = hd.WeightedFlowAccumulation(w, frac_bits, "mask", threshold)
    assert same_bytes(f.apply(codes), want_mask)


# ---------------------------------------------------------------------------
# UpstreamExtreme and BreachDepressions: upext_forest_degree_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("strip, segment", STRIPS, ids=STRIP_IDS)
def test_strips_carry_upstream_extremes_through_the_second_stride(cus, strip, segment, mode):
    shape = strip_of(strip, cus)
    codes = sr.strip_codes(shape, segment)
    along = -1 if mode == "min" else 1                  # the running extreme keeps changing
    late = sr.late_mask(shape, cus)
    # ... and against the drift it is found near the head and carried through every tile
    cases = [(along, sr.strip_values(shape, along, np.float32, seed=13)),
             (-along, sr.strip_values(shape, -along, np.float32, seed=13))]
    if strip == "row" and segment is None:
        cases.append((along, sr.strip_values(shape, along, U32, seed=14)))
    for trend, v in cases:
        want_extreme, want_where = sr.strip_upextreme(shape, v, mode, segment)
        if trend == along:
            assert np.unique(want_where[late]).size > sr.SECOND_STRIDE // 2
        elif segment is None:
            assert want_where[late].max() < sr.TS * sr.TS
        outs, stats = extremes(codes, v, mode)
        assert same_bytes(outs["extreme"], want_extreme), v.dtype
        assert same_bytes(outs["where"], want_where), v.dtype
        assert stats["absent"] == (int(np.isnan(v).sum()) if v.dtype == np.float32 else 0)


@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("raster", RASTERS)
def test_upstream_extremes_past_the_cap_match_the_kahn_reference(cus, raster, mode):
    codes = codes_of(raster, cus)
    v = random_values("f32n", codes.shape, np.random.default_rng(len(raster)))
    want_extreme, want_where = upext_kahn(codes, v, mode)
    outs, stats = extremes(codes, v, mode)
    assert same_bytes(outs["extreme"], want_extreme)
    assert same_bytes(outs["where"], want_where)
    assert stats["absent"] == int(np.isnan(v).sum()) > 0


def test_the_tall_raster_is_breached_as_the_reference_carves_it(cus):
    codes = codes_of("tall", cus)
    dem = sr.tall_dem_2d(cus)
    want_carved, want_source, pits, lowered = sr.tall_carved(cus)
    late = sr.late_mask(codes.shape, cus)
    low = want_source != NOWHERE
    assert low[late].any() and low[~late].any() and not low[late].all()
    outs, stats = upextreme.breach(dem, codes, ("carved", "source"))
    assert same_bytes(outs["carved"], want_carved)
    assert same_bytes(outs["source"], want_source)
    assert stats["pits"] == pits and stats["lowered"] == lowered


# ---------------------------------------------------------------------------
# FlowPathSum and FlowPathExtreme: flowpath_forest_kernel
# ---------------------------------------------------------------------------
PARITIES = {}


def note_rounds(name, stats, least=2):
    """Both node arrays serve as the result over the file: the parity of the last round.  At
    least two rounds everywhere but in two places where one is inherent: a strip in segments
    of 50 has no forest path of more than two nodes, and under ``acc >= 10`` a path ends at the
    first stream cell, a few cells away."""
    assert stats["forest_rounds"] >= least
    PARITIES[name] = stats["forest_rounds"]
    print(name, "forest_rounds", stats["forest_rounds"], "parity", stats["forest_rounds"] % 2)


@pytest.mark.parametrize("strip, segment", STRIPS, ids=STRIP_IDS)
def test_strips_carry_path_sums_and_extremes_through_the_second_stride(cus, strip, segment):
    shape = strip_of(strip, cus)
    codes = sr.strip_codes(shape, segment)
    stop = sr.strip_answer(shape, segment)["stop"]
    w = sr.strip_weights(shape, seed=15)
    want = sr.strip_pathsum(shape, w, segment)
    assert segment or want.max() > 2 ** 44
    got, stats = path_sum(codes, w)
    assert np.array_equal(got["stop"], stop) and np.array_equal(got["sum"], want)
    assert same(got["value"], value_of(got["stop"], want, 0))
    assert stats["stops"] == sr.strip_answer(shape, segment)["outlets"].size
    note_rounds(f"strip-{strip}-{segment}-sum", stats, 1 if segment else 2)
    late = sr.late_mask(shape, cus)
    for mode in ("min", "max"):
        # with the drift the extreme towards the end changes from tile to tile, the late ones
        # included; against it the holder lies in the last tiles and is carried up to the head
        for trend in (1, -1) if mode == "min" else (-1, 1):
            v = sr.strip_values(shape, trend, np.float32, seed=16)
            want_extreme, want_where = sr.strip_pathextreme(shape, v, mode, segment)
            if trend == (1 if mode == "min" else -1):
                assert np.unique(want_where[late]).size > sr.SECOND_STRIDE // 2
            elif segment is None:
                assert late.ravel()[want_where[~late]].all()
            got, stats = path_extreme(codes, v, mode)
            assert np.array_equal(got["stop"], stop)
            assert same(got["extreme"], want_extreme) and np.array_equal(got["where"], want_where)
            assert stats["absent"] == int(np.isnan(v).sum())
            note_rounds(f"strip-{strip}-{segment}-{mode}{trend:+d}", stats, 1 if segment else 2)


STREAM_FORMS = ("none", "mask", "acc")


def streams_of(form, raster, cus):
    """(streams, threshold, the mask they mean) as the path operators take them."""
    codes = codes_of(raster, cus)
    if form == "none":
        return None, None, None
    if form == "mask":
        mask = random_seeds(codes.shape, seed=codes.shape[0] * 3 + codes.shape[1], every=50) != 0
        return mask.astype(np.uint8) * 255, None, mask
    acc = sr.acc_of(raster, cus).astype(U32)
    return acc, sr.SPARSE_THRESHOLD, acc >= sr.SPARSE_THRESHOLD


@pytest.mark.parametrize("form", STREAM_FORMS)
@pytest.mark.parametrize("raster", RASTERS)
def test_path_sums_per_step_past_the_cap(cus, raster, form):
    codes = codes_of(raster, cus)
    w = np.random.default_rng(17).integers(0, Q_MAX + 1, codes.shape).astype(U32)
    streams, threshold, mask = streams_of(form, raster, cus)
    got, stats = path_sum(codes, w, streams, threshold)
    q = w.astype(np.int64)
    stop, total = sum_doubling(codes, q, mask)
    assert np.array_equal(got["stop"], stop) and np.array_equal(got["sum"], total)
    assert same(got["value"], value_of(stop, total, 0))
    assert sum_holds(codes, q, got["stop"], got["sum"], streams=mask)
    assert stats["unreached"] == int((stop == 0).sum())
    assert (form == "none") == (stats["unreached"] == 0)
    note_rounds(f"{raster}-{form}-sum", stats, 1 if form == "acc" else 2)


@pytest.mark.parametrize("raster", RASTERS)
def test_path_sums_per_unit_length_past_the_cap(cus, raster):
    codes = codes_of(raster, cus)
    table = fp.geographic_step_lengths(codes.shape[0], 60.0, 1.0 / 1200, 1.0 / 1200)
    streams, threshold, mask = streams_of("none", raster, cus)
    q = fp.quantise_steps(codes, None, "length", table, 16)
    assert 0 < q.max() <= Q_MAX
    got, stats = path_sum(codes, None, streams, threshold, "length", table, 16)
    stop, total = sum_doubling(codes, q, mask)
    assert np.array_equal(got["stop"], stop) and np.array_equal(got["sum"], total)
    assert same(got["value"], value_of(stop, total, 16))
    assert sum_holds(codes, q, got["stop"], got["sum"], streams=mask)
    note_rounds(f"{raster}-none-length", stats)


@pytest.mark.parametrize("form", STREAM_FORMS)
@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("raster", RASTERS)
def test_path_extremes_past_the_cap(cus, raster, mode, form):
    codes = codes_of(raster, cus)
    v = random_values("f32n", codes.shape, np.random.default_rng(18))
    streams, threshold, mask = streams_of(form, raster, cus)
    got, stats = path_extreme(codes, v, mode, streams, threshold)
    stop, extreme, where = extreme_doubling(codes, v, mode, mask)
    assert np.array_equal(got["stop"], stop)
    assert same(got["extreme"], extreme) and np.array_equal(got["where"], where)
    assert extreme_holds(codes, v, mode, got["stop"], got["extreme"], got["where"], streams=mask)
    assert stats["absent"] == int(np.isnan(v).sum())
    note_rounds(f"{raster}-{form}-{mode}", stats, 1 if form == "acc" else 2)


def test_both_node_arrays_have_held_the_result(cus):
    """The result of the path operators is read from the node array of the last round: an odd
    and an even last round both occur.  Two calls of its own, so that the test stands alone;
    whatever the tests above have noted is held to the same."""
    shape = strip_of("row", cus)
    _, stats = path_sum(sr.strip_codes(shape), sr.strip_weights(shape, seed=15), want=("sum",))
    note_rounds("strip-row-None-sum", stats)
    codes = codes_of("wide", cus)
    _, stats = path_sum(codes, np.ones(codes.shape, np.uint8), want=("sum",))
    note_rounds("wide-none-unit", stats)
    assert {rounds % 2 for rounds in PARITIES.values()} == {0, 1}, PARITIES


# ---------------------------------------------------------------------------
# DInfFlowAccumulation: dinfacc_schedule_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frac_bits", [0, 16])
@pytest.mark.parametrize("segment", [None, sr.SEGMENT], ids=["one_path", "segments"])
def test_a_strip_of_258_tiles_takes_the_second_schedule_workgroup(segment, frac_bits):
    shape = sr.DINF_SHAPES[0]
    assert sr.schedule_blocks(shape) == 2
    words = sr.strip_words(shape, segment)
    _, stats = assert_accumulation(words, frac_bits, sr.strip_dinf(shape, frac_bits, segment))
    # (one path: about a round per tile, unless a tile sees its neighbour's cells of the same
    # round)
    assert stats["rounds"] >= 2


@pytest.mark.parametrize("shape", sr.DINF_SHAPES[1:], ids=by_shape)
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_random_words_across_the_schedule_workgroup_boundary(shape, frac_bits):
    assert sr.schedule_blocks(shape) >= 2
    words = random_acyclic_words(shape, seed=sr.DINF_SEED)
    assert counts_of(words)["split_cells"] >= 0.05 * words.size
    _, stats = assert_accumulation(words, frac_bits)
    assert stats["rounds"] >= 2


@pytest.mark.parametrize("strip", ["row", "column"])
def test_the_big_strips_take_nine_schedule_workgroups(cus, strip):
    """``segments`` only: one path takes about one host-synchronised round per tile."""
    shape = strip_of(strip, cus)
    assert sr.schedule_blocks(shape) >= 3
    words = sr.strip_words(shape, sr.SEGMENT)
    for frac_bits in (0, 16):
        _, stats = assert_accumulation(words, frac_bits,
                                       sr.strip_dinf(shape, frac_bits, sr.SEGMENT))
        assert stats["rounds"] >= 2


def test_canonical_words_of_the_tall_raster_give_its_d8_accumulation(cus):
    """The trunk is one path through every tile row, so the rounds are about as many."""
    codes = codes_of("tall", cus)
    assert sr.schedule_blocks(codes.shape) >= 3
    codes = np.where(terminal_mask(codes), 0, codes).astype(np.uint8)
    want = sr.acc_of("tall", cus) << 16
    _, stats = assert_accumulation(dinf.words_from_d8(codes), 16, want)
    print("tall D-infinity rounds", stats["rounds"], "visits", stats["tile_visits"])
    assert stats["rounds"] >= 2


# ---------------------------------------------------------------------------
# the four older operators on the tall raster: full tiles in the second stride
# ---------------------------------------------------------------------------
def test_tall_raster_flow_accumulation_matches_the_kahn_reference(cus):
    codes = codes_of("tall", cus)
    acc = flowacc(codes)
    assert acc.dtype == U32 and np.array_equal(acc, sr.acc_of("tall", cus))


def test_tall_raster_flow_trace_matches_the_doubling_reference(cus):
    codes = codes_of("tall", cus)
    got, _ = trace(codes, cellsize=CELL)
    stop, ncard, ndiag = trace_doubling(codes)
    assert np.array_equal(got["stop"], stop)
    assert np.array_equal(got["ncard"], ncard) and np.array_equal(got["ndiag"], ndiag)
    assert np.array_equal(got["distance"], distance_of(stop, ncard, ndiag, CELL))


def test_tall_raster_watersheds_match_the_doubling_reference_and_the_numbering_rule(cus):
    codes = codes_of("tall", cus)
    assert sr.watershed_scan_loops(codes.shape) >= 2
    assert np.array_equal(watersheds(codes), labels_doubling(codes))
    labels, outlets = sr.compact_by_rule(codes)
    basins = hd.Watersheds(labels="compact")
    assert np.array_equal(basins.apply(codes), labels)
    assert np.array_equal(basins.outlets, outlets)
    assert basins.stats["basins"] == outlets.size == int(terminal_mask(codes).sum())
    late = sr.late_mask(codes.shape, cus).ravel()
    assert late[outlets].any() and not late[outlets].all()


def test_tall_raster_upstream_length_matches_the_kahn_reference(cus):
    codes = codes_of("tall", cus)
    ncard, ndiag = upstream_kahn(codes)
    outs = up(codes)
    assert np.array_equal(outs["ncard"], ncard) and np.array_equal(outs["ndiag"], ndiag)
