"""
tests/size_regimes.py without a device: every input that tests/test_gpu_size_regimes.py and
tests/test_gpu_size_regimes_newer.py run satisfies the predicate it exists for, at 64, 256 and
304 compute units; every closed form agrees with the suite's existing reference of the same
operator on a small copy of the same construction (a strip of 700 cells, a column of 9 000
rows); the zonal inputs put ids into every scan chunk, so that no chunk offset can be wrong
unseen; and the tall raster sends flow, carved cells and streams through the tiles past the
first grid stride, so that the path operators, which no stride-skipping mutant may be run
against, cannot be right there by accident.
"""
import numpy as np
import pytest

import size_regimes as sr
from test_depressions import reference as depressions_reference
from test_dinf import accumulate_ref, counts_of
from test_flowacc import acc_kahn, terminal_mask
from test_flowpath import extreme_doubling, sum_doubling
from test_flowsum import wsum_kahn
from test_flowtrace import trace_doubling
from test_gpu_dinf import random_acyclic_words
from test_streamnet import COUNTERS, same_table, table_np
from test_streamorder import link_ends, order_kahn, stream_of
from test_upextreme import same_bytes, upext_kahn
from test_upstream import upstream_kahn
from test_watersheds import labels_doubling


def by_shape(shape):
    return f"{shape[0]}x{shape[1]}"


# ---------------------------------------------------------------------------
# the predicates themselves, on figures worked out by hand
# ---------------------------------------------------------------------------
def test_the_predicates_on_the_thresholds_themselves():
    assert (sr.TS, sr.PER, sr.SCAN_CHUNK, sr.ONE_NT) == (64, 4 * 64 - 4, 256 * 16, 1024)
    assert [sr.scan_chunks(w) for w in (1, 4096, 4097, 8192, 8193)] == [1, 1, 2, 2, 3]
    assert sr.zonal_words((512, 512)) == 4096 and sr.zonal_words((5, 52429)) == 4097
    assert sr.tile_words((4097, 1)) == 4097 and sr.tile_words((1400, 130)) == 1400 * 3
    assert sr.tile_words((512, 512)) == 4096 and sr.tile_words((2048, 2048)) == 16 * 4096
    # 16384^2 sits exactly at the limit of the one workgroup, the tall column just past it
    assert sr.one_kernel_loops(sr.tile_words((16384, 16384))) == 1
    assert sr.one_kernel_loops(4 * 1024 * 1024 + 1) == 2
    assert sr.tiles_of((1, 140000)) == 2188 and sr.tiles_of((65, 67200)) == 2 * 1050
    assert sr.watershed_scan_loops((2048, 2048)) == 1 and sr.watershed_scan_loops((1, 65537)) == 2
    # 256 CUs: 2 048 workgroups of 256 slots = 524 288 slots = 2 080.5 tiles
    assert not sr.past_the_cap((1, 2080 * 64), 256) and sr.past_the_cap((1, 2080 * 64 + 1), 256)
    assert not sr.past_the_cap((2048, 2048), 256) and sr.past_the_cap((4096, 4096), 256)
    assert sr.second_stride_tiles((1, 2081 * 64), 256) == 0
    assert sr.second_stride_tiles((1, 2082 * 64), 256) == 1
    assert sr.dense_ends(8400, 4200) and not sr.dense_ends(8399, 4200)


# ---------------------------------------------------------------------------
# 1. zonal statistics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(sr.ZONAL_SHAPES), ids=by_shape)
def test_zonal_inputs_fill_every_scan_chunk(shape):
    words, chunks = sr.ZONAL_SHAPES[shape]
    assert (sr.zonal_words(shape), sr.scan_chunks(words)) == (words, chunks)
    n = shape[0] * shape[1]
    for kind in sr.ZONE_KINDS:
        zones = sr.zones_of(kind, shape)
        assert zones.dtype == np.uint32 and zones.shape == shape, kind
        assert int(zones.max()) == n, kind
        filled = sr.ids_per_chunk(zones)
        assert filled.size == chunks and filled[0] > 0 and filled[-1] > 0, kind
        if kind in sr.FILLING_KINDS or kind == "edges":
            assert (filled > 0).all(), kind             # no offset is multiplied by nothing
    edges = np.unique(sr.zones_of("edges", shape)).tolist()
    assert edges == [i for i in sr.CHUNK_EDGE_IDS if i <= n] + ([n] if n not in
                                                                sr.CHUNK_EDGE_IDS else [])
    # the last id is the last bit of the last word in use
    assert sr.zones_of("own", shape).max() == n and (n - 1) // 64 == words - 1


def test_three_chunks_hold_ids_so_that_two_wrong_offsets_cannot_cancel():
    shape = (771, 700)
    assert sr.ZONAL_SHAPES[shape][1] == 3
    for kind in sr.FILLING_KINDS + ("edges",):
        filled = sr.ids_per_chunk(sr.zones_of(kind, shape))
        assert filled.size == 3 and (filled > 0).all(), kind
    assert sr.ids_per_chunk(sr.zones_of("edges", shape)).tolist() == [2, 2, 2]


# ---------------------------------------------------------------------------
# 2. stream order and stream network
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(sr.STREAM_SHAPES), ids=by_shape)
def test_stream_inputs_reach_their_chunks_and_both_end_kernels(shape):
    words, chunks = sr.STREAM_SHAPES[shape]
    assert (sr.tile_words(shape), sr.scan_chunks(words)) == (words, chunks)
    for ramp in (False, True):
        codes, acc = sr.stream_case(shape, ramp)
        for kind in sr.STREAM_KINDS + ("sparse",):
            stream = stream_of(codes, *sr.stream_form(kind, shape, acc))
            ends = np.flatnonzero(link_ends(codes, stream).ravel() == np.arange(codes.size) + 1)
            assert ends.size == sr.link_count(codes, stream)
            if shape[1] == 1:           # at most a link per word
                assert not sr.dense_ends(ends.size, words)
                # every cell a stream cell: the last one ends a link in the last chunk
                assert kind != "all" or ends[-1] // sr.SCAN_CHUNK == chunks - 1
                continue
            assert sr.dense_ends(ends.size, words) == (kind != "sparse"), (kind, ends.size)
            # ends in every chunk
            word = ends // shape[1] * (words // shape[0]) + ends % shape[1] // sr.TS
            assert (np.bincount(word // sr.SCAN_CHUNK, minlength=chunks) > 0).all(), kind


def test_the_tall_column_is_past_the_one_workgroup_and_has_links_in_every_chunk():
    rows = sr.TALL[0]
    words = sr.tile_words(sr.TALL)
    assert words == rows and sr.scan_chunks(words) == 1025 > sr.ONE_NT
    assert sr.one_kernel_loops(words) == 2
    tops, ends = sr.tall_runs(rows)
    assert (tops[1:] > ends[:-1] + 1).all() and tops[0] >= 1 and ends[-1] == rows - 2
    assert (np.bincount(ends // sr.SCAN_CHUNK, minlength=1025) > 0).all()
    assert not sr.dense_ends(ends.size, words) and 2000 < ends.size < 10000
    # no run lines up with the tiles
    assert (tops % sr.TS != 0).any() and ((ends + 1) % sr.TS != 0).any()
    dem, filled = sr.tall_dem(rows)
    assert (sr.roots_per_chunk(dem, filled) > 0).all()


def test_the_tall_closed_form_is_the_numpy_grouping_of_a_column_of_9000():
    rows = 9000
    runs = sr.tall_runs(rows)
    codes, mask = sr.tall_codes(rows), sr.tall_mask(rows, runs)
    dem = np.random.default_rng(1).normal(100.0, 30.0, (rows, 1)).astype(np.float32)
    table, row, counters, rasters = sr.tall_answer(rows, runs, dem, 12.5)
    want, want_row, want_counters = table_np(codes, mask, dem, 12.5)
    assert same_table(table, want) and row.dtype == np.uint32 and np.array_equal(row, want_row)
    assert counters == want_counters and set(counters) == set(COUNTERS)
    assert sr.scan_chunks(sr.tile_words((rows, 1))) == 3 and runs[0].size > 5
    order, magnitude = order_kahn(codes, mask)
    assert np.array_equal(rasters["order"], order)
    assert np.array_equal(rasters["magnitude"], magnitude)
    assert np.array_equal(rasters["link"], link_ends(codes, mask))
    # the depressions of the column: as many as runs of raised cells, some in every chunk
    dem, filled = sr.tall_dem(rows)
    _, count, table = depressions_reference(dem, filled)
    per_chunk = sr.roots_per_chunk(dem, filled)
    assert per_chunk.sum() == count and (per_chunk > 0).all()
    assert np.array_equal(np.bincount(table["first"] // sr.SCAN_CHUNK), per_chunk)


# ---------------------------------------------------------------------------
# 4. strips past the grid cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cus", sr.CUS)
def test_strips_are_past_the_cap_at_any_compute_unit_count(cus):
    n = sr.strip_length(cus)
    assert n % sr.TS == sr.PARTIAL and n % sr.SEGMENT != 0
    for shape in list(sr.strip_shapes(cus).values()) + [sr.wide_shape(cus)]:
        assert sr.past_the_cap(shape, cus), shape
    for shape in sr.strip_shapes(cus).values():
        assert shape in ((1, n), (n, 1))
        assert sr.second_stride_tiles(shape, cus) == sr.SECOND_STRIDE
        # one tile less is not enough: the smallest such strip
        assert sr.second_stride_tiles((1, n - sr.TS), cus) == sr.SECOND_STRIDE - 1
        # whole tiles with exits of their own lie in the second stride
        assert sr.tiles_of(shape) * sr.PER > sr.CAP_PER_CU * cus * sr.FOREST_NT + 50 * sr.PER
    wide = sr.wide_shape(cus)
    assert wide[0] == 65 and wide[1] % (50 * sr.TS) == 0
    assert not sr.past_the_cap((65, wide[1] - 50 * sr.TS), cus)
    assert sr.second_stride_tiles(wide, cus) > 0
    if cus == 256:
        assert n == 139557 and wide == (65, 67200)
        # the segments put basins into more tiles than the watershed scan has threads
        assert sr.watershed_scan_loops((1, n)) == 3 and sr.watershed_scan_loops(wide) == 3
    if cus >= 256:
        assert sr.watershed_scan_loops((1, n)) >= 2 and sr.watershed_scan_loops(wide) >= 2
        assert sr.strip_answer((1, n), sr.SEGMENT)["outlets"].size == -(-n // sr.SEGMENT) > 2048


@pytest.mark.parametrize("shape", [(1, 700), (700, 1)], ids=by_shape)
@pytest.mark.parametrize("segment", [None, sr.SEGMENT], ids=["one_path", "segments"])
def test_strip_closed_forms_are_the_references_on_700_cells(shape, segment):
    codes = sr.strip_codes(shape, segment)
    want = sr.strip_answer(shape, segment)
    assert np.array_equal(want["acc"], acc_kahn(codes))
    stop, ncard, ndiag = trace_doubling(codes)
    assert np.array_equal(want["stop"], stop) and np.array_equal(want["to_end"], ncard)
    assert not ndiag.any()
    assert np.array_equal(want["stop"], labels_doubling(codes))
    up_card, up_diag = upstream_kahn(codes)
    assert np.array_equal(want["up"], up_card) and not up_diag.any()
    labels, outlets = sr.compact_by_rule(codes)
    assert np.array_equal(want["compact"], labels) and np.array_equal(want["outlets"], outlets)
    assert outlets.size == int(terminal_mask(codes).sum()) == (14 if segment else 1)
    # segments do not line up with tiles
    assert segment is None or sr.TS % segment != 0


# ---------------------------------------------------------------------------
# 5. - 7. the newer operators: flowsum, upstream extremes, path sums, D-infinity
# ---------------------------------------------------------------------------
def test_the_newer_predicates_on_the_thresholds_themselves():
    assert sr.SCHEDULE_NT == 256
    assert [sr.schedule_blocks((1, n * 64)) for n in (1, 256, 257)] == [1, 1, 2]
    assert sr.schedule_blocks((1024, 1024)) == 1 and sr.schedule_blocks((1025, 1024)) == 2
    # 256 CUs: 524 288 slots in the first stride, tile 2 080 straddles its end
    assert sr.late_tiles((1, 2081 * 64), 256).size == 0
    assert sr.late_tiles((1, 2083 * 64), 256).tolist() == [2081, 2082]
    assert 2080 * sr.PER < sr.CAP_PER_CU * 256 * sr.FOREST_NT <= 2081 * sr.PER
    assert sr.tile_of_cells((65, 130)).ravel()[[0, 63, 64, 129, 64 * 130, 64 * 130 + 129]] \
        .tolist() == [0, 0, 1, 2, 3, 5]
    assert sr.late_mask((1, 2083 * 64), 256).sum() == 2 * 64
    assert sr.full_late_tiles((64, 2083 * 64), 256) == 2
    assert sr.full_late_tiles((63, 2083 * 64), 256) == 0


@pytest.mark.parametrize("cus", sr.CUS)
def test_the_newer_inputs_satisfy_their_predicates_at_any_compute_unit_count(cus):
    tall, wide = sr.tall_shape(cus), sr.wide_shape(cus)
    assert tall == (wide[1], 65) and sr.tiles_of(tall) == sr.tiles_of(wide)
    assert sr.past_the_cap(tall, cus)
    late = sr.late_tiles(tall, cus)
    assert late.size == sr.second_stride_tiles(tall, cus) > 0
    assert late[-1] == sr.tiles_of(tall) - 1
    assert late[0] * sr.PER >= sr.CAP_PER_CU * cus * sr.FOREST_NT > (late[0] - 1) * sr.PER
    assert sr.full_late_tiles(tall, cus) >= 8
    assert sr.full_late_tiles(wide, cus) == 0           # what the wide raster does not supply
    assert sr.late_mask(tall, cus).sum() == sr.full_late_tiles(tall, cus) * 64 * 64 \
        + (late.size - sr.full_late_tiles(tall, cus)) * 64
    if cus == 256:
        assert tall == (67200, 65) and late.tolist() == list(range(2081, 2100))
        assert sr.full_late_tiles(tall, cus) == 9 and sr.late_mask(tall, cus).sum() == 37504
    # the schedule of the D-infinity accumulation does not depend on the compute units
    assert [sr.tiles_of(s) for s in sr.DINF_SHAPES] == [258, 258, 18 * 17]
    assert all(sr.schedule_blocks(s) >= 2 for s in sr.DINF_SHAPES)
    assert sr.schedule_blocks(sr.DINF_SHAPES[0]) == 2
    assert sr.DINF_SHAPES[0][1] % sr.TS == sr.PARTIAL       # a whole tile and a partial one there
    assert divmod(256, 17) == (15, 1)                   # tile 256 of 18 x 17 is (15, 1)
    for shape in sr.strip_shapes(cus).values():
        assert sr.schedule_blocks(shape) >= 3
    assert sr.schedule_blocks(tall) >= 3
    if cus == 256:
        assert sr.schedule_blocks(sr.strip_shapes(cus)["row"]) == 9


@pytest.mark.parametrize("cus", sr.CUS)
def test_the_tall_raster_exercises_its_late_tiles(cus):
    """Conditions on the input, so that a kernel that goes wrong past its first stride cannot
    give the right answer: flow crosses the late tiles' edges both ways, more of it arrives in
    a late tile than a tile holds, the carving lowers cells inside and outside, and the stream
    set divides them."""
    shape = sr.tall_shape(cus)
    codes = sr.tall_codes_2d(cus)
    assert codes.shape == shape and codes.dtype == np.uint8
    late = sr.late_mask(shape, cus)
    steps = sr.late_crossings(codes, cus)
    print(cus, "CUs:", steps)
    assert steps["into"] > 100 and steps["out"] > 100
    assert steps["from_first"] > 0 and steps["to_first"] > 0
    acc = sr.acc_of("tall", cus)
    assert acc[late].max() > 64 * 64                    # the flow entered from outside
    assert acc.max() < 2 ** 32
    stream = acc >= sr.SPARSE_THRESHOLD
    assert stream[late].any() and not stream[late].all()
    _, source, pits, lowered = sr.tall_carved(cus)
    low = source != sr.NONE
    assert pits > 0 and lowered == int(low.sum())
    assert low[late].any() and low[~late].any() and not low[late].all()
    if cus == 256:
        assert steps == {"into": 605, "out": 670, "from_first": 3, "to_first": 68}
        assert int(low[late].sum()) == 13692 and lowered == 1610380


def newer_strips():
    return [(shape, segment) for shape in ((1, 700), (700, 1)) for segment in (None, sr.SEGMENT)]


STRIP_IDS = [f"{by_shape(shape)}-{'segments' if segment else 'one_path'}"
             for shape, segment in newer_strips()]


@pytest.mark.parametrize("shape, segment", newer_strips(), ids=STRIP_IDS)
def test_the_newer_closed_forms_are_the_references_on_700_cells(shape, segment):
    codes = sr.strip_codes(shape, segment)
    stop = sr.strip_answer(shape, segment)["stop"]
    q = sr.strip_weights(shape, seed=7).astype(np.int64)
    assert q.ravel()[0] == 2 ** 31 - 1 and q.max() < 2 ** 31
    assert np.array_equal(sr.strip_flowsum(shape, q, segment), wsum_kahn(codes, q))
    got_stop, total = sum_doubling(codes, q)
    assert np.array_equal(stop, got_stop)
    assert np.array_equal(sr.strip_pathsum(shape, q, segment), total)
    for mode in ("min", "max"):
        for trend in (-1, 1):
            for dtype in (np.float32, np.uint32):
                v = sr.strip_values(shape, trend, dtype, seed=5)
                assert v.dtype == dtype and v.shape == shape
                if dtype == np.float32:         # ties, absent values and both zeros
                    assert np.isnan(v).any() and np.unique(v[~np.isnan(v)]).size < 0.5 * v.size
                for got, want in ((sr.strip_upextreme(shape, v, mode, segment),
                                   upext_kahn(codes, v, mode)),
                                  (sr.strip_pathextreme(shape, v, mode, segment),
                                   extreme_doubling(codes, v, mode)[1:])):
                    assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1])
    # the running extreme changes all along the path when the values drift its way
    v = sr.strip_values((1, 7000), -1, seed=5)
    assert np.unique(sr.strip_upextreme((1, 7000), v, "min")[1]).size > 7000 // sr.TS // 2
    assert np.unique(sr.strip_pathextreme((1, 7000), v, "max")[1]).size > 7000 // sr.TS // 2
    words = sr.strip_words(shape, segment)
    assert words.ravel()[-1] == 0 and (words.ravel()[:-1] != 0).sum() >= 700 - 14
    for frac_bits in (0, 16):
        assert np.array_equal(sr.strip_dinf(shape, frac_bits, segment),
                              accumulate_ref(words, frac_bits))


def test_strip_words_on_the_length_the_schedule_tests_use():
    shape = (1, 16485)
    assert shape == sr.DINF_SHAPES[0]
    for segment in (None, sr.SEGMENT):
        assert np.array_equal(accumulate_ref(sr.strip_words(shape, segment)),
                              sr.strip_answer(shape, segment)["acc"] << 16)


@pytest.mark.parametrize("shape", sr.DINF_SHAPES[1:], ids=by_shape)
def test_random_words_split_on_the_schedule_shapes(shape):
    words = random_acyclic_words(shape, seed=sr.DINF_SEED)
    share = counts_of(words)["split_cells"] / words.size
    print(by_shape(shape), "split share", share)
    assert share >= 0.05
    assert (0.075 < share < 0.076) if shape[0] == 3 else (0.111 < share < 0.112)


def test_the_numbering_rule_on_a_raster_of_several_tiles():
    codes = np.zeros((70, 130), np.uint8)               # every cell its own basin
    labels, outlets = sr.compact_by_rule(codes)
    assert labels[0, :3].tolist() == [1, 2, 3] and labels[1, 0] == 65       # row-major in a tile
    assert labels[0, 64] == 64 * 64 + 1 and labels[0, 128] == 2 * 64 * 64 + 1
    assert labels[64, 0] == 64 * 130 + 1 and labels[69, 129] == 70 * 130    # the partial tiles
    assert np.array_equal(outlets[labels.ravel() - 1], np.arange(70 * 130))
    codes = sr.random_acyclic_codes(70, 130, seed=3, ramp=True)
    labels, outlets = sr.compact_by_rule(codes)
    assert np.array_equal(outlets[labels.ravel() - 1] + 1, labels_doubling(codes).ravel())
    assert np.array_equal(np.unique(labels), np.arange(1, outlets.size + 1))
