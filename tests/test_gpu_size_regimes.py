"""
The tiled operators past one scan chunk and one grid stride, on the MI355X: the inputs of
tests/size_regimes.py, each reaching the far side of a host-side decision that every other
raster of the suite leaves at its trivial value, against the suite's own references and the
closed forms that tests/test_size_regimes.py holds to those references.  Every comparison is
``np.array_equal`` or ``same_bits`` / ``same_table``; a test that exists for a branch asserts
that branch's predicate on its own input first.

  ZonalStatistics, zonal_count, broadcast     ids in two and three chunks of hdem_scan.h
  StreamOrder, StreamNetwork                  tile words in two and three chunks of the same
                                              scan, both forms of the end kernel above one chunk
  the column of 4 194 404 rows                the per-thread loop of hdem_scan_one_kernel, through
                                              the stream network and the depressions (1 025 chunks)
  strips and 65 x 67 200 (at 256 CUs)         the second stride of the grid-stride forest
                                              kernels; the same loop of hdem_scan_one_kernel
                                              through Watersheds (hdem_scan_exclusive_small over
                                              more than 1 024 tile counts)

The per-thread loop of hdem_scan_one_kernel (``chunk >= 2``) is reached three ways: by the two
tall-column tests (4 194 404 rows, 1 025 chunk sums) through the stream network and through
the depressions, and by the ``wide`` and strip cases through Watersheds (more than 1 024 tile
counts).  Only the zonal path does not get there: it needs more than 1 024 chunks of 262 144
ids, a raster of more than 268 435 456 cells.

The value-only mutant of that kernel that was run against this file, once, with the tests it
fails (it keeps every store in bounds: the ranks it gives stay below the true ones and a rank
is compared with K before it indexes a column, so ranks collide and rows are wrong, nothing is
written elsewhere).  While the scan had a copy per operator the same mutation failed 13 tests
in the header (the zonal ones below) and 19 in the stream network's copy; the files that used
these kernels before this one -- tests/test_gpu_zonal.py, tests/test_gpu_streamnet.py,
tests/test_gpu_streamorder.py, tests/test_gpu_terrain_attributes.py -- passed under both.
  hdem_scan_one_kernel writing ``sums[t] = 0`` -> 36 of the 55 tests:
      test_zonal_tables_with_ids_past_one_scan_chunk at 5 x 52 429, 1024 x 512 and 771 x 700
      with all four zone kinds (512 x 512, one chunk, passes), and
      test_zonal_uint32_values_in_three_chunks (13);
      test_stream_networks_past_one_scan_chunk at 1400 x 130 and 2800 x 130 with all four
      stream sets, flat and ramp (both end kernels), and at 4097 x 1 with every cell a stream
      cell (its second chunk is one word: the other stream sets leave no end there; 4096 x 1,
      one chunk, passes), and
      test_the_tall_column_takes_the_per_thread_loop_of_the_streamnet_scan (19);
      test_the_tall_column_takes_the_per_thread_loop_of_the_depression_scan (1);
      test_strips_take_the_second_stride_of_the_forest_kernels with ``segments``, row and
      column (the compact labels of 2 792 basins in 2 181 tiles; ``one_path`` has one basin
      and passes), and
      test_wide_raster_watersheds_match_the_doubling_reference_and_the_numbering_rule (3);
      nothing else
"""
import numpy as np
import pytest

import hydrodem_amd as hd
import size_regimes as sr
import test_gpu_depressions as gpu_depressions
import test_gpu_streamnet as gpu_streamnet
import test_gpu_zonal as gpu_zonal
from hydrodem_amd import backend, zonal
from test_flowacc import acc_kahn, terminal_mask
from test_flowtrace import distance_of, trace_doubling
from test_gpu_flowacc import flowacc
from test_gpu_flowtrace import trace
from test_gpu_streamnet import links_of, run
from test_gpu_upstream import up
from test_gpu_watersheds import watersheds
from test_streamnet import COUNTERS, random_dem, same_table
from test_streamorder import link_ends, order_kahn, stream_of
from test_upstream import upstream_kahn
from test_watersheds import labels_doubling
from test_zonal import float_values, same_bits, zonal_np

pytestmark = pytest.mark.gpu

U32 = np.uint32
CELL = 12.5


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


# ---------------------------------------------------------------------------
# 1. ZonalStatistics: the chunk offsets of hdem_scan.h
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(sr.ZONAL_SHAPES), ids=by_shape)
@pytest.mark.parametrize("kind", list(sr.ZONE_KINDS))
def test_zonal_tables_with_ids_past_one_scan_chunk(kind, shape):
    words, chunks = sr.ZONAL_SHAPES[shape]
    assert sr.zonal_words(shape) == words and sr.scan_chunks(words) == chunks
    zones = sr.zones_of(kind, shape)
    filled = sr.ids_per_chunk(zones)
    assert filled[-1] > 0 and (kind == "extremes" or (filled > 0).all())
    values = gpu_zonal.with_a_nan_zone(zones, float_values(shape, shape[0]))
    want, counters = zonal_np(zones, values)
    table, stats = zonal.zonal(zones, values)
    assert gpu_zonal.same_table(table, want)
    assert {k: stats[k] for k in gpu_zonal.COUNTERS} == counters
    count, _ = zonal.zonal_count(zones)
    assert count == counters["zones"] == int(filled.sum())
    # the device form against the host form
    with backend.DeviceRaster.from_host(zones) as dz, backend.DeviceRaster.from_host(values) as dv:
        on_device, device_stats = zonal.zonal_dev(dz, dv)
        assert list(on_device) == list(table)
        assert all(same_bits(on_device[name], table[name]) for name in table)
        assert {k: device_stats[k] for k in counters} == counters
        assert zonal.zonal_count_dev(dz)[0] == count
        # a lookup by rank, straight from the table of the reference
        for name, fill in (("count", 7), ("min", -1.5)):
            with zonal.zonal_broadcast_dev(dz, want[name], fill) as raster:
                assert same_bits(raster.to_host(),
                                 gpu_zonal.broadcast_np(zones, want["id"], want[name], fill))
    operator = hd.ZonalStatistics(values)
    ids = operator.apply(zones)["id"]
    assert same_bits(ids, want["id"])
    assert same_bits(operator.broadcast("count", 7),
                     gpu_zonal.broadcast_np(zones, ids, want["count"], 7))
    assert same_bits(operator.broadcast("min", -1.5),
                     gpu_zonal.broadcast_np(zones, ids, want["min"], -1.5))


def test_zonal_uint32_values_in_three_chunks():
    shape = (771, 700)
    assert sr.scan_chunks(sr.zonal_words(shape)) == 3
    zones = sr.zones_of("blobs", shape)
    assert (sr.ids_per_chunk(zones) > 0).all()
    values = np.random.default_rng(5).integers(0, 2 ** 32, shape, dtype=np.uint64).astype(U32)
    gpu_zonal.check(zones, values)
    gpu_zonal.check(zones)


# ---------------------------------------------------------------------------
# 2. StreamOrder and StreamNetwork: the scan of hdem_scan.h under hdem_streamnet.hip
# ---------------------------------------------------------------------------
def stream_kinds(shape):
    return sr.STREAM_KINDS + (("sparse",) if shape[1] > 1 else ())


@pytest.mark.parametrize("shape, kind", [(shape, kind) for shape in sr.STREAM_SHAPES
                                         for kind in stream_kinds(shape)],
                         ids=lambda v: by_shape(v) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("ramp", [False, True], ids=["flat", "ramp"])
def test_stream_networks_past_one_scan_chunk(shape, kind, ramp):
    words, chunks = sr.STREAM_SHAPES[shape]
    assert sr.tile_words(shape) == words and sr.scan_chunks(words) == chunks
    codes, acc = sr.stream_case(shape, ramp)
    streams, threshold = sr.stream_form(kind, shape, acc)
    stream = stream_of(codes, streams, threshold)
    dem = random_dem(shape, shape[0] + shape[1])
    outs, count = links_of(codes, streams, threshold)
    assert count == sr.link_count(codes, stream)
    # which of the two end kernels runs
    if shape[1] > 1:
        assert sr.dense_ends(count, words) == (kind != "sparse")
    else:
        assert not sr.dense_ends(count, words)
    order, magnitude = order_kahn(codes, stream)
    assert np.array_equal(outs["order"], order) and np.array_equal(outs["magnitude"], magnitude)
    assert np.array_equal(outs["link"], link_ends(codes, stream))
    got = run(codes, streams, threshold, dem, CELL, of=(outs, count))
    gpu_streamnet.check(got, codes, stream, dem, CELL)


@pytest.fixture(scope="module")
def tall():
    rows = sr.TALL[0]
    runs = sr.tall_runs(rows)
    dem = np.random.default_rng(7).normal(100.0, 30.0, sr.TALL).astype(np.float32)
    return runs, dem, sr.tall_answer(rows, runs, dem, CELL)


def test_the_tall_column_takes_the_per_thread_loop_of_the_streamnet_scan(tall):
    rows = sr.TALL[0]
    words = sr.tile_words(sr.TALL)
    assert sr.scan_chunks(words) > sr.ONE_NT and sr.one_kernel_loops(words) == 2
    runs, dem, (table, row, counters, rasters) = tall
    assert (np.bincount(runs[1] // sr.SCAN_CHUNK, minlength=sr.scan_chunks(words)) > 0).all()
    assert not sr.dense_ends(runs[1].size, words)
    codes, mask = sr.tall_codes(rows), sr.tall_mask(rows, runs)
    outs, count = links_of(codes, mask)
    assert count == counters["links"]
    for name in ("order", "magnitude", "link"):
        assert outs[name].dtype == rasters[name].dtype, name
        assert np.array_equal(outs[name], rasters[name]), name
    got_table, got_row, stats = run(codes, mask, None, dem, CELL, of=(outs, count))
    assert list(got_table) == list(gpu_streamnet.NAMES)
    assert same_table(got_table, table)
    assert got_row.dtype == U32 and np.array_equal(got_row, row)
    assert {k: stats[k] for k in COUNTERS} == counters


# ---------------------------------------------------------------------------
# 3. Depressions, compact labels: the scan of hdem_scan.h under hdem_depressions.hip
# ---------------------------------------------------------------------------
def test_the_tall_column_takes_the_per_thread_loop_of_the_depression_scan():
    words = sr.tile_words(sr.TALL)
    assert sr.scan_chunks(words) > sr.ONE_NT and sr.one_kernel_loops(words) == 2
    dem, filled = sr.tall_dem(sr.TALL[0])
    assert (sr.roots_per_chunk(dem, filled) > 0).all()
    _, count, _, _ = gpu_depressions.check(dem, filled)
    assert count == int(sr.roots_per_chunk(dem, filled).sum())


# ---------------------------------------------------------------------------
# 4. strips past the grid cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("segment", [None, sr.SEGMENT], ids=["one_path", "segments"])
@pytest.mark.parametrize("strip", ["row", "column"])
def test_strips_take_the_second_stride_of_the_forest_kernels(cus, strip, segment):
    shape = sr.strip_shapes(cus)[strip]
    assert sr.past_the_cap(shape, cus)
    assert sr.second_stride_tiles(shape, cus) == sr.SECOND_STRIDE
    assert sr.watershed_scan_loops(shape) >= 2
    codes = sr.strip_codes(shape, segment)
    want = sr.strip_answer(shape, segment)
    zero = np.zeros(shape, np.int64)

    acc = flowacc(codes)
    assert acc.dtype == U32 and np.array_equal(acc, want["acc"])

    got, stats = trace(codes, cellsize=CELL)
    assert np.array_equal(got["stop"], want["stop"])
    assert np.array_equal(got["ncard"], want["to_end"]) and np.array_equal(got["ndiag"], zero)
    assert np.array_equal(got["distance"], distance_of(want["stop"], want["to_end"], zero, CELL))
    assert stats["stops"] == want["outlets"].size

    assert np.array_equal(watersheds(codes), want["stop"])
    basins = hd.Watersheds(labels="compact")
    compact = basins.apply(codes)
    assert compact.dtype == U32 and np.array_equal(compact, want["compact"])
    assert basins.outlets.dtype == U32 and np.array_equal(basins.outlets, want["outlets"])
    assert basins.stats["basins"] == want["outlets"].size
    if segment:         # basins in more tiles than hdem_scan_one_kernel has threads
        tiles_with_outlets = np.unique(want["outlets"] // sr.TS).size
        assert tiles_with_outlets > sr.WATERSHED_SCAN_NT and want["outlets"].size > 2048

    outs = up(codes, ("ncard", "ndiag", "length"), CELL)
    assert np.array_equal(outs["ncard"], want["up"]) and np.array_equal(outs["ndiag"], zero)
    assert np.array_equal(outs["length"], (want["up"] * CELL).astype(np.float32))


@pytest.fixture(scope="module")
def wide(cus):
    shape = sr.wide_shape(cus)
    assert sr.past_the_cap(shape, cus) and sr.second_stride_tiles(shape, cus) > 0
    assert sr.watershed_scan_loops(shape) >= 2
    return sr.wide_codes(cus)


def test_wide_raster_flow_accumulation_matches_the_kahn_reference(wide):
    assert np.array_equal(flowacc(wide), acc_kahn(wide))


def test_wide_raster_flow_trace_matches_the_doubling_reference(wide):
    got, _ = trace(wide, cellsize=CELL)
    stop, ncard, ndiag = trace_doubling(wide)
    assert np.array_equal(got["stop"], stop)
    assert np.array_equal(got["ncard"], ncard) and np.array_equal(got["ndiag"], ndiag)
    assert np.array_equal(got["distance"], distance_of(stop, ncard, ndiag, CELL))


def test_wide_raster_watersheds_match_the_doubling_reference_and_the_numbering_rule(wide):
    assert np.array_equal(watersheds(wide), labels_doubling(wide))
    labels, outlets = sr.compact_by_rule(wide)
    basins = hd.Watersheds(labels="compact")
    assert np.array_equal(basins.apply(wide), labels)
    assert np.array_equal(basins.outlets, outlets)
    assert basins.stats["basins"] == outlets.size == int(terminal_mask(wide).sum())
    assert np.unique(outlets // wide.shape[1] // sr.TS * (wide.shape[1] // sr.TS)
                     + outlets % wide.shape[1] // sr.TS).size > sr.WATERSHED_SCAN_NT


def test_wide_raster_upstream_length_matches_the_kahn_reference(wide):
    ncard, ndiag = upstream_kahn(wide)
    outs = up(wide)
    assert np.array_equal(outs["ncard"], ncard) and np.array_equal(outs["ndiag"], ndiag)
