"""
Size regimes of the tiled operators: inputs for tests/test_size_regimes.py (the predicates and
the closed forms, on the CPU) and tests/test_gpu_size_regimes.py (the HIP operators on them).
A plain helper module: mirrored constants, one predicate per host-side decision that depends
on the size of the raster, builders of the rasters that reach the far side of each decision,
and the answers of the constructed ones in closed form.

Every other raster that the suite checks bit for bit has 130 x 257 or 200 x 333 cells, where
every decision below takes its trivial value:

  decision                                             trivial until        predicate
  chunks of a rank scan (hdem_scan.h, under the zonal   4 096 words          scan_chunks
    statistics, the stream network, the depressions)
  per-thread loop of the one workgroup over the        1 024 chunks         one_kernel_loops
    chunk sums (hdem_scan_one_kernel, ``chunk >= 2``)
  the same loop over the tile counts of Watersheds     1 024 tiles          watershed_scan_loops
    (hdem_scan_exclusive_small)
  second stride of the grid-stride forest kernels      8 * CUs workgroups   past_the_cap,
    (flowacc / upstream degree kernels, the forests                           second_stride_tiles
    of Watersheds and the flow trace)
  streamnet_end_kernel or streamnet_end_sparse_kernel  K >= 2 * words       dense_ends

The words of a scan are ``zonal_words`` (one bit per id 1 ... H * W) for the zonal statistics
and ``tile_words`` (one 64-bit word per tile row: H * ceil(W / 64)) for the stream network and
the depressions, so a raster one column wide and 4 097 rows long already has two chunks, and a
strip of 140 000 cells has 2 188 tiles.
"""
import functools

import numpy as np

from test_flowacc import acc_kahn, random_acyclic_codes, receivers
from test_streamorder import link_stops
from test_watersheds import labels_doubling
from test_zonal import blobs, extremes, own_zones

U32 = np.uint32
E, S = 1, 4
NONE = 0xFFFFFFFF

# ---------------------------------------------------------------------------
# the kernels' constants, each with the line it mirrors
# ---------------------------------------------------------------------------
TS = 64                     # hdem_d8tile.h `constexpr int TS = 64` (tile edge, bits of a word)
PER = 252                   # hdem_d8tile.h `constexpr int PER = 4 * TS - 4`
SCAN_CHUNK = 4096           # hdem_scan.h `HDEM_SCAN_CHUNK = HDEM_SCAN_NT * HDEM_SCAN_PER` (256 * 16)
ONE_NT = 1024               # hdem_scan.h `HDEM_SCAN_ONE_NT = 1024`
WATERSHED_SCAN_NT = 1024    # the same workgroup: hdem_watershed.hip calls hdem_scan_exclusive_small
FOREST_NT = 256             # `constexpr int NT = 256` of hdem_flowacc.hip, hdem_upstream.hip,
                            # hdem_watershed.hip and hdem_flowtrace.hip (the forest workgroups)
CAP_PER_CU = 8              # hdem_d8tile.h d8_forest_plan_of `(int64_t)ctx->num_cus * 8`; the same
                            # in `degree_blocks` of hdem_flowacc.hip and hdem_upstream.hip
CUS = (64, 256, 304)        # compute-unit counts the inputs are checked at; the MI355X has 256


def _ceil(a, b):
    return -(-int(a) // int(b))


# ---------------------------------------------------------------------------
# the predicates
# ---------------------------------------------------------------------------
def tiles_of(shape):
    """The number of 64 x 64 tiles (d8_grid_of: ``tiles_y * tiles_x``)."""
    return _ceil(shape[0], TS) * _ceil(shape[1], TS)


def zonal_words(shape):
    """hdem_zonal.hip zonal_carve: ``ws->words = (cells + 63) / 64``."""
    return _ceil(shape[0] * shape[1], 64)


def tile_words(shape):
    """hdem_streamnet.hip, hdem_depressions.hip: ``words = (int64_t)H * g.tiles_x``."""
    return shape[0] * _ceil(shape[1], TS)


def scan_chunks(words):
    """``chunks = (words + SCAN_CHUNK - 1) / SCAN_CHUNK``: the workgroups of the sums and the
    apply kernel; above 1 a chunk offset other than ``sums[0] = 0`` is used."""
    return _ceil(words, SCAN_CHUNK)


def one_kernel_loops(words):
    """``chunk = (n + ONE_NT - 1) / ONE_NT`` of the scan's one workgroup, n the chunks: what a
    thread adds up; 1 until there are more than 1 024 chunks."""
    return _ceil(scan_chunks(words), ONE_NT)


def watershed_scan_loops(shape):
    """``chunk = (n + HDEM_SCAN_ONE_NT - 1) / HDEM_SCAN_ONE_NT`` of hdem_scan_one_kernel, n the
    tiles: what a thread of the scan over the watersheds' tile counts adds up."""
    return _ceil(tiles_of(shape), WATERSHED_SCAN_NT)


def forest_blocks(shape):
    """``(nslots + NT - 1) / NT`` with ``nslots = tiles * PER``: the workgroups a forest kernel
    would have without the cap."""
    return _ceil(tiles_of(shape) * PER, FOREST_NT)


def past_the_cap(shape, cus):
    """The grid of a grid-stride forest kernel is ``min(forest_blocks, 8 * CUs)``: true when
    the kernel takes a second stride."""
    return forest_blocks(shape) > CAP_PER_CU * cus


def second_stride_tiles(shape, cus):
    """The tiles all of whose perimeter slots are reached in the second stride or later."""
    first = _ceil(CAP_PER_CU * cus * FOREST_NT, PER)
    return max(0, tiles_of(shape) - first)


def dense_ends(count, words):
    """hdem_streamnet.hip launch_tile_and_end: ``if (a.K >= 2 * words)`` streamnet_end_kernel,
    else streamnet_end_sparse_kernel."""
    return count >= 2 * words


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------
# 1. zonal statistics: ids past one scan chunk
# ---------------------------------------------------------------------------
# shape -> (words, chunks): the last id of 512 x 512 is the last bit of chunk 0; the second
# chunk of 5 x 52 429 is one word (and its tiles are partial); 1024 x 512 is two chunks exactly
ZONAL_SHAPES = {(512, 512): (4096, 1), (5, 52429): (4097, 2), (1024, 512): (8192, 2),
                (771, 700): (8433, 3)}
# the first and the last id of the first three chunks
CHUNK_EDGE_IDS = (1, 262144, 262145, 524288, 524289)


def chunk_edges(shape, seed=0):
    """A raster holding exactly the ids {1, 262 144, 262 145, 524 288, 524 289, H * W}, as far
    as the raster has them: a random one at every cell, each at least once."""
    n = shape[0] * shape[1]
    ids = np.array(sorted({i for i in CHUNK_EDGE_IDS if i <= n} | {n}), U32)
    zones = ids[np.random.default_rng(seed).integers(0, ids.size, shape)]
    zones.flat[:ids.size] = ids
    return np.ascontiguousarray(zones, U32)


def blobs_to_the_last_id(shape, seed=0):
    """``blobs`` whose last cell holds the id H * W, the last bit of the last word."""
    zones = blobs(shape, seed)
    zones.flat[-1] = shape[0] * shape[1]
    return zones


ZONE_KINDS = {"own": own_zones, "blobs": blobs_to_the_last_id, "edges": chunk_edges,
              "extremes": extremes}
# ... those whose ids lie in every chunk of every shape
FILLING_KINDS = ("own", "blobs")


@functools.lru_cache(maxsize=None)
def zones_of(kind, shape):
    return _frozen(ZONE_KINDS[kind](shape))


def ids_per_chunk(zones):
    """The number of ids present in every scan chunk of the zones' bitmap."""
    ids = np.unique(zones[zones > 0]).astype(np.int64)
    return np.bincount((ids - 1) // (64 * SCAN_CHUNK),
                       minlength=scan_chunks(zonal_words(zones.shape)))


# ---------------------------------------------------------------------------
# 2. stream order and stream network: tile words past one scan chunk
# ---------------------------------------------------------------------------
# shape -> (words, chunks)
STREAM_SHAPES = {(4096, 1): (4096, 1), (4097, 1): (4097, 2), (1400, 130): (4200, 2),
                 (2800, 130): (8400, 3)}
STREAM_KINDS = ("all", "acc", "mask")
# 2800 x 130, ramp: `acc >= 4` leaves 37 010 links for 8 400 words, which is still dense
SPARSE_THRESHOLD = 10        # ... and `acc >= 10` 15 032, below the 16 800 of two per word


@functools.lru_cache(maxsize=None)
def stream_case(shape, ramp):
    """(codes, their accumulation as uint32), made once and read-only."""
    codes = random_acyclic_codes(*shape, seed=shape[0] * 1000 + shape[1], ramp=ramp)
    return _frozen(codes, acc_kahn(codes).astype(U32))


def stream_form(kind, shape, acc):
    """(streams, threshold) as the operators take them; ``sparse``: a threshold high enough
    for fewer than two links per word."""
    if kind == "all":
        return None, None
    if kind == "acc":
        return acc, 4
    if kind == "sparse":
        return acc, SPARSE_THRESHOLD
    return np.random.default_rng(shape[1]).random(shape) < 0.6, None


def link_count(codes, stream):
    """K: the number of links (of cells that end one)."""
    return int(link_stops(codes, stream).sum())


# One column, all S, the streams in runs: every run is one link.
TALL = (4 * 1024 * 1024 + 100, 1)


def tall_runs(rows, seed=0):
    """(tops, ends) of the runs in a column of ``rows`` cells: 300 ... 1 500 cells long and
    1 ... 600 cells apart, so that every scan chunk (4 096 rows) holds an end and no run lines
    up with a tile; the last run ends on the last cell but one."""
    rng = np.random.default_rng(seed)
    m = rows // 301 + 2
    length, gap = rng.integers(300, 1501, m), rng.integers(1, 601, m)
    ends = np.cumsum(length + gap) - 1
    tops = ends - length + 1
    keep = ends < rows - 40
    tops, ends = tops[keep], ends[keep]
    return _frozen(np.append(tops, rows - 30), np.append(ends, rows - 2))


def tall_codes(rows):
    return np.full((rows, 1), S, np.uint8)


def tall_mask(rows, runs):
    tops, ends = runs
    edge = np.zeros(rows + 1, np.int64)
    edge[tops] += 1
    edge[ends + 1] -= 1
    return (np.cumsum(edge[:-1]) > 0).reshape(rows, 1)


def tall_answer(rows, runs, dem=None, cellsize=1.0):
    """The table, the ``row`` raster, the counters and the (order, magnitude, link) rasters of
    ``tall_codes`` with ``tall_mask`` as streams, run by run: no run drains into another, the
    dry cells above a run are its catchment, those below the last run reach no stream."""
    tops, ends = (np.asarray(a, np.int64) for a in runs)
    k = ends.size
    cells = ends - tops + 1
    ncard = cells - 1
    table = {"end": ends.astype(U32), "top": tops.astype(U32), "down": np.full(k, NONE, U32),
             "order": np.ones(k, np.uint8), "magnitude": np.ones(k, U32),
             "cells": cells.astype(U32), "ncard": ncard.astype(U32), "ndiag": np.zeros(k, U32),
             "length": (ncard.astype(np.float64) * float(cellsize)).astype(np.float32),
             "catchment": np.diff(ends, prepend=-1).astype(U32)}
    if dem is not None:
        flat = np.asarray(dem, np.float32).ravel()
        table["z_top"], table["z_end"] = flat[tops], flat[ends]
    mask = tall_mask(rows, runs).ravel()
    run_of = np.cumsum(np.bincount(tops, minlength=rows))          # 1 + the run at or above
    row = np.where(mask, run_of, 0).astype(U32).reshape(rows, 1)
    counters = {"links": k, "stream_cells": int(cells.sum()),
                "catchment_cells": int(ends[-1]) + 1, "tops": k}
    rasters = {"order": mask.astype(np.uint8).reshape(rows, 1),
               "magnitude": mask.astype(U32).reshape(rows, 1),
               "link": np.where(mask, ends[np.maximum(run_of, 1) - 1] + 1, 0)
               .astype(U32).reshape(rows, 1)}
    return table, row, counters, rasters


# ---------------------------------------------------------------------------
# 3. depressions: the same column
# ---------------------------------------------------------------------------
def tall_dem(rows, seed=0):
    """(dem, filled): random in [0, 1) and ``max(dem, 0.5)``; half of the cells are raised."""
    dem = np.random.default_rng(seed).random((rows, 1), dtype=np.float32)
    return dem, np.maximum(dem, np.float32(0.5))


def roots_per_chunk(dem, filled):
    """The number of depressions of a one-column pair whose first cell lies in every chunk."""
    raised = (filled > dem).ravel()
    first = raised & ~np.concatenate([[False], raised[:-1]])
    return np.bincount(np.flatnonzero(first) // SCAN_CHUNK,
                       minlength=scan_chunks(tile_words(dem.shape)))


# ---------------------------------------------------------------------------
# 4. strips past the grid cap
# ---------------------------------------------------------------------------
PARTIAL = 37                # cells of a strip's last tile
SECOND_STRIDE = 100         # whole tiles a strip has in the second stride
SEGMENT = 50                # cells from one terminal to the next: no divisor of the tile edge


def strip_length(cus):
    """The smallest multiple of 64, plus a partial tile, at which a strip is past the cap with
    ``SECOND_STRIDE`` whole tiles behind it: the last workgroup's second stride alone would
    reach perimeter slots that a one-cell-wide tile does not use.  139 557 at 256 CUs."""
    tiles = 1
    while second_stride_tiles((1, tiles * TS), cus) < SECOND_STRIDE:
        tiles += 1
    return (tiles - 1) * TS + PARTIAL


def strip_shapes(cus):
    n = strip_length(cus)
    return {"row": (1, n), "column": (n, 1)}


def wide_shape(cus):
    """65 rows (the second row of tiles is one cell high) by as many whole tile columns, a
    multiple of 50 of them, as put the raster past the cap: 65 x 67 200 at 256 CUs."""
    columns = 50
    while not past_the_cap((65, columns * TS), cus):
        columns += 50
    return 65, columns * TS


def strip_codes(shape, segment=None):
    """All E (a row) or all S (a column): one path to the last cell, which points outside.
    ``segment``: every ``segment``-th cell is terminal (code 0) instead."""
    codes = np.full(shape, E if shape[0] == 1 else S, np.uint8)
    if segment:
        codes.reshape(-1)[segment - 1::segment] = 0
    return codes


def strip_answer(shape, segment=None):
    """What the operators give on ``strip_codes``, as int64 rasters: position in the path
    counted from 1 (``acc``), steps to the end (``to_end``: the trace's ncard), 1 + the end's
    index (``stop``, also the outlet label), the compact label, steps from the head (``up``),
    and ``outlets``, the ends in ascending order (on a strip the order by tile and row-major
    inside a tile is the order of the flat index)."""
    n = shape[0] * shape[1]
    at = np.arange(n, dtype=np.int64)
    head = at // segment * segment if segment else np.zeros(n, np.int64)
    end = np.minimum(head + segment - 1, n - 1) if segment else np.full(n, n - 1, np.int64)
    answer = {"acc": at - head + 1, "to_end": end - at, "stop": end + 1,
              "compact": (at // segment if segment else head) + 1, "up": at - head}
    answer = {name: a.reshape(shape) for name, a in answer.items()}
    answer["outlets"] = np.unique(end)
    return answer


def compact_by_rule(codes):
    """(labels, outlets) of ``Watersheds(labels="compact")`` from the numbering the operator
    documents: the terminal cells by 64 x 64 tile (row-major), row-major inside a tile."""
    h, w = codes.shape
    outlet = labels_doubling(codes).astype(np.int64).ravel() - 1
    terminals = np.flatnonzero(receivers(codes) < 0)
    y, x = np.divmod(terminals, w)
    order = np.lexsort((x % TS, y % TS, x // TS, y // TS))
    outlets = terminals[order]
    number = np.zeros(h * w, np.int64)
    number[outlets] = np.arange(1, outlets.size + 1)
    return number[outlet].reshape(h, w), outlets


@functools.lru_cache(maxsize=None)
def wide_codes(cus):
    shape = wide_shape(cus)
    return _frozen(random_acyclic_codes(*shape, seed=shape[1], ramp=True))
