"""
Size regimes of the tiled operators: inputs for tests/test_size_regimes.py (the predicates and
the closed forms, on the CPU), tests/test_gpu_size_regimes.py and
tests/test_gpu_size_regimes_newer.py (the HIP operators on them).
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
  second stride of flowsum_forest_degree_kernel,       8 * CUs workgroups   past_the_cap,
    upext_forest_degree_kernel and                                            late_tiles,
    flowpath_forest_kernel (private copies of the                             full_late_tiles
    same grid: weighted accumulation, upstream
    extremes and the breach, path sums and extremes)
  second workgroup of dinfacc_schedule_kernel (one     256 tiles            schedule_blocks
    thread per tile: D-infinity accumulation)

The last two rows are run by tests/test_gpu_size_regimes_newer.py, which also takes the four
older forest operators to ``tall_codes_2d``: the ``wide`` raster has no full tile past the first
stride (its late tiles are one cell high), the same extent upright has nine at 256 CUs.

The words of a scan are ``zonal_words`` (one bit per id 1 ... H * W) for the zonal statistics
and ``tile_words`` (one 64-bit word per tile row: H * ceil(W / 64)) for the stream network and
the depressions, so a raster one column wide and 4 097 rows long already has two chunks, and a
strip of 140 000 cells has 2 188 tiles.
"""
import functools

import numpy as np

from hydrodem_amd import dinf
from test_flowacc import acc_kahn, random_acyclic_codes, receivers
from test_streamorder import link_stops
from test_upextreme import IDENTITY, carve_ref, split_words, words_of
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
# The operators merged since keep the same two figures in copies of their own:
#   hdem_flowsum.hip    `constexpr int NT = 256`, `forest_blocks = (nslots + NT - 1) / NT` and
#                       `degree_blocks = min(forest_blocks, (int64_t)ctx->num_cus * 8)`
#   hdem_upextreme.hip  `constexpr int NT = 256`, `forest_blocks = (g.nslots + NT - 1) / NT` and
#                       the same `degree_blocks`
#   hdem_flowpath.hip   `constexpr int NT = 256` and `d8_forest_plan_of(ctx, nslots, NT)`, whose
#                       grid is `min((nslots + nt - 1) / nt, (int64_t)ctx->num_cus * 8)`
# ... the same figures as FOREST_NT and CAP_PER_CU, so forest_blocks and past_the_cap serve them
SCHEDULE_NT = 256           # hdem_stencil_tile.h `constexpr int NT = 256`, the workgroup of
                            # dinfacc_schedule_kernel (hdem_dinf.hip): one thread per tile
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


# ---------------------------------------------------------------------------
# 5. the same extent stood upright: full tiles in the second stride
# ---------------------------------------------------------------------------
def tall_shape(cus):
    """``wide_shape`` transposed: two tile columns, the second one cell wide, so that the tiles
    past the first stride alternate between full 64 x 64 tiles and one-column tiles.
    67 200 x 65 at 256 CUs."""
    return wide_shape(cus)[1], 65


@functools.lru_cache(maxsize=None)
def tall_codes_2d(cus):
    """``random_acyclic_codes`` with the ramp, as ``wide_codes``, and the west column made a
    trunk: all S down to a terminal cell in the last row.  The ramp sends every path north-west
    and the raster is 65 cells wide, so on its own no path collects more than about 1 900 cells
    (1 915 at 256 CUs) and hardly a step enters the last tiles from the tiles above them (2 at
    256 CUs, none at 64 and 304).  The trunk collects what reaches the west edge and carries it
    south into the tiles past the first stride.  Every other cell still steps to a strictly
    lower one and the trunk never leaves its column, so the codes stay acyclic."""
    shape = tall_shape(cus)
    codes = random_acyclic_codes(*shape, seed=shape[0], ramp=True)
    codes[:, 0] = S
    codes[-1, 0] = 0
    return _frozen(codes)


def late_tiles(shape, cus):
    """The indices (row-major, ``ty * tiles_x + tx``; a tile's slots are ``tile * PER ...``) of
    the tiles all of whose perimeter slots lie past the first stride: the last
    ``second_stride_tiles`` of them."""
    tiles = tiles_of(shape)
    return np.arange(tiles - second_stride_tiles(shape, cus), tiles)


def tile_of_cells(shape):
    """The tile index of every cell, int64."""
    y, x = np.indices(shape, dtype=np.int64)
    return y // TS * _ceil(shape[1], TS) + x // TS


def late_mask(shape, cus):
    """The cells of ``late_tiles``."""
    late = late_tiles(shape, cus)
    return tile_of_cells(shape) >= late[0] if late.size else np.zeros(shape, bool)


def full_late_tiles(shape, cus):
    """The number of ``late_tiles`` that are whole 64 x 64 tiles."""
    tiles_x = _ceil(shape[1], TS)
    ty, tx = np.divmod(late_tiles(shape, cus), tiles_x)
    return int((((ty + 1) * TS <= shape[0]) & ((tx + 1) * TS <= shape[1])).sum())


def late_crossings(codes, cus):
    """The D8 steps that change tile with a late tile on either side: ``into`` one (from any
    other tile), ``out`` of one (to any other tile), and of these the steps between a late tile
    and a tile of the first stride, ``from_first`` and ``to_first``."""
    rec = receivers(codes)
    tile = tile_of_cells(codes.shape).ravel()
    first_late = late_tiles(codes.shape, cus)[0]
    src = np.flatnonzero(rec >= 0)
    dst = rec[src]
    src, dst = tile[src], tile[dst]
    cross = src != dst
    return {"into": int((cross & (dst >= first_late)).sum()),
            "out": int((cross & (src >= first_late)).sum()),
            "from_first": int(((src < first_late) & (dst >= first_late)).sum()),
            "to_first": int(((src >= first_late) & (dst < first_late)).sum())}


BREACH_SEED = 3              # the DEM of the breach test: default_rng(3).random(shape) * 100


def tall_dem_2d(cus):
    shape = tall_shape(cus)
    return (np.random.default_rng(BREACH_SEED).random(shape) * 100).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tall_carved(cus):
    """``carve_ref`` of ``tall_dem_2d`` along ``tall_codes_2d``: (carved, source, pits, lowered)."""
    carved, source, pits, lowered = carve_ref(tall_dem_2d(cus), tall_codes_2d(cus))
    return _frozen(carved, source) + (pits, lowered)


@functools.lru_cache(maxsize=None)
def acc_of(kind, cus):
    """``acc_kahn`` of the wide or the tall codes, int64, made once."""
    return _frozen(acc_kahn(wide_codes(cus) if kind == "wide" else tall_codes_2d(cus)))


# ---------------------------------------------------------------------------
# 6. the schedule of the D-infinity accumulation: one thread per tile
# ---------------------------------------------------------------------------
def schedule_blocks(shape):
    """hdem_dinf.hip ``dim3((unsigned)((tiles + NT - 1) / NT))`` of dinfacc_schedule_kernel."""
    return _ceil(tiles_of(shape), SCHEDULE_NT)


# 258 tiles in a row, the last one partial: the smallest strip with a tile in the second
# workgroup; the same three rows high; 18 x 17 tiles: tiles_x = 17 does not divide 256, tile 256
# is (15, 1) and its eight neighbours lie on both sides of the workgroup boundary
DINF_SHAPES = ((1, 257 * TS + PARTIAL), (3, 257 * TS + PARTIAL), (1093, 1029))
DINF_SEED = 4               # of test_gpu_dinf.random_acyclic_words on the last two


def strip_words(shape, segment=None):
    """The canonical D-infinity words of ``strip_codes``; a word may not point outside the
    raster as a D8 code may, so the last cell is terminal."""
    codes = strip_codes(shape, segment)
    codes.reshape(-1)[-1] = 0
    return dinf.words_from_d8(codes)


# ---------------------------------------------------------------------------
# 7. the newer operators on strips, in closed form
# ---------------------------------------------------------------------------
def _heads_and_ends(n, segment):
    at = np.arange(n, dtype=np.int64)
    head = at // segment * segment if segment else np.zeros(n, np.int64)
    end = np.minimum(head + segment - 1, n - 1) if segment else np.full(n, n - 1, np.int64)
    return at, head, end


def strip_flowsum(shape, q, segment=None):
    """WeightedFlowAccumulation on ``strip_codes``: the prefix sum of ``q`` restarted at every
    segment head, int64."""
    n = shape[0] * shape[1]
    at, head, _ = _heads_and_ends(n, segment)
    prefix = np.concatenate([[0], np.cumsum(np.asarray(q, np.int64).ravel())])
    return (prefix[at + 1] - prefix[head]).reshape(shape)


def strip_pathsum(shape, q, segment=None):
    """FlowPathSum on ``strip_codes`` without streams: the sum of ``q`` from the cell to the
    cell before its segment end (the stop costs nothing), int64; the stop raster is
    ``strip_answer["stop"]``."""
    n = shape[0] * shape[1]
    at, _, end = _heads_and_ends(n, segment)
    prefix = np.concatenate([[0], np.cumsum(np.asarray(q, np.int64).ravel())])
    return (prefix[end] - prefix[at]).reshape(shape)


def _running(words, mode, segment, backwards):
    """The running unsigned minimum / maximum of flat uint64 words inside every segment, from
    the head forwards or from the end backwards."""
    n = words.size
    width = segment or n
    rows = _ceil(n, width)
    padded = np.full(rows * width, IDENTITY[mode], np.uint64)
    padded[:n] = words
    padded = padded.reshape(rows, width)
    best = np.minimum if mode == "min" else np.maximum
    if backwards:
        padded = padded[:, ::-1]
    run = best.accumulate(padded, axis=1)
    if backwards:
        run = run[:, ::-1]
    return np.ascontiguousarray(run).ravel()[:n]


def strip_upextreme(shape, values, mode, segment=None):
    """UpstreamExtreme on ``strip_codes``, (extreme, where): the running extreme from the
    segment head to the cell, with its holder, in the word order of test_upextreme.words_of
    (a NaN is absent, equal values keep the smallest index)."""
    values = np.ascontiguousarray(values)
    run = _running(words_of(values, mode), mode, segment, backwards=False)
    return split_words(run, mode, values.dtype, shape)


def strip_pathextreme(shape, values, mode, segment=None):
    """FlowPathExtreme on ``strip_codes`` without streams, (extreme, where): the running
    extreme from the cell to its segment end, both included."""
    values = np.ascontiguousarray(values)
    run = _running(words_of(values, mode), mode, segment, backwards=True)
    return split_words(run, mode, values.dtype, shape)


def strip_dinf(shape, frac_bits, segment=None):
    """DInfFlowAccumulation on ``strip_words``: the D8 accumulation in units of 2^-frac_bits."""
    return strip_answer(shape, segment)["acc"] << frac_bits


def strip_weights(shape, seed=0):
    """uint32 weights below 2^31 with the bound itself at cell 0."""
    w = np.random.default_rng(seed).integers(0, 2 ** 31, shape, dtype=np.int64).astype(U32)
    w.reshape(-1)[0] = 2 ** 31 - 1
    return w


def strip_values(shape, trend, dtype=np.float32, seed=0):
    """Values along a strip that drift by ``trend`` per eight cells under noise of 30, floored
    to whole numbers (ties), 5 % NaN and some -0.0 for float32: with ``trend`` -1 the running
    minimum from the head keeps changing all the way (and the running maximum from the end),
    with +1 the other two: a new holder in about three tiles of four, held for 80 cells on
    average and 500 at the most, so that a tile's answer comes from up to eight tiles away.
    Against the drift the extreme is found near the far end and carried the whole way."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    v = np.floor(rng.normal(0.0, 30.0, n) + trend * np.arange(n) / 8)
    if np.dtype(dtype) == U32:
        return (v - v.min()).astype(U32).reshape(shape)
    v = v.astype(np.float32)
    v[v == 0] = np.where(rng.random(int((v == 0).sum())) < 0.5, -0.0, 0.0)
    v[rng.random(n) < 0.05] = np.nan
    return v.reshape(shape)
