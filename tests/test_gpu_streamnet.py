"""
The stream network as a table on the MI355X (``StreamNetwork``, ``DemToStreamNetwork``,
``hdem_streamlinks_u8[_dev]``): every column, the ``row`` raster and every counter bit for bit
against ``table_np`` of tests/test_streamnet.py, on random acyclic codes with the three forms of
the stream set, on constructed networks with known tables (links that span many tiles), on the
network of a real fill, against ``Watersheds``, ``FlowDistance`` and the flow accumulation,
column by column, across the two forms and under poisoned memory, and the refusals, each an
ordinary error return in bounded time.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, streamnet, streamorder
from test_flowacc import acc_kahn, random_acyclic_codes
from test_gpu_scribble import Case, execute
from test_streamnet import (COLUMNS, COUNTERS, accumulate_down, constructed, holds_known,
                            invariants_hold, random_dem, same_table, table_np)
from test_streamorder import stream_of

pytestmark = pytest.mark.gpu

NAMES = tuple(n for n, _ in COLUMNS)
CELL = 12.5


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def links_of(codes, streams=None, threshold=None):
    """The stream order's three rasters and its count of links."""
    outs, stats = streamorder.streamorder(np.ascontiguousarray(codes, dtype=np.uint8), streams,
                                          threshold, ("order", "magnitude", "link"))
    return outs, stats["links"]


def run(codes, streams=None, threshold=None, dem=None, cellsize=1.0, columns=None, row=True,
        of=None):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    outs, count = of or links_of(codes, streams, threshold)
    return streamnet.streamlinks(codes, outs["link"], count, streams, threshold, outs["order"],
                                 outs["magnitude"], dem, cellsize, columns, row)


def check(got, codes, stream, dem=None, cellsize=1.0):
    """Bit for bit against the NumPy grouping, and the counters."""
    table, row, stats = got
    want, want_row, counters = table_np(codes, stream, dem, cellsize)
    assert list(table) == [n for n in NAMES if n in want]
    assert all(table[n].dtype == dict(COLUMNS)[n] for n in table)
    assert same_table(table, want)
    assert row.dtype == np.uint32 and np.array_equal(row, want_row)
    assert {k: stats[k] for k in COUNTERS} == counters
    assert stats["tile_h"] == 64 and stats["tile_w"] == 64
    return want, counters


# ---------------------------------------------------------------------------
# random acyclic codes, the three forms of the stream set
# ---------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 130), (130, 1), (64, 64), (65, 63), (70, 90), (129, 200), (257, 130)]


@pytest.fixture(scope="module")
def cases():
    """Codes, their accumulation and a dem with some NaN per (shape, ramp), made once."""
    made = {}

    def get(shape, ramp):
        if (shape, ramp) not in made:
            codes = random_acyclic_codes(*shape, seed=shape[0] * 1000 + shape[1], ramp=ramp)
            made[shape, ramp] = (codes, acc_kahn(codes).astype(np.uint32),
                                 random_dem(shape, shape[0] + shape[1]))
        return made[shape, ramp]
    return get


def stream_form(kind, shape, acc):
    if kind == "all":
        return None, None
    if kind == "acc":
        return acc, 4
    return np.random.default_rng(shape[1]).random(shape) < 0.6, None


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ramp", [False, True], ids=["flat", "ramp"])
@pytest.mark.parametrize("kind", ["all", "acc", "mask"])
def test_random_acyclic_codes_match_the_numpy_grouping(cases, shape, ramp, kind):
    codes, acc, dem = cases(shape, ramp)
    streams, threshold = stream_form(kind, shape, acc)
    got = run(codes, streams, threshold, dem, CELL)
    check(got, codes, stream_of(codes, streams, threshold), dem, CELL)


# ---------------------------------------------------------------------------
# constructed networks: links that span tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _, _ in constructed()])
def test_constructed_networks_have_their_known_tables(name):
    codes, stream = next((c, s) for n, c, s in constructed() if n == name)
    dem = random_dem(codes.shape, 3)
    got = run(codes, None if stream.all() else stream, None, dem, 30.0)
    want, counters = check(got, codes, stream, dem, 30.0)
    assert holds_known(name, got[0]) and invariants_hold(codes, stream, got[0], counters)
    if name == "serpentine":
        assert got[0]["length"][0] == np.float32(25799 * 30.0) and want["cells"][0] == 25800


# ---------------------------------------------------------------------------
# a real network
# ---------------------------------------------------------------------------
def test_the_chain_from_a_dem_matches_the_grouping_of_its_own_codes():
    z = hdem_synth.synth_dem(512, 512)
    chain = hd.DemToStreamNetwork(100, cellsize=30.0)
    row = chain.apply(z)
    parts = hd.DemToStreamOrder(threshold=100, keep_partial_results=True)
    parts.apply(z)
    conditioning = hd.HydroConditioning(epsilon=chain.filters[0].epsilon)
    assert np.array_equal(conditioning.apply(z), parts.codes)
    stream = parts.accumulation >= 100
    want, want_row, counters = table_np(parts.codes, stream, conditioning.filled, 30.0)
    assert same_table(chain.table, want) and np.array_equal(row, want_row)
    assert chain.count == counters["links"] > 100
    st = chain.stats["StreamNetwork"]
    assert {k: st[k] for k in COUNTERS} == counters
    assert st["order_stats"] == chain.stats["StreamNetwork"]["order_stats"]
    assert st["order_stats"]["links"] == chain.count
    assert set(chain.stats) == {"SinkFill", "FlowAccumulation", "StreamNetwork"}
    assert invariants_hold(parts.codes, stream, chain.table, counters)
    # the filled dem descends along the D8 paths
    assert (chain.table["z_top"] >= chain.table["z_end"]).all()
    assert int(chain.table["order"].max()) >= 3 and int(chain.table["cells"].max()) > 64
    total = accumulate_down(chain.table["down"], chain.table["catchment"])
    assert np.array_equal(total, parts.accumulation.ravel()[chain.table["end"]])
    # the two-step calls on the same rasters, and the device form of the chain
    two = run(parts.codes, parts.accumulation, 100, conditioning.filled, 30.0)
    assert same_table(two[0], chain.table) and np.array_equal(two[1], row)
    with backend.DeviceRaster.from_host(z) as dz:
        with chain.apply_device(dz) as out:
            assert backend.is_device_raster(out) and np.array_equal(out.to_host(), row)
    assert same_table(chain.table, want)
    resolved = hd.DemToStreamNetwork(100, epsilon=0.0, flats="resolve", columns=("cells", "down"))
    resolved.apply(z)
    assert list(resolved.table) == ["down", "cells"] and "ResolveFlats" in resolved.stats


# ---------------------------------------------------------------------------
# against the existing operators
# ---------------------------------------------------------------------------
def test_catchments_agree_with_watersheds_flow_distance_and_accumulation(cases):
    shape = (257, 130)
    codes, acc, _ = cases(shape, True)
    for kind in ("acc", "mask", "all"):
        streams, threshold = stream_form(kind, shape, acc)
        outs, count = links_of(codes, streams, threshold)
        table, row, stats = run(codes, streams, threshold, of=(outs, count))
        # the catchment Watersheds draws for every link, regrouped by row
        labels = hd.Watersheds(pour_points=outs["link"]).apply(codes)
        row_of = np.zeros(codes.size + 1, np.int64)
        row_of[table["end"].astype(np.int64) + 1] = np.arange(count) + 1
        area = np.bincount(row_of[labels.ravel()], minlength=count + 1)
        assert np.array_equal(area[1:], table["catchment"])
        # ... and with the compact ids as pour points the labels index the table
        compact = hd.Watersheds(pour_points=row).apply(codes)
        assert np.array_equal(np.bincount(compact.ravel(), minlength=count + 1)[1:],
                              table["catchment"])
        if kind != "all":
            stream = stream_of(codes, streams, threshold)
            distance = hd.FlowDistance(stream).apply(codes)
            assert int(table["catchment"].sum()) == int((~np.isnan(distance)).sum()) == \
                stats["catchment_cells"]
        if kind != "mask":
            total = accumulate_down(table["down"], table["catchment"])
            assert np.array_equal(total, acc.ravel()[table["end"]])


# ---------------------------------------------------------------------------
# column subsets
# ---------------------------------------------------------------------------
def test_every_column_alone_and_no_trace_without_catchment(cases):
    shape = (70, 90)
    codes, acc, dem = cases(shape, True)
    of = links_of(codes, acc, 4)
    whole, whole_row, _ = run(codes, acc, 4, dem, CELL, of=of)
    assert list(whole) == list(NAMES)
    ctx = backend.context()
    ctx.profile(True)
    try:
        for name in NAMES:
            table, row, stats = run(codes, acc, 4, dem, CELL, columns=(name,), row=False, of=of)
            assert list(table) == [name] and row is None
            assert table[name].tobytes() == whole[name].tobytes(), name
            # the flow trace runs for catchment and for nothing else
            assert (stats["ms_trace"] > 0) == (name == "catchment"), name
            assert (stats["catchment_cells"] > 0) == (name == "catchment"), name
            assert stats["ms_rank"] > 0 and stats["ms_tile"] > 0
        table, row, stats = run(codes, acc, 4, columns=(), of=of)
        assert table == {} and np.array_equal(row, whole_row) and stats["ms_trace"] == 0
        rest = tuple(n for n in NAMES if n != "catchment")
        table, _, stats = run(codes, acc, 4, dem, CELL, columns=rest, of=of)
        assert stats["ms_trace"] == 0 and same_table(table, {n: whole[n] for n in rest})
        # every cell a stream cell: each is its own first stream cell, nothing to trace
        table, _, stats = run(codes, columns=("catchment", "cells"))
        assert stats["ms_trace"] == 0 and np.array_equal(table["catchment"], table["cells"])
        assert stats["catchment_cells"] == codes.size
    finally:
        ctx.profile(False)
    assert run(codes, acc, 4, of=of)[2]["ms_rank"] == 0
    # without the rasters and the dem the default is what is left
    table, _, _ = streamnet.streamlinks(codes, of[0]["link"], of[1], acc, 4, cellsize=CELL)
    assert list(table) == [n for n in NAMES if n not in ("order", "magnitude", "z_top", "z_end")]
    assert same_table(table, {n: whole[n] for n in table})


# ---------------------------------------------------------------------------
# the two forms, two runs, poisoned memory
# ---------------------------------------------------------------------------
def on_device(ctx, codes, acc, dem, threshold=4):
    """The device form on ``ctx``: the table, the row raster and the stats as host data."""
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8, ctx=ctx) as dc, \
            backend.DeviceRaster.from_host(acc, dtype=np.uint32, ctx=ctx) as dacc, \
            backend.DeviceRaster.from_host(dem, dtype=np.float32, ctx=ctx) as ddem:
        outs, st = streamorder.streamorder_dev(dc, dacc, threshold, ("order", "magnitude", "link"))
        with outs["order"], outs["magnitude"], outs["link"]:
            table, row, stats = streamnet.streamlinks_dev(
                dc, outs["link"], st["links"], dacc, threshold, outs["order"], outs["magnitude"],
                ddem, CELL, None, True)
            with row:
                assert backend.is_device_raster(row) and row.dtype == np.uint32
                return table, row.to_host(), {k: stats[k] for k in COUNTERS}


def test_host_form_device_form_and_two_runs_are_identical(cases):
    codes, acc, dem = cases((257, 130), True)
    a = run(codes, acc, 4, dem, CELL)
    check(a, codes, acc >= 4, dem, CELL)
    b = run(codes, acc, 4, dem, CELL)
    c = on_device(backend.context(), codes, acc, dem)
    for other in (b, c):
        assert same_table(a[0], other[0]) and np.array_equal(a[1], other[1])
        assert {k: a[2][k] for k in COUNTERS} == {k: other[2][k] for k in COUNTERS}
    assert all(isinstance(v, np.ndarray) for v in c[0].values())


def poison_inputs(shape, seed=None):
    """What the ``cases`` fixture makes for (shape, ramp=True)."""
    codes = random_acyclic_codes(*shape, seed=shape[0] * 1000 + shape[1], ramp=True)
    return {"codes": codes, "acc": acc_kahn(codes).astype(np.uint32),
            "dem": random_dem(shape, shape[0] + shape[1])}


def poison_run(call, inp, threshold=4):
    """The stream order's three rasters, then the table and the row raster from them."""
    dc, dacc, ddem = call.up(inp["codes"]), call.up(inp["acc"]), call.up(inp["dem"])
    outs, st = streamorder.streamorder_dev(dc, dacc, threshold, ("order", "magnitude", "link"))
    for raster in outs.values():
        call.stack.enter_context(raster)
    table, row, stats = streamnet.streamlinks_dev(
        dc, outs["link"], st["links"], dacc, threshold, outs["order"], outs["magnitude"],
        ddem, CELL, None, True)
    assert backend.is_device_raster(row) and row.dtype == np.uint32
    assert "row" not in table
    return dict(table, row=call.host(row)), {k: stats[k] for k in COUNTERS}


def poison_check(inp, got):
    want, want_row, _ = table_np(inp["codes"], inp["acc"] >= 4, inp["dem"], CELL)
    assert same_table({k: v for k, v in got.items() if k != "row"}, want)
    assert np.array_equal(got["row"], want_row)


POISON_CASE = Case("streamnet-table-and-row", ((129, 200), (130, 197)), poison_inputs, poison_run,
                   poison_check, False, frozenset())


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x7F])
def test_poisoned_memory_changes_nothing(cases, byte):
    codes, acc, dem = cases((129, 200), True)
    want = run(codes, acc, 4, dem, CELL)
    got, counters = execute(POISON_CASE, {"codes": codes, "acc": acc, "dem": dem}, byte, False)
    row = got.pop("row")
    assert same_table(got, want[0]) and np.array_equal(row, want[1])
    assert counters == {k: want[2][k] for k in COUNTERS}


# ---------------------------------------------------------------------------
# K == 0
# ---------------------------------------------------------------------------
def test_no_link_at_all():
    codes = random_acyclic_codes(70, 90, seed=1, ramp=True)
    mask = np.zeros(codes.shape, bool)
    outs, count = links_of(codes, mask)
    assert count == 0 and not outs["link"].any()
    table, row, stats = run(codes, mask, of=(outs, count))
    assert list(table) == [n for n in NAMES if not n.startswith("z_")]
    assert all(v.shape == (0,) for v in table.values())
    assert row.shape == codes.shape and not row.any() and stats["links"] == 0
    f = hd.StreamNetwork(mask)
    assert not f.apply(codes).any() and f.count == 0 and f.table["end"].shape == (0,)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        with f.apply_device(dc) as out:
            assert not out.to_host().any()


# ---------------------------------------------------------------------------
# the operators against the two-step calls
# ---------------------------------------------------------------------------
def test_the_operator_equals_the_two_step_calls(cases):
    codes, acc, dem = cases((129, 200), False)
    want = run(codes, acc, 4, dem, CELL)
    f = hd.StreamNetwork(acc, threshold=4, dem=dem, cellsize=CELL, keep_partial_results=True)
    row = f.apply(codes)
    assert np.array_equal(row, want[1]) and same_table(f.table, want[0])
    assert f.count == want[2]["links"] == f.stats["order_stats"]["links"]
    assert {k: f.stats[k] for k in COUNTERS} == {k: want[2][k] for k in COUNTERS}
    outs, _ = links_of(codes, acc, 4)
    assert np.array_equal(f.order, outs["order"]) and np.array_equal(f.magnitude, outs["magnitude"])
    assert np.array_equal(f.links, outs["link"]) and isinstance(f.links, np.ndarray)
    g = hd.StreamNetwork(acc >= 4, columns=("cells", "length"), cellsize=CELL)
    assert np.array_equal(g.apply(codes), row) and list(g.table) == ["cells", "length"]
    assert g.order is None and g.links is None
    assert same_table(g.table, {n: want[0][n] for n in ("cells", "length")})
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(dem, dtype=np.float32) as ddem:
        dev = hd.StreamNetwork(acc, threshold=4, dem=ddem, cellsize=CELL,
                               keep_partial_results=True)
        out = dev.apply_device(dc)
        # the rasters handed out are the caller's to free
        with out, dev.order, dev.magnitude, dev.links:
            assert all(backend.is_device_raster(r) for r in (out, dev.order, dev.links))
            assert np.array_equal(out.to_host(), row)
            assert np.array_equal(dev.links.to_host(), outs["link"])
        assert same_table(dev.table, want[0])
        plain = hd.StreamNetwork(acc, threshold=4)
        with plain.apply_device(dc) as out:
            assert np.array_equal(out.to_host(), row) and plain.links is None
        assert list(plain.table) == [n for n in NAMES if not n.startswith("z_")]


# ---------------------------------------------------------------------------
# refusals: each returns, and the context stays usable
# ---------------------------------------------------------------------------
def still_works():
    table, row, _ = run(np.full((3, 5), 4, np.uint8))
    assert table["cells"].tolist() == [3] * 5 and table["end"].tolist() == [10, 11, 12, 13, 14]
    assert np.array_equal(row, np.tile(np.arange(1, 6, dtype=np.uint32), (3, 1)))


def test_links_of_other_codes_or_streams_and_a_wrong_count_are_refused(cases):
    shape = (129, 200)
    codes, acc, dem = cases(shape, True)
    outs, count = links_of(codes, acc, 4)
    says = "the links do not belong to these codes and streams"
    other = random_acyclic_codes(*shape, seed=77, ramp=True)
    with pytest.raises(ValueError, match=says):
        run(other, acc, 4, dem, of=(outs, count))
    still_works()
    for streams, threshold in ((acc, 8), (acc, 2), (None, None),
                               (np.random.default_rng(1).random(shape) < 0.6, None)):
        with pytest.raises(ValueError, match=says):
            run(codes, streams, threshold, dem, of=(outs, count))
    still_works()
    for wrong in (count - 1, count + 1, 1):
        with pytest.raises(ValueError, match=says):
            run(codes, acc, 4, dem, of=(outs, wrong))
    still_works()
    # one link id moved to its neighbour's, one erased, one set off the streams
    stream = acc >= 4
    on = np.argwhere(stream)
    for how in ("moved", "erased", "foreign"):
        link = outs["link"].copy()
        y, x = on[len(on) // 2]
        if how == "moved":
            link[y, x] = link[stream][0] if link[y, x] != link[stream][0] else link[stream][-1]
        elif how == "erased":
            link[y, x] = 0
        else:
            y, x = np.argwhere(~stream)[7]
            link[y, x] = link[stream][0]
        with pytest.raises(ValueError, match=says):
            run(codes, acc, 4, of=(dict(outs, link=link), count))
    still_works()
    check(run(codes, acc, 4, dem, of=(outs, count)), codes, stream, dem)


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(cases, bad):
    codes, acc, _ = cases((70, 90), True)
    of = links_of(codes, acc, 4)
    wrong = codes.copy()
    wrong[20, 33] = bad
    for columns in (None, ("cells",)):
        with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
            run(wrong, acc, 4, columns=columns, of=of)
    still_works()


def test_argument_combinations_are_refused_by_the_library():
    ctx = backend.context()
    lib = ctx.lib
    codes = np.full((4, 6), 1, np.uint8)
    link = np.tile(np.arange(6, 25, 6, dtype=np.uint32)[:, None], (1, 6))
    out = np.zeros(4, np.uint32)
    raster = np.zeros((4, 6), np.uint32)
    st = backend._StreamLinksStats()                # pylint: disable=protected-access
    head = (ctx.handle, codes.ctypes.data, 4, 6)
    none = (None, backend.FT_STREAMS_NONE, 0)
    operands = (link.ctypes.data, None, None, None)

    def call(fn, streams=none, given=operands, cellsize=1.0, count=4, columns=None, row=None,
             flags=0, stats=None):
        cols = [None] * 12
        for k, v in (columns or {5: out.ctypes.data}).items():
            cols[k] = v
        return fn(*head, *streams, *given, cellsize, count, *cols, row, flags, stats)

    for fn in (lib.hdem_streamlinks_u8, lib.hdem_streamlinks_u8_dev):
        assert call(fn, columns={0: None}) == backend.BAD_ARG
        assert b"no output wanted" in lib.hdem_last_error()
        assert call(fn, flags=1) == backend.BAD_ARG and b"flags" in lib.hdem_last_error()
    fn = lib.hdem_streamlinks_u8
    for cellsize in (0.0, -1.0, float("nan"), float("inf")):
        assert call(fn, cellsize=cellsize) == backend.BAD_ARG
        assert b"cellsize" in lib.hdem_last_error()
    assert call(fn, given=(None, None, None, None)) == backend.BAD_ARG
    assert b"link raster is null" in lib.hdem_last_error()
    for k, says in ((10, b"z_top and z_end need the dem"), (11, b"z_top and z_end need the dem"),
                    (3, b"order column needs the order raster"),
                    (4, b"magnitude column needs the magnitude raster")):
        assert call(fn, columns={k: out.ctypes.data}) == backend.BAD_ARG
        assert says in lib.hdem_last_error()
    for count in (-1, 25):
        assert call(fn, count=count) == backend.BAD_ARG and b"K is" in lib.hdem_last_error()
    for streams, says in (((codes.ctypes.data, 0, 0), b"must be null"),
                          ((None, 1, 0), b"mask is null"),
                          ((codes.ctypes.data, 1, 2), b"no threshold"),
                          ((codes.ctypes.data, 2, 0), b"threshold >= 1"),
                          ((None, 7, 0), b"unknown stream kind")):
        assert call(fn, streams=streams) == backend.BAD_ARG and says in lib.hdem_last_error()
    st.struct_size = 3
    assert call(fn, stats=ctypes.byref(st)) == backend.BAD_ARG
    assert b"hdem_streamlinks_stats.struct_size is 3" in lib.hdem_last_error()
    # a shorter struct is filled as far as it goes
    st = backend._StreamLinksStats()                # pylint: disable=protected-access
    st.struct_size, st.tops = 32, -7
    assert call(fn, row=raster.ctypes.data, stats=ctypes.byref(st)) == backend.OK
    assert st.struct_size == 32 and st.links == 4 and st.stream_cells == 24 and st.tops == -7
    assert out.tolist() == [6] * 4 and np.array_equal(raster[:, 0], [1, 2, 3, 4])
    still_works()


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_streamlinks_u8_dev, ctx.lib.hdem_streamlinks_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, None, 0, 0, fake, None, None, None, 1.0, 5,
                *[fake if k == 5 else None for k in range(12)], None, 0, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    still_works()
