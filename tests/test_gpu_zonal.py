"""
Zonal statistics on the MI355X (``ZonalStatistics``, ``DemToBasins``,
``hdem_zonal_count_u32[_dev]``, ``hdem_zonal_table_u32[_dev]``, ``hdem_zonal_broadcast_dev``):
every column, K and every counter bit for bit against ``zonal_np`` of tests/test_zonal.py, on
the zone rasters that strain the tiling, the ranks and the per-tile table, with every value
type; against the library's own operators; across the two forms, column subsets and poisoned
memory; and the refusals, each an ordinary error return in bounded time.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, zonal
from test_flowacc import random_acyclic_codes
from test_gpu_scribble import Case, execute
from test_zonal import (COUNTERS, SHAPES, ZONE_KINDS, blobs, float_values, multiples, one_zone,
                        salt_and_pepper, same_bits, same_table, zonal_np)

pytestmark = pytest.mark.gpu

U32 = np.uint32
TABLE_SLOTS = 512           # slots of the tile pass's table: more zones in a tile overflow


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def by_shape(shape):
    return f"{shape[0]}x{shape[1]}"


def check(zones, values=None, frac_bits=16):
    """The host form bit for bit against the NumPy restatement, and the counters."""
    table, stats = zonal.zonal(zones, values, None, frac_bits)
    want, counters = zonal_np(zones, values, frac_bits)
    assert same_table(table, want)
    assert {k: stats[k] for k in COUNTERS} == counters
    assert (stats["tile_h"], stats["tile_w"], stats["capped"]) == (64, 64, 0)
    if values is not None:
        dtype = values.dtype
        assert same_bits(table["mean"], zonal.with_mean(dict(want), dtype, frac_bits)["mean"])
    return table, stats


def with_a_nan_zone(zones, values):
    """``values`` with NaN all over the zone of the first cell that has one."""
    on = np.flatnonzero(zones.ravel())
    if on.size:
        values[zones == zones.ravel()[on[0]]] = np.nan
    return values


# ---------------------------------------------------------------------------
# the zone rasters, each at every shape
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=by_shape)
@pytest.mark.parametrize("kind", list(ZONE_KINDS))
def test_zone_rasters_without_and_with_float_values(kind, shape):
    zones = ZONE_KINDS[kind](shape)
    _, stats = check(zones)
    values = with_a_nan_zone(zones, float_values(shape, shape[0]))
    table, with_values = check(zones, values)
    if kind == "zeros":
        assert stats["zones"] == 0 and all(column.size == 0 for column in table.values())
    if kind == "own" and min(shape[0], 64) * min(shape[1], 64) > TABLE_SLOTS:
        # a tile with more zones than its table has slots: the global path ran
        assert stats["overflow"] > 0 and with_values["overflow"] > 0
    if kind == "one":
        assert table["count"].tolist() == [zones.size] and table["valid"][0] == 0
        assert table["at_min"][0] == table["at_max"][0] == 0xFFFFFFFF


@pytest.mark.parametrize("shape", SHAPES, ids=by_shape)
def test_ids_that_collide_under_a_masking_hash(shape):
    for j in range(13):         # up to the 4 096 slots of the id set
        zones = multiples(shape, j)
        if zones is not None:
            check(zones, float_values(shape, j))


# ---------------------------------------------------------------------------
# the values
# ---------------------------------------------------------------------------
def clamping_values(shape, seed):
    values = float_values(shape, seed)
    rng = np.random.default_rng(seed)
    values[rng.random(shape) < 0.02] = 1e10
    values[rng.random(shape) < 0.02] = -3e9
    values[rng.random(shape) < 0.02] = 40000.0
    values[rng.random(shape) < 0.02] = -2.5
    return values


@pytest.mark.parametrize("shape", [(65, 63), (129, 200)], ids=by_shape)
@pytest.mark.parametrize("frac_bits", [0, 16, 30])
def test_quantised_sums_and_the_cells_that_clamp(frac_bits, shape):
    values = clamping_values(shape, 5)
    for zones in (blobs(shape, 1), one_zone(shape)):
        _, stats = check(zones, values, frac_bits)
        assert stats["clamped"] > 0


@pytest.mark.parametrize("shape", [(64, 64), (129, 200)], ids=by_shape)
def test_uint32_values_need_the_64_bit_sum(shape):
    rng = np.random.default_rng(9)
    values = (U32(0xFFFFFFFF) - rng.integers(0, 5, shape).astype(U32)).astype(U32)
    table, _ = check(one_zone(shape), values)
    assert int(table["sum"][0]) > 2 ** 32 * (shape[0] * shape[1] - 1)
    check(blobs(shape, 2), rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(U32))


@pytest.mark.parametrize("shape", SHAPES, ids=by_shape)
def test_uint8_values(shape):
    values = np.random.default_rng(shape[1]).integers(0, 256, shape).astype(np.uint8)
    for kind in ("one", "salt", "blobs", "own"):
        check(ZONE_KINDS[kind](shape), values)


@pytest.mark.parametrize("shape", [(64, 64), (129, 200)], ids=by_shape)
def test_ties_go_to_the_smallest_index(shape):
    rng = np.random.default_rng(4)
    few = rng.integers(0, 3, shape)
    for zones in (one_zone(shape), salt_and_pepper(shape, 3), blobs(shape, 3)):
        for values in (few.astype(np.float32), few.astype(np.uint8), few.astype(U32)):
            table, _ = check(zones, values)
            flat, labels = values.ravel(), zones.ravel()
            for r in (0, table["id"].size - 1):
                cells = np.flatnonzero(labels == table["id"][r])
                assert table["at_min"][r] == cells[flat[cells] == flat[cells].min()][0]
                assert table["at_max"][r] == cells[flat[cells] == flat[cells].max()][0]


# ---------------------------------------------------------------------------
# against the library's own operators
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrains():
    """D8 codes and the DEM behind them: random acyclic codes (no DEM), and the fill of a
    200 x 333 synthetic raster."""
    z = hdem_synth.synth_dem(200, 333)
    chain = hd.HydroConditioning(epsilon=1e-3)
    return {"random": (random_acyclic_codes(130, 197, seed=11, ramp=True), None),
            "synth": (chain.apply(z), z)}


@pytest.mark.parametrize("terrain", ["random", "synth"])
def test_basin_areas_are_the_accumulation_at_the_outlets(terrains, terrain):
    codes, _ = terrains[terrain]
    labels = hd.Watersheds().apply(codes)
    table = hd.ZonalStatistics().apply(labels)
    acc = hd.FlowAccumulation().apply(codes)
    assert np.array_equal(table["count"], acc.ravel()[table["id"] - 1])
    assert np.array_equal(labels.ravel()[table["id"] - 1], table["id"])     # an outlet labels itself
    assert int(table["count"].sum()) == codes.size


@pytest.mark.parametrize("terrain", ["random", "synth"])
def test_links_and_their_catchments(terrains, terrain):
    codes, _ = terrains[terrain]
    acc = hd.FlowAccumulation().apply(codes)
    network = hd.StreamNetwork(acc, threshold=6)
    row = network.apply(codes)
    assert network.count > 1
    on_links = hd.ZonalStatistics().apply(row)
    assert np.array_equal(on_links["id"], np.arange(1, network.count + 1))
    assert np.array_equal(on_links["count"], network.table["cells"])
    catchments = hd.Watersheds(pour_points=row).apply(codes)
    drained = hd.ZonalStatistics(columns="count").apply(catchments)
    assert np.array_equal(drained["count"], network.table["catchment"])


@pytest.mark.parametrize("terrain", ["noise", "synth"])
def test_depressions_and_their_inventory(terrain):
    rng = np.random.default_rng(2)
    z = hdem_synth.synth_dem(200, 333) if terrain == "synth" else \
        rng.normal(100.0, 30.0, (130, 197)).astype(np.float32)
    inventory = hd.DepressionInventory()
    labels = inventory.apply(z)
    assert inventory.count > 1
    table = hd.ZonalStatistics(inventory.filled).apply(labels)
    assert np.array_equal(table["id"], np.arange(1, inventory.count + 1))
    assert np.array_equal(table["count"], inventory.table["area"])
    assert np.array_equal(table["first"], inventory.table["first"])
    assert same_bits(table["min"], inventory.table["level"])
    assert same_bits(table["max"], inventory.table["level"])     # a filled depression is level


@pytest.mark.parametrize("flats, epsilon", [("keep", 1e-3), ("resolve", 0.0)])
def test_dem_to_basins_is_its_stages_one_by_one(flats, epsilon):
    z = hdem_synth.synth_dem(200, 333)
    codes = hd.HydroConditioning(epsilon=epsilon, flats=flats).apply(z)
    basins = hd.Watersheds(labels="compact")
    labels = basins.apply(codes)
    table = hd.ZonalStatistics(z).apply(labels)
    chain = hd.DemToBasins(epsilon=epsilon, flats=flats)
    got = chain.apply(z)
    assert same_bits(got, labels)
    assert list(chain.table) == list(table) + ["outlet"]
    assert all(same_bits(chain.table[name], table[name]) for name in table)
    assert same_bits(chain.table["outlet"], basins.outlets)
    assert chain.count == basins.stats["basins"] == table["id"].size
    assert set(chain.stats) == {"SinkFill", "Watersheds", "ZonalStatistics"} | (
        {"ResolveFlats"} if flats == "resolve" else set())
    # compact label k is row k - 1, and a basin's lowest cell is no higher than its outlet
    assert np.array_equal(table["id"], np.arange(1, chain.count + 1))
    assert not np.any(table["min"] > z.ravel()[chain.table["outlet"]])


# ---------------------------------------------------------------------------
# forms and memory
# ---------------------------------------------------------------------------
SUBSETS = [("count",), ("id",), ("min",), ("at_max", "id"), ("sum", "valid"),
           ("first", "row_max", "col_min"), ("max", "at_min", "sum")]


@pytest.mark.parametrize("shape", [(64, 64), (65, 63), (129, 200)], ids=by_shape)
def test_forms_repeats_and_column_subsets_agree(shape):
    zones, values = blobs(shape, 6), float_values(shape, 6)
    full, stats = zonal.zonal(zones, values)
    with backend.DeviceRaster.from_host(zones) as dz, backend.DeviceRaster.from_host(values) as dv:
        for _ in range(2):
            on_device, device_stats = zonal.zonal_dev(dz, dv)
            assert list(on_device) == list(full)
            assert all(same_bits(on_device[name], full[name]) for name in full)
            assert {k: device_stats[k] for k in COUNTERS} == {k: stats[k] for k in COUNTERS}
        for subset in SUBSETS:
            for table, _ in (zonal.zonal(zones, values, subset), zonal.zonal_dev(dz, dv, subset)):
                assert set(table) - {"mean"} == set(subset)
                assert all(same_bits(table[name], full[name]) for name in subset)
    again, _ = zonal.zonal(zones, values)
    assert all(same_bits(again[name], full[name]) for name in full)
    operator = hd.ZonalStatistics(values, frac_bits=16)
    assert all(same_bits(operator.apply(zones)[name], full[name]) for name in full)
    assert operator.stats["zones"] == full["id"].size


def broadcast_np(zones, ids, column, fill):
    rows = np.searchsorted(ids, zones)
    rows[zones == 0] = 0
    picked = column[rows] if column.size else np.zeros(zones.shape, column.dtype)
    return np.where(zones == 0, np.array(fill).astype(column.dtype), picked)


@pytest.mark.parametrize("shape", SHAPES, ids=by_shape)
def test_broadcast_is_a_lookup_by_rank(shape):
    zones, values = blobs(shape, 8), float_values(shape, 8)
    operator = hd.ZonalStatistics(values)
    table = operator.apply(zones)
    ids = table["id"]
    assert same_bits(operator.broadcast("count", 7), broadcast_np(zones, ids, table["count"], 7))
    assert same_bits(operator.broadcast("min", -1.5), broadcast_np(zones, ids, table["min"], -1.5))
    ranks = np.arange(ids.size, dtype=U32)
    assert same_bits(operator.broadcast(ranks, 0xFFFFFFFF),
                     broadcast_np(zones, ids, ranks, 0xFFFFFFFF))
    with backend.DeviceRaster.from_host(zones) as dz:
        operator.apply_device(dz)
        with operator.broadcast("at_max") as raster:
            assert backend.is_device_raster(raster)
            assert same_bits(raster.to_host(), broadcast_np(zones, ids, table["at_max"], 0))
    with pytest.raises(ValueError, match="4-byte"):
        operator.broadcast("sum")
    with pytest.raises(ValueError, match="one entry per zone"):
        operator.broadcast(np.zeros(ids.size + 1, U32))
    empty = hd.ZonalStatistics()
    assert empty.apply(np.zeros(shape, U32))["id"].size == 0
    assert same_bits(empty.broadcast("count", 3), np.full(shape, 3, U32))


def poison_inputs(shape, seed=12):
    zones = blobs(shape, seed)
    zones[:40, :50] = np.arange(1, 2001, dtype=U32).reshape(40, 50)     # a tile past its table
    return {"zones": zones, "values": float_values(shape, seed)}


def poison_run(call, inp):
    """Count, table and broadcast of device rasters."""
    dz, dv = call.up(inp["zones"]), call.up(inp["values"])
    count, count_stats = zonal.zonal_count_dev(dz)
    table, stats = zonal.zonal_dev(dz, dv)
    table["raster"] = call.host(zonal.zonal_broadcast_dev(dz, table["count"], 0xABCD))
    assert count == stats["zones"] == count_stats["zones"]
    return table, {k: stats[k] for k in COUNTERS}


def poison_check(inp, got):
    assert same_table({k: v for k, v in got.items() if k != "raster"},
                      zonal_np(inp["zones"], inp["values"])[0])


POISON_SHAPES = [(130, 197), (64, 64)]
POISON_CASE = Case("zonal-count-table-broadcast", tuple(POISON_SHAPES), poison_inputs, poison_run,
                   poison_check, False, frozenset())


@pytest.mark.parametrize("shape", POISON_SHAPES, ids=by_shape)
def test_poisoned_memory_changes_nothing(shape):
    inp = POISON_CASE.build(shape)
    want, counters = execute(POISON_CASE, inp, None, False)
    POISON_CASE.check(inp, want)
    for byte in (0x00, 0xFF, 0x7F, 0x01):       # 0x00 first: the most forgiving poison
        got, got_counters = execute(POISON_CASE, inp, byte, False)
        assert list(got) == list(want) and got_counters == counters, hex(byte)
        for name in want:
            assert same_bits(got[name], want[name]), (hex(byte), name)


# ---------------------------------------------------------------------------
# refusals: an error return in bounded time, then a good call on the same context
# ---------------------------------------------------------------------------
def test_an_id_past_the_raster_is_refused_and_counted():
    shape = (65, 63)
    zones = blobs(shape, 1)
    good = zones.copy()
    zones[3, 5] = zones[64, 62] = shape[0] * shape[1] + 1
    zones[10, 10] = 0xFFFFFFF0
    for call in (lambda: zonal.zonal(zones), lambda: zonal.zonal_count(zones),
                 lambda: hd.ZonalStatistics().apply(zones)):
        with pytest.raises(ValueError, match=r"4095: 3 cells hold a larger id.*4294967280"):
            call()
    with backend.DeviceRaster.from_host(zones) as dz:
        with pytest.raises(ValueError, match="3 cells hold a larger id"):
            zonal.zonal_dev(dz)
        with pytest.raises(ValueError, match="3 cells hold a larger id"):
            zonal.zonal_broadcast_dev(dz, np.zeros(4, U32))
    check(good)


GUARD, PAD = 0x5A5A5A5A, 64


@pytest.mark.parametrize("off_by", [-1, 1, 7])
def test_a_wrong_count_is_refused_and_writes_nothing_outside_the_columns(off_by):
    shape = (129, 200)
    zones, values = blobs(shape, 3), float_values(shape, 3)
    true_count, _ = zonal.zonal_count(zones)
    given = true_count + off_by
    names = zonal.ZONAL_COLUMNS
    # one block of 8-byte words: a guard, then for every column room for `given` entries and a guard
    words = PAD + len(names) * (given + PAD)
    block = np.full(2 * words, GUARD, U32)
    ctx = backend.context()
    with backend.DeviceRaster.from_host(zones) as dz, backend.DeviceRaster.from_host(values) as dv, \
            backend.DeviceRaster.from_host(block.reshape(1, -1)) as guarded:
        offsets = [guarded.ptr + 8 * (PAD + k * (given + PAD)) for k in range(len(names))]
        stats = backend._ZonalStats()
        rc = ctx.lib.hdem_zonal_table_u32_dev(ctx.handle, dz.ptr, *shape, dv.ptr, 1, 16, given,
                                              *offsets, 0, ctypes.byref(stats))
        assert rc == backend.BAD_ARG
        message = ctx.lib.hdem_last_error().decode()
        assert f"K = {given}" in message and f"holds {true_count}" in message
        assert stats.zones == true_count
        after = guarded.to_host().ravel()
    untouched = np.ones(words, bool)
    sizes = {name: zonal.column_dtype(name, np.float32).itemsize for name in names}
    for k, name in enumerate(names):
        start = PAD + k * (given + PAD)
        untouched[start:start + (given * sizes[name] + 7) // 8] = False
    assert np.all(after.view(np.uint64)[untouched] == np.uint64(GUARD * (2 ** 32 + 1)))
    check(zones, values)


def test_values_of_another_shape_are_refused_before_the_device():
    zones = blobs((65, 63), 1)
    with pytest.raises(ValueError, match="the zones"):
        zonal.zonal(zones, np.zeros((63, 65), np.float32))
    with backend.DeviceRaster.from_host(np.zeros((63, 65), np.float32)) as dv:
        with pytest.raises(ValueError, match="the zones"):
            hd.ZonalStatistics(dv).apply(zones)
    check(zones, float_values((65, 63), 1))


def test_the_c_calls_refuse_bad_arguments():
    ctx = backend.context()
    zones = blobs((8, 9), 1)
    count, _ = zonal.zonal_count(zones)
    out = np.zeros(count, U32)
    stats = backend._ZonalStats()
    table = lambda **kw: ctx.lib.hdem_zonal_table_u32(          # noqa: E731
        ctx.handle, zones.ctypes.data, 8, 9, kw.get("values"), kw.get("value_type", 0),
        kw.get("frac_bits", 16), kw.get("count", count), None, kw.get("out", out.ctypes.data),
        *[None] * 6, kw.get("min"), *[None] * 4, kw.get("flags", 0), ctypes.byref(stats))
    assert table() == backend.OK and int(out.sum()) == int((zones > 0).sum())
    values = np.zeros((8, 9), np.float32)
    for bad in ({"flags": 1}, {"value_type": 4, "values": values.ctypes.data}, {"value_type": 1},
                {"values": values.ctypes.data}, {"frac_bits": 31}, {"count": -1}, {"count": 73},
                {"min": out.ctypes.data}, {"out": None}):
        assert table(**bad) == backend.BAD_ARG, bad
    assert table() == backend.OK
