"""
Depression labelling and inventory on the GPU (``Depressions``, ``DepressionInventory``,
``hdem_depressions_f32[_dev]``, ``hdem_depression_table_f32[_dev]``).

The definition and the references are those of tests/test_depressions.py; every comparison is
``np.array_equal``.  ``check`` runs the host form and the device form, compact labels with
the table and ``labels="first"``, against the reference.  Masks go in as ``dem = 0, filled =
mask``.  Hand grids inside one tile, the seams of a 130 x 130 raster cell by cell, long chains
of tiles (corridors, a serpentine, a U, the spiral corridor), random masks at the percolation
threshold in every tile geometry, fills made by the library itself, the depth quantum, and
the errors.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from test_depressions import COLUMNS, first_labels, mask_pair, reference
from test_gpu_flats import spiral_corridor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def assert_table(got, want):
    for name in COLUMNS + ("volume",):
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name], want[name]), name


def check(dem, filled, cellsize=1.0):
    """Host and device form, both label modes and the table against the reference; returns
    (compact labels, K, table, stats)."""
    dem = np.ascontiguousarray(dem, dtype=np.float32)
    filled = np.ascontiguousarray(filled, dtype=np.float32)
    want, count, table = reference(dem, filled, cellsize)
    want_first = first_labels(want, table["first"])
    with np.errstate(invalid="ignore"):
        raised = int((filled > dem).sum())

    op = hd.Depressions(dem=dem, table=True, cellsize=cellsize)
    got = op.apply(filled)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert op.count == count == op.stats["depressions"]
    assert op.stats["raised_cells"] == raised
    assert count <= op.stats["tile_components"] <= raised
    assert op.stats["tile_h"] == op.stats["tile_w"] == 64
    assert_table(op.table, table)
    by_first = hd.Depressions(dem=dem, labels="first")
    assert np.array_equal(by_first.apply(filled), want_first)
    assert by_first.count == count and by_first.table is None
    stats = op.stats

    with backend.DeviceRaster.from_host(filled) as on_device, \
            backend.DeviceRaster.from_host(dem) as dem_on_device:
        op = hd.Depressions(dem=dem_on_device, table=True, cellsize=cellsize)
        with op.apply_device(on_device) as out:
            assert out.dtype == np.uint32 and np.array_equal(out.to_host(), want)
        assert op.count == count
        assert_table(op.table, table)
        assert {k: v for k, v in op.stats.items() if not k.startswith("ms_")} == \
            {k: v for k, v in stats.items() if not k.startswith("ms_")}
        with hd.Depressions(dem=dem, labels="first").apply_device(on_device) as out:
            assert np.array_equal(out.to_host(), want_first)
        assert np.array_equal(on_device.to_host(), filled, equal_nan=True)    # operands untouched
        assert np.array_equal(dem_on_device.to_host(), dem, equal_nan=True)
    return want, count, table, stats


def check_mask(mask):
    return check(*mask_pair(mask))


# ---------------------------------------------------------------------------
# inside one tile
# ---------------------------------------------------------------------------
def test_the_hand_grid_with_its_answers_written_out():
    from test_depressions import HAND, HAND_DEM, HAND_FILLED, HAND_TABLE
    labels, count, table, stats = check(HAND_DEM, HAND_FILLED, cellsize=30.0)
    assert count == 5 and np.array_equal(labels, HAND)
    assert table["area"].tolist() == HAND_TABLE["area"]
    assert stats["tile_components"] == 5


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1)])
def test_rasters_one_cell_wide(shape):
    _, count, _, _ = check_mask(np.ones(shape, bool))
    assert count == 1
    every_other = np.zeros(shape, bool)
    every_other.flat[::2] = True
    _, count, _, _ = check_mask(every_other)
    assert count == (max(shape) + 1) // 2


def test_a_tile_that_is_all_raised_and_a_raster_with_nothing_raised():
    labels, count, table, stats = check_mask(np.ones((64, 64), bool))
    assert count == 1 and table["area"].tolist() == [4096] and labels.min() == 1
    assert stats["tile_components"] == 1
    _, count, table, stats = check_mask(np.zeros((70, 90), bool))
    assert count == 0 and stats["raised_cells"] == 0
    assert all(len(table[name]) == 0 for name in COLUMNS)


# ---------------------------------------------------------------------------
# the seams of a 130 x 130 raster
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [((63, 63), (64, 64)), ((63, 64), (64, 63))],
                         ids=["diagonal", "antidiagonal"])
def test_two_cells_that_meet_at_the_corner_of_four_tiles(cells):
    mask = np.zeros((130, 130), bool)
    for cell in cells:
        mask[cell] = True
    labels, count, table, stats = check_mask(mask)
    assert count == 1 and stats["tile_components"] == 2
    assert table["first"].tolist() == [cells[0][0] * 130 + cells[0][1]]


def test_a_checkerboard_is_one_depression_and_isolated_cells_are_their_own():
    yy, xx = np.indices((130, 130))
    _, count, table, stats = check_mask((yy + xx) % 2 == 0)
    assert count == 1 and table["area"].tolist() == [8450]
    yy, xx = np.indices((130, 131))
    labels, count, table, _ = check_mask((yy % 2 == 0) & (xx % 2 == 0))
    assert count == 65 * 66 == 4290
    assert np.array_equal(table["area"], np.ones(4290, np.uint32))


# ---------------------------------------------------------------------------
# long chains of tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("upright", [False, True])
def test_a_corridor_across_64_tiles(upright):
    mask = np.zeros((5, 4097), bool)
    mask[2, 1:] = True
    _, count, table, stats = check_mask(mask.T if upright else mask)
    assert count == 1 and table["area"].tolist() == [4096]
    assert stats["tile_components"] == 65


def serpentine(tiles=5):
    n = 64 * tiles
    mask = np.zeros((n, n), bool)
    for r in range(tiles):
        y = 64 * r + 32
        mask[y, 2:n - 2] = True
        if r + 1 < tiles:
            mask[y:y + 65, n - 3 if r % 2 == 0 else 2] = True
    return mask


@pytest.mark.parametrize("flipped", [False, True])
def test_a_serpentine_over_5_x_5_tiles(flipped):
    mask = serpentine()
    _, count, table, stats = check_mask(mask[::-1, ::-1] if flipped else mask)
    assert count == 1 and stats["tile_components"] == 25
    assert table["area"].tolist() == [int(mask.sum())]


def test_a_u_whose_arms_join_in_the_last_tile_row():
    mask = np.zeros((300, 200), bool)
    mask[0:291, 10] = True                               # the first cell: the top of this arm
    mask[5:291, 150] = True
    mask[290, 10:151] = True
    labels, count, table, _ = check_mask(mask)
    assert count == 1 and table["first"].tolist() == [10] and labels[5, 150] == 1
    mask[290, 100] = False                               # cut: the other arm is its own
    labels, count, table, _ = check_mask(mask)
    assert count == 2 and table["first"].tolist() == [10, 5 * 200 + 150]


@pytest.mark.parametrize("shape,offset", [((66, 66), 1), ((130, 130), 33)])
def test_a_spiral_corridor_inside_one_tile_and_across_four(shape, offset):
    _, count, table, _ = check_mask(spiral_corridor(shape, offset) < 9)
    assert count == 1 and table["area"].tolist() == [2047]


# ---------------------------------------------------------------------------
# random masks at the 8-connected percolation threshold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,density,seed", [((300, 300), 0.41, 3), ((130, 130), 0.5, 4)])
def test_random_masks_at_the_percolation_threshold(shape, density, seed):
    mask = np.random.default_rng(seed).random(shape) < density
    _, count, table, stats = check_mask(mask)
    print(f"{shape} p={density}: K={count}, largest {table['area'].max()} cells, "
          f"{stats['tile_components']} tile components")
    assert table["area"].max() > 2000                    # a cluster that spans tiles
    if seed == 3:
        assert count == 1323 and table["area"].max() == 24877


def test_every_tile_geometry():
    sizes = (63, 64, 65, 127, 129)
    for h in sizes:
        for w in sizes:
            check_mask(np.random.default_rng(h * 131 + w).random((h, w)) < 0.41)


# ---------------------------------------------------------------------------
# fills made by the library
# ---------------------------------------------------------------------------
def with_nan_patch(z):
    z = z.copy()
    z[200:204, 300:303] = np.nan
    return z


@pytest.mark.parametrize("epsilon", [0.0, 1e-3])
@pytest.mark.parametrize("variant", ["rough", "srtm"])
def test_the_depressions_of_a_fill(variant, epsilon):
    z = hdem_synth.synth_dem(512, 512, variant=variant)
    if variant == "rough":
        z = with_nan_patch(z)
    filled = hd.SinkFill(epsilon=epsilon).apply(z)
    labels, count, table, _ = check(z, filled, cellsize=30.0)
    print(f"{variant} eps={epsilon}: K={count}, largest {table['area'].max()} cells")
    assert count > 1                                     # (of the reference: a real input)
    assert not labels[np.isnan(z)].any()
    if epsilon == 0.0:
        # one water level per depression: the level is the fill at any of its cells
        assert np.array_equal(table["level"], filled.ravel()[table["first"]])
        cells = np.flatnonzero(labels)
        highest = np.full(count, -np.inf, np.float32)
        np.maximum.at(highest, labels.ravel()[cells].astype(np.int64) - 1, filled.ravel()[cells])
        assert np.array_equal(highest, table["level"])


def test_the_inventory_of_a_2048_raster_and_the_chain_give_the_same_labels():
    z = hdem_synth.synth_dem(2048, 2048, variant="rough")
    inventory = hd.DepressionInventory(cellsize=30.0)
    labels = inventory.apply(z)
    assert np.array_equal(inventory.filled, hd.SinkFill().apply(z))
    want, count, table = reference(z, inventory.filled, cellsize=30.0)
    assert np.array_equal(labels, want) and inventory.count == count
    assert_table(inventory.table, table)
    assert inventory.stats["depressions"] == count and inventory.fill_stats["converged"]
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(), hd.Depressions(dem=z)]
    assert np.array_equal(chain.apply(z), labels)
    assert chain.filters[1].count == count
    # the device form leaves the filled raster to the caller
    with backend.DeviceRaster.from_host(z) as dz:
        with inventory.apply_device(dz) as out, inventory.filled as filled:
            assert isinstance(filled, backend.DeviceRaster)
            assert np.array_equal(out.to_host(), want)
        assert_table(inventory.table, table)


# ---------------------------------------------------------------------------
# depths
# ---------------------------------------------------------------------------
def test_the_depth_quantum_saturates_rounds_and_levels_may_be_negative():
    dem = np.zeros((70, 70), np.float32)
    filled = dem.copy()
    filled[3, 3] = 3000.0                                # past 2048 m: 2^31 - 1 quanta
    filled[3, 4] = 1.0
    filled[10, 66] = np.float32(7.6e-6)                  # eight quanta
    filled[10, 67] = np.float32(2.5 / 2 ** 20)           # a tie: to even, two
    dem[40:50, 60:68] = -10.0
    filled[40:50, 60:68] = -5.0                          # a lake below zero, over a seam
    dem[44, 63] = -np.inf
    _, count, table, _ = check(dem, filled, cellsize=0.5)
    assert count == 3
    assert table["volume_q20"].tolist() == [2 ** 31 - 1 + 2 ** 20, 10, 79 * 5 * 2 ** 20 + 2 ** 31 - 1]
    assert table["level"].tolist() == [1.0, np.float32(2.5 / 2 ** 20), -5.0]
    assert table["max_depth"].tolist() == [3000.0, np.float32(7.6e-6), np.inf]


# ---------------------------------------------------------------------------
# the same bytes every time
# ---------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    mask = np.random.default_rng(11).random((300, 300)) < 0.41
    dem, filled = mask_pair(mask)
    filled *= np.random.default_rng(12).random(mask.shape).astype(np.float32)
    runs = []
    for _ in range(2):
        op = hd.Depressions(dem=dem, table=True)
        labels = op.apply(filled)
        runs.append(labels.tobytes() + b"".join(op.table[name].tobytes() for name in COLUMNS))
    assert runs[0] == runs[1]


def test_phase_times_are_reported_while_profiling():
    ctx = backend.context()
    op = hd.Depressions(dem=np.zeros((130, 130), np.float32))
    ctx.profile(True)
    try:
        op.apply(np.ones((130, 130), np.float32))
    finally:
        ctx.profile(False)
    assert op.stats["ms_tile"] > 0 and op.stats["ms_seam"] > 0 and op.stats["ms_final"] > 0
    assert "struct_size" not in op.stats and "reserved2" not in op.stats


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def test_labels_that_do_not_fit_the_rasters_are_refused():
    mask = np.random.default_rng(5).random((70, 90)) < 0.3
    dem, filled = mask_pair(mask)
    labels, count, table = reference(dem, filled)
    with pytest.raises(ValueError, match="greater than K"):
        backend.depression_table(dem, filled, labels, count - 1)
    other, _, _ = reference(*mask_pair(~mask))
    with pytest.raises(ValueError, match="do not belong to these rasters"):
        backend.depression_table(dem, filled, other, int(other.max()))
    with backend.DeviceRaster.from_host(dem) as d, backend.DeviceRaster.from_host(filled) as f, \
            backend.DeviceRaster.from_host(other) as foreign, \
            backend.DeviceRaster.from_host(labels) as good:
        with pytest.raises(ValueError, match="do not belong to these rasters"):
            backend.depression_table_dev(d, f, foreign, int(other.max()))
        with pytest.raises(ValueError, match="greater than K"):
            backend.depression_table_dev(d, f, good, 1)
        with backend.DeviceRaster.from_host(labels[:, :-1]) as narrow:
            with pytest.raises(ValueError):
                backend.depression_table_dev(d, f, narrow, count)
        with backend.DeviceRaster.from_host(labels.astype(np.float32)) as wrong:
            with pytest.raises(ValueError):
                backend.depression_table_dev(d, f, wrong, count)
        with pytest.raises(ValueError):
            backend.depressions_dev(d, good)                     # a filled raster is float32
        with pytest.raises(ValueError):
            backend.depressions_dev(d, narrow_raster_like(f))
        assert_table(backend.depression_table_dev(d, f, good, count), table)    # still usable


def narrow_raster_like(raster):
    """The same device memory seen as one column fewer (never dereferenced)."""
    return backend.DeviceRaster.wrap(raster.ptr, (raster.shape[0], raster.shape[1] - 1),
                                     raster.dtype, raster.ctx)


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_depressions_f32_dev, ctx.lib.hdem_depressions_f32):
        st = backend.DepressionsStats()
        rc = fn(ctx.handle, fake, fake, 65536, 65536, 0, fake, ctypes.byref(st))
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
        rc = fn(ctx.handle, fake, fake, 65536, 65536, backend.DEPR_COMPACT, fake, None)
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    for fn in (ctx.lib.hdem_depression_table_f32_dev, ctx.lib.hdem_depression_table_f32):
        rc = fn(ctx.handle, fake, fake, fake, 65536, 65536, 1, fake, None, None, None, None)
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    assert check_mask(np.ones((1, 5), bool))[1] == 1


def test_the_c_entry_points_check_flags_columns_and_struct_size():
    ctx = backend.context()
    z = np.zeros((4, 4), np.float32)
    w = z.copy()
    w[1:3, 1:3] = 1.0
    with backend.DeviceRaster.from_host(z) as dz, backend.DeviceRaster.from_host(w) as dw, \
            backend.DeviceRaster.empty((4, 4), np.uint32, ctx) as out:
        fn = ctx.lib.hdem_depressions_f32_dev
        call = lambda flags, st: fn(ctx.handle, dz.ptr, dw.ptr, 4, 4, flags, out.ptr, st)  # noqa: E731
        assert call(2, None) == backend.BAD_ARG
        assert b"flags" in ctx.lib.hdem_last_error()
        assert fn(ctx.handle, dz.ptr, None, 4, 4, 0, out.ptr, None) == backend.BAD_ARG
        st = backend.DepressionsStats()
        st.struct_size = 2
        assert call(0, ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend.DepressionsStats()
        st.struct_size = 24                              # an older, shorter struct
        st.tile_components, st.tile_h = -5, -7
        assert call(backend.DEPR_COMPACT, ctypes.byref(st)) == backend.OK
        assert st.struct_size == 24 and st.depressions == 1 and st.raised_cells == 4
        assert st.tile_components == -5 and st.tile_h == -7      # nothing beyond it is written
        want = np.zeros((4, 4), np.uint32)
        want[1:3, 1:3] = 1
        assert np.array_equal(out.to_host(), want)
        table = ctx.lib.hdem_depression_table_f32_dev
        none = [None] * 5
        assert table(ctx.handle, dz.ptr, dw.ptr, out.ptr, 4, 4, 1, *none) == backend.BAD_ARG
        assert b"column" in ctx.lib.hdem_last_error()
        assert table(ctx.handle, dz.ptr, dw.ptr, out.ptr, 4, 4, 17, out.ptr,
                     *none[1:]) == backend.BAD_ARG
        assert table(ctx.handle, dz.ptr, dw.ptr, None, 4, 4, 1, out.ptr,
                     *none[1:]) == backend.BAD_ARG
        # K == 0 is legal and launches nothing: the labels are not even looked at
        assert table(ctx.handle, dz.ptr, dw.ptr, out.ptr, 4, 4, 0, out.ptr,
                     *none[1:]) == backend.OK
        # one column alone
        with backend.DeviceRaster.empty((1, 1), np.uint32, ctx) as area:
            assert table(ctx.handle, dz.ptr, dw.ptr, out.ptr, 4, 4, 1, None, area.ptr,
                         None, None, None) == backend.OK
            assert area.to_host().tolist() == [[4]]
