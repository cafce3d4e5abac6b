"""
D8 watershed labelling on the MI355X (``Watersheds``, ``hdem_watershed_u8[_dev]``).  Every
comparison is ``np.array_equal``: exact answers on constructed paths, the hazards of the
tiled scheme as hand-built cases with written-out answers, agreement with reference (b) of
tests/test_watersheds.py on random acyclic codes (outlet and pour-point mode) and on the
filled synthetic DEMs, the local proof and the compact numbering at 16384^2 (basin areas
against the device ``FlowAccumulation``), and the error cases (invalid bytes, cycles, size).

Value-only mutants of the kernels that were run against this file, with a test each fails:
  the seed left out of a perimeter stop's forest word, and a seeded exit cell treated as an
  exit                          -> test_a_seed_on_a_frame_exit_cell_and_on_the_cell_it_drains_into
  corner ``slot_of`` one tile off -> test_a_diagonal_corner_crossing_between_four_tiles
  11 doubling rounds in the tile pass -> test_a_spiral
  the forest schedule cut to two launches -> test_a_row_and_a_column_take_their_last_cell
(No tile reads the seeds of its halo, so "halo seeds ignored" has no counterpart here.)
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from oracle.hdem_oracle_np import d8_flow_direction
from test_flowacc import random_acyclic_codes, terminal_mask
from test_gpu_flowacc import path_codes, snake, spiral
from test_watersheds import labels_doubling, outlet_labels_hold, random_seeds

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
RANDOM_SHAPES = [(1, 1), (1, 2), (3, 3), (63, 63), (64, 64), (65, 65), (130, 257), (257, 130),
                 (1, 4097), (4097, 1)]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def watersheds(codes, pour_points=None, labels="outlet"):
    got = hd.Watersheds(pour_points, labels).apply(np.ascontiguousarray(codes, dtype=np.uint8))
    assert got.dtype == np.uint32 and got.shape == np.shape(codes)
    return got


def index1(shape):
    """1 + flat index of every cell: the outlet-mode label of a terminal cell."""
    return (np.arange(shape[0] * shape[1], dtype=np.int64) + 1).reshape(shape)


def outlet_answer(shape, cells):
    """Outlet-mode answer for ``path_codes(shape, cells)``: the path holds its last cell's
    label, every other cell its own."""
    want = index1(shape)
    last = want[cells[-1]]
    for y, x in cells:
        want[y, x] = last
    return want


# ---------------------------------------------------------------------------
# constructed paths: exact answers
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_take_their_last_cell():
    got = watersheds(np.full((1, 10000), E, np.uint8))           # 156 tile crossings
    assert np.array_equal(got[0], np.full(10000, 10000))
    got = watersheds(np.full((10000, 1), S, np.uint8))
    assert np.array_equal(got[:, 0], np.full(10000, 10000))


def test_a_snake_through_every_tile():
    cells = snake(512, 512)
    f = hd.Watersheds()
    got = f.apply(path_codes((512, 512), cells))
    assert np.array_equal(got, np.full((512, 512), cells[-1][0] * 512 + cells[-1][1] + 1))
    assert f.stats["tile_h"] == 64 and f.stats["tile_w"] == 64
    assert f.stats["basins"] == 1 and f.stats["exits"] == 512 * 7 + 7
    assert f.stats["forest_rounds"] >= 2                 # 3591 crossings at 4 jumps a round


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    assert len(cells) == 4096
    got = watersheds(path_codes(shape, cells))
    assert np.array_equal(got, outlet_answer(shape, cells))
    assert (got == got[cells[0]]).sum() == 4096


def test_a_cone_drains_to_its_apex():
    n = 301
    yy, xx = np.indices((n, n), dtype=np.float32)
    z = np.sqrt((yy - n // 2) ** 2 + (xx - n // 2) ** 2).astype(np.float32)
    codes = d8_flow_direction(z)
    got = watersheds(codes)
    want = index1((n, n))
    want[1:-1, 1:-1] = want[n // 2, n // 2]              # D8 leaves the border cells at 0
    assert np.array_equal(got, want)


def test_codes_pointing_outside_the_raster_are_terminal():
    h, w = 100, 130
    got = watersheds(np.full((h, w), N, np.uint8))         # row 0 points off the top
    assert np.array_equal(got, np.repeat(index1((h, w))[:1], h, axis=0))
    got = watersheds(np.full((h, w), E, np.uint8))         # last column off the right
    assert np.array_equal(got, np.repeat(index1((h, w))[:, -1:], w, axis=1))
    codes = np.zeros((h, w), np.uint8)
    codes[0, :], codes[-1, :], codes[:, 0], codes[:, -1] = N, S, W_, E
    codes[0, 0], codes[0, -1], codes[-1, 0], codes[-1, -1] = NW, NE, SW, SE
    assert np.array_equal(watersheds(codes), index1((h, w)))


# ---------------------------------------------------------------------------
# random acyclic codes against reference (b)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_match_the_doubling_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    want = labels_doubling(codes)
    if codes.size >= 9:
        assert len(np.unique(want)) > 1                  # an all-same answer cannot pass
    assert np.array_equal(watersheds(codes), want)


@pytest.mark.parametrize("shape", RANDOM_SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_with_pour_points_match_the_doubling_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    seeds = random_seeds(shape, seed=shape[0] * 3 + shape[1], every=50)
    want = labels_doubling(codes, seeds)
    print(f"{shape} ramp={ramp}: {100.0 * np.count_nonzero(want) / want.size:.1f} % labelled")
    if codes.size >= 9:
        assert (want == 0).any() and (want != 0).any()   # neither all-zero nor all-same
    assert np.array_equal(want[seeds != 0], seeds[seeds != 0])
    assert want.max() == 2 ** 32 - 1
    assert np.array_equal(watersheds(codes, seeds), want)


# ---------------------------------------------------------------------------
# the hazards of the tiled scheme, answers written out
# ---------------------------------------------------------------------------
def test_a_seed_on_a_frame_exit_cell_and_on_the_cell_it_drains_into():
    row = np.full((1, 130), E, np.uint8)                 # tiles end at x = 63 and 127
    seeds = np.zeros((1, 130), np.uint32)
    seeds[0, 63] = 7                                     # the exit cell of tile 0 itself
    assert np.array_equal(watersheds(row, seeds)[0], [7] * 64 + [0] * 66)
    seeds[:] = 0
    seeds[0, 64] = 9                                     # the halo cell that exit drains into
    assert np.array_equal(watersheds(row, seeds)[0], [9] * 65 + [0] * 65)
    seeds[0, 63] = 7                                     # both
    assert np.array_equal(watersheds(row, seeds)[0], [7] * 64 + [9] + [0] * 65)
    col = np.full((130, 1), N, np.uint8)                 # upwards: exits at y = 64 and 128
    seeds = np.zeros((130, 1), np.uint32)
    seeds[64, 0], seeds[127, 0] = 3, 2 ** 32 - 1
    assert np.array_equal(watersheds(col, seeds)[:, 0],
                          [0] * 64 + [3] * 63 + [2 ** 32 - 1] * 3)


@pytest.mark.parametrize("anti", [False, True], ids=["SE", "SW"])
def test_a_diagonal_corner_crossing_between_four_tiles(anti):
    n = 128
    cells = [(k, n - 1 - k if anti else k) for k in range(n)]    # (63, 63) -> (64, 64)
    codes = path_codes((n, n), cells)
    codes[cells[-1]] = SW if anti else SE                # the last one points outside
    assert np.array_equal(watersheds(codes), outlet_answer((n, n), cells))
    for at in (64, 70):                                  # the corner cell itself; further in
        seeds = np.zeros((n, n), np.uint32)
        seeds[cells[at]] = 5
        want = np.zeros((n, n), np.int64)
        for y, x in cells[:at + 1]:
            want[y, x] = 5
        assert np.array_equal(watersheds(codes, seeds), want)
        assert np.array_equal(watersheds(codes, [cells[at] + (5,)]), want)


def test_a_seed_on_a_terminal_cell():
    row = np.full((1, 10), E, np.uint8)                  # cell 9 points outside
    assert np.array_equal(watersheds(row, [(0, 9, 4)])[0], [4] * 10)
    row[0, 9] = 0
    assert np.array_equal(watersheds(row, [(0, 9, 4)])[0], [4] * 10)
    assert np.array_equal(watersheds(row, [(0, 9), (0, 2)])[0], [2] * 3 + [1] * 7)


def test_two_nested_seeds_on_one_path_crossing_four_tiles():
    cells = ([(30, x) for x in range(5, 121)] + [(y, 120) for y in range(31, 101)]
             + [(100, x) for x in range(119, 5, -1)])
    assert len(cells) == 300
    assert {(y // 64, x // 64) for y, x in cells} == {(0, 0), (0, 1), (1, 1), (1, 0)}
    codes = path_codes((128, 128), cells)
    want = np.zeros((128, 128), np.int64)
    for k, (y, x) in enumerate(cells):
        want[y, x] = 11 if k <= 100 else 22 if k <= 250 else 0
    got = watersheds(codes, [cells[100] + (11,), cells[250] + (22,)])
    assert np.array_equal(got, want)
    assert (got == 11).sum() == 101 and (got == 22).sum() == 150
    assert np.array_equal(watersheds(codes), outlet_answer((128, 128), cells))


# ---------------------------------------------------------------------------
# the filled synthetic DEMs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,eps", [("rough", 1e-3), ("srtm", 0.0)])
def test_fill_d8_watersheds_chain_on_4096(variant, eps):
    import oracle  # noqa: F401
    from oracle import c_oracle
    z = hdem_synth.synth_dem(4096, 4096, variant=variant)
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(epsilon=eps), hd.D8FlowDirection(), hd.Watersheds()]
    got = chain.apply(z)
    assert got.dtype == np.uint32
    codes = c_oracle.d8(c_oracle.sinkfill_pflood(z, eps))
    assert codes.dtype == np.uint8
    assert np.array_equal(got, labels_doubling(codes))
    assert chain.filters[2].stats["exits"] > 0
    assert chain.filters[2].stats["basins"] == int(terminal_mask(codes).sum())


def test_16384_holds_the_local_proof_and_compact_labels_give_the_basin_areas():
    z = hdem_synth.synth_dem(16384, 16384)
    with backend.DeviceRaster.from_host(z) as dz:
        del z
        filled, dcodes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
        filled.free()
    with dcodes:
        dlab, none, stats = backend.watershed_dev(dcodes)
        with dlab:
            codes, labels = dcodes.to_host(), dlab.to_host()
        assert none is None
        f = hd.Watersheds(labels="compact")
        with f.apply_device(dcodes) as dcompact:
            compact = dcompact.to_host()
        dacc, _ = backend.flowacc_dev(dcodes)
        with dacc:
            acc = dacc.to_host()
    ok, terminals = outlet_labels_hold(codes, labels)
    assert ok                                            # acyclic codes: a proof
    assert stats["exits"] > 0 and stats["forest_rounds"] >= 2
    k = f.stats["basins"]
    outlets = f.outlets
    assert k == terminals == stats["basins"]
    assert outlets.dtype == np.uint32 and outlets.shape == (k,)
    assert compact.min() == 1 and compact.max() == k
    areas = np.bincount(compact.ravel(), minlength=k + 1)
    assert areas[0] == 0 and (areas[1:] > 0).all()       # exactly 1 ... K
    assert len(np.unique(outlets)) == k
    oy, ox = np.divmod(outlets.astype(np.int64), codes.shape[1])
    assert np.array_equal(labels[oy, ox], outlets.astype(np.int64) + 1)   # terminal cells
    assert np.array_equal(outlets[compact.ravel() - 1].astype(np.int64) + 1,
                          labels.ravel())
    assert np.array_equal(areas[1:], acc[oy, ox])


# ---------------------------------------------------------------------------
# host and device paths, repeatability, profiling
# ---------------------------------------------------------------------------
def test_host_and_device_paths_are_bit_equal_and_repeatable():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    seeds = random_seeds(codes.shape, seed=11, every=200)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(seeds, dtype=np.uint32) as ds:
        for pour, labels in ((None, "outlet"), (seeds, "outlet"), (None, "compact")):
            f, g, d = (hd.Watersheds(pour, labels) for _ in range(3))
            a = f.apply(codes)
            b = g.apply(codes)
            with d.apply_device(dc) as dev:
                assert dev.dtype == np.uint32
                c = dev.to_host()
            assert a.dtype == b.dtype == c.dtype == np.uint32
            assert np.array_equal(a, b) and np.array_equal(a, c)
            if labels == "compact":
                assert np.array_equal(f.outlets, g.outlets)
                assert np.array_equal(f.outlets, d.outlets)
                assert np.array_equal(f.outlets[a.ravel() - 1].astype(np.int64) + 1,
                                      labels_doubling(codes).ravel())
                assert len(f.outlets) == int(terminal_mask(codes).sum()) == a.max()
            else:
                assert f.outlets is None and d.outlets is None
                assert np.array_equal(a, labels_doubling(codes, pour))
        with hd.Watersheds(pour_points=ds).apply_device(dc) as dev:     # seeds on the device
            assert np.array_equal(dev.to_host(), labels_doubling(codes, seeds))
        assert np.array_equal(hd.Watersheds(pour_points=ds).apply(codes),
                              labels_doubling(codes, seeds))


def test_compact_labels_on_small_and_partial_tiles():
    for shape in [(1, 1), (3, 3), (65, 65), (130, 257)]:
        codes = random_acyclic_codes(*shape, seed=shape[0] + shape[1], ramp=True)
        f = hd.Watersheds(labels="compact")
        got = f.apply(codes)
        k = int(terminal_mask(codes).sum())
        assert f.stats["basins"] == k == len(f.outlets)
        assert np.array_equal(np.unique(got), np.arange(1, k + 1))
        assert np.array_equal(f.outlets[got.ravel() - 1].astype(np.int64) + 1,
                              labels_doubling(codes).ravel())


def test_profiling_fills_the_phase_times_and_leaves_them_zero_when_off():
    codes = random_acyclic_codes(300, 300, seed=5, ramp=True)
    ctx = backend.context()
    f = hd.Watersheds()
    f.apply(codes)
    assert f.stats["ms_tile"] == 0 and f.stats["ms_forest"] == 0 and f.stats["ms_final"] == 0
    ctx.profile(True)
    try:
        f.apply(codes)
    finally:
        ctx.profile(False)
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0
    assert "struct_size" not in f.stats


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def rim_codes():
    codes = np.zeros((256, 256), np.uint8)               # clockwise round a 200 x 200 rim:
    y0, x0, n = 10, 20, 200                              # through all four tiles round (128, 128)
    codes[y0, x0:x0 + n - 1] = E
    codes[y0:y0 + n - 1, x0 + n - 1] = S
    codes[y0 + n - 1, x0 + 1:x0 + n] = W_
    codes[y0 + 1:y0 + n, x0] = N
    assert int((codes != 0).sum()) == 796
    return codes


def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="cycle: 2 cells never resolve"):
        watersheds(np.array([[E, W_]], np.uint8))
    codes = rim_codes()
    codes[100, 21:100] = W_                              # 79 cells that drain into the loop
    with pytest.raises(ValueError, match="cycle: 875 cells never resolve"):
        watersheds(codes)
    with pytest.raises(ValueError, match="cycle"):
        watersheds(codes, labels="compact")
    with pytest.raises(ValueError, match="cycle"):       # a pour point elsewhere does not help
        watersheds(codes, [(0, 0)])
    cells = snake(130, 70)
    assert np.array_equal(watersheds(path_codes((130, 70), cells)),
                          outlet_answer((130, 70), cells))
    # a loop that holds a pour point resolves there: legal, and reference (b) agrees
    want = np.zeros((256, 256), np.int64)
    want[codes != 0] = 6
    got = watersheds(codes, [(10, 150, 6)])
    assert np.array_equal(got, want)
    seeds = np.zeros((256, 256), np.uint32)
    seeds[10, 150] = 6
    assert np.array_equal(got, labels_doubling(codes, seeds))


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        watersheds(codes)
    with pytest.raises(ValueError, match="invalid D8 code"):
        watersheds(codes, [(0, 0)])
    assert np.array_equal(watersheds(np.full((3, 5), S, np.uint8))[:, 0], [11, 11, 11])


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_watershed_u8_dev, ctx.lib.hdem_watershed_u8):
        st = backend.WatershedStats()
        rc = fn(ctx.handle, fake, 65536, 65536, None, 0, fake, None, ctypes.byref(st))
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
        rc = fn(ctx.handle, fake, 65536, 65536, fake, 0, fake, None, None)
        assert rc == backend.BAD_ARG and b"2^32" in ctx.lib.hdem_last_error()
    assert np.array_equal(watersheds(np.full((1, 5), E, np.uint8))[0], [5] * 5)


def test_the_c_entry_points_check_flags_outlets_and_struct_size():
    ctx = backend.context()
    with backend.DeviceRaster.from_host(np.full((4, 4), E, np.uint8), dtype=np.uint8) as dc, \
            backend.DeviceRaster.empty((4, 4), np.uint32, ctx) as do:
        fn = ctx.lib.hdem_watershed_u8_dev
        call = lambda seeds, flags, outlets, st: fn(      # noqa: E731
            ctx.handle, dc.ptr, 4, 4, seeds, flags, do.ptr, outlets, st)
        assert call(do.ptr, backend.WS_COMPACT, do.ptr, None) == backend.BAD_ARG
        assert b"pour points" in ctx.lib.hdem_last_error()
        assert call(None, backend.WS_COMPACT, None, None) == backend.BAD_ARG
        assert call(None, 0, do.ptr, None) == backend.BAD_ARG
        assert call(None, 2, None, None) == backend.BAD_ARG
        st = backend.WatershedStats()
        st.struct_size = 0
        assert call(None, 0, None, ctypes.byref(st)) == backend.BAD_ARG
        assert b"struct_size" in ctx.lib.hdem_last_error()
        st = backend.WatershedStats()
        st.struct_size = 16                              # an older, shorter struct
        st.exits, st.tile_h = -5, -7
        assert call(None, 0, None, ctypes.byref(st)) == backend.OK
        assert st.struct_size == 16 and st.basins == 4
        assert st.exits == -5 and st.tile_h == -7        # nothing beyond it is written
        assert np.array_equal(do.to_host(), np.repeat([[4], [8], [12], [16]], 4, axis=1))
