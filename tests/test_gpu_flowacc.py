"""
D8 flow accumulation on the MI355X (``FlowAccumulation``, ``hdem_flowacc_u8[_dev]``):
exact answers on constructed paths, agreement with the host references of
tests/test_flowacc.py on random acyclic codes and on the filled synthetic DEMs, the
local balance check at 16384^2, and the error cases (invalid bytes, cycles, size).
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend
from oracle.hdem_oracle_np import d8_flow_direction
from test_flowacc import (acc_brute, acc_kahn, balanced, random_acyclic_codes,
                          terminal_mask)

pytestmark = pytest.mark.gpu

E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def flowacc(codes):
    return hd.FlowAccumulation().apply(np.ascontiguousarray(codes, dtype=np.uint8))


def path_codes(shape, cells):
    """Codes that send each cell of ``cells`` (a list of (y, x), neighbours in order) to
    the next one; the last is terminal, every other cell is 0."""
    codes = np.zeros(shape, np.uint8)
    by_step = {(0, 1): E, (1, 1): SE, (1, 0): S, (1, -1): SW, (0, -1): W_, (-1, -1): NW,
               (-1, 0): N, (-1, 1): NE}
    for (y, x), (ny, nx) in zip(cells[:-1], cells[1:]):
        codes[y, x] = by_step[(ny - y, nx - x)]
    return codes


def path_answer(shape, cells):
    acc = np.ones(shape, np.int64)
    for k, (y, x) in enumerate(cells):
        acc[y, x] = k + 1
    return acc


def snake(h, w):
    return [(y, x if y % 2 == 0 else w - 1 - x) for y in range(h) for x in range(w)]


def spiral(y0, x0, n):
    cells, top, left, bottom, right = [], y0, x0, y0 + n - 1, x0 + n - 1
    while top <= bottom and left <= right:
        cells += [(top, x) for x in range(left, right + 1)]
        cells += [(y, right) for y in range(top + 1, bottom + 1)]
        if top < bottom:
            cells += [(bottom, x) for x in range(right - 1, left - 1, -1)]
        if left < right:
            cells += [(y, left) for y in range(bottom - 1, top, -1)]
        top, left, bottom, right = top + 1, left + 1, bottom - 1, right - 1
    return cells


# ---------------------------------------------------------------------------
# constructed paths: exact answers
# ---------------------------------------------------------------------------
def test_a_row_and_a_column_count_their_position():
    got = flowacc(np.full((1, 10000), E, np.uint8))
    assert got.dtype == np.uint32
    assert np.array_equal(got[0], np.arange(1, 10001))          # 156 tile crossings
    got = flowacc(np.full((10000, 1), S, np.uint8))
    assert np.array_equal(got[:, 0], np.arange(1, 10001))


def test_a_snake_through_every_tile():
    cells = snake(512, 512)
    codes = path_codes((512, 512), cells)
    f = hd.FlowAccumulation()
    got = f.apply(codes)
    assert np.array_equal(got, path_answer((512, 512), cells))
    assert f.stats["tile_h"] == 64 and f.stats["tile_w"] == 64
    assert f.stats["max_hops"] >= 63                      # the path crosses every tile


@pytest.mark.parametrize("offset", [0, 1], ids=["one_tile", "four_tiles"])
def test_a_spiral(offset):
    shape = (64 + 2 * offset, 64 + 2 * offset)
    cells = spiral(offset, offset, 64)
    assert len(cells) == 4096
    codes = path_codes(shape, cells)
    assert np.array_equal(flowacc(codes), path_answer(shape, cells))


def test_a_cone_drains_to_its_apex():
    n = 301
    yy, xx = np.indices((n, n), dtype=np.float32)
    z = np.sqrt((yy - n // 2) ** 2 + (xx - n // 2) ** 2).astype(np.float32)
    codes = d8_flow_direction(z)
    got = flowacc(codes)
    assert got[n // 2, n // 2] == 299 * 299
    assert np.array_equal(got, acc_brute(codes))


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (63, 63), (64, 64), (65, 65),
                                   (127, 129), (7, 1000), (1000, 7), (4097, 300)])
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_random_acyclic_codes_match_the_kahn_reference(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=ramp)
    assert np.array_equal(flowacc(codes), acc_kahn(codes))


def test_codes_pointing_outside_the_raster_are_terminal():
    h, w = 100, 130
    got = flowacc(np.full((h, w), N, np.uint8))            # row 0 points off the top
    assert np.array_equal(got, np.repeat(np.arange(h, 0, -1)[:, None], w, axis=1))
    got = flowacc(np.full((h, w), E, np.uint8))            # last column off the right
    assert np.array_equal(got, np.repeat(np.arange(1, w + 1)[None, :], h, axis=0))
    codes = np.zeros((h, w), np.uint8)
    codes[0, :], codes[-1, :], codes[:, 0], codes[:, -1] = N, S, W_, E
    codes[0, 0], codes[0, -1], codes[-1, 0], codes[-1, -1] = NW, NE, SW, SE
    assert np.array_equal(flowacc(codes), np.ones((h, w), np.int64))


# ---------------------------------------------------------------------------
# the filled synthetic DEMs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,eps", [("rough", 1e-3), ("srtm", 0.0)])
def test_fill_d8_accumulation_chain_on_4096(variant, eps):
    z = hdem_synth.synth_dem(4096, 4096, variant=variant)
    chain = hd.ComposedFilter()
    chain.filters = [hd.SinkFill(epsilon=eps), hd.D8FlowDirection(), hd.FlowAccumulation()]
    got = chain.apply(z)
    assert got.dtype == np.uint32
    codes = hd.D8FlowDirection().apply(hd.SinkFill(epsilon=eps).apply(z))
    host = hd.FlowAccumulation().apply(codes)
    assert np.array_equal(got, host)                       # member by member, on the host
    assert np.array_equal(host, acc_kahn(codes))
    assert chain.filters[2].stats["exits"] > 0


def test_16384_passes_the_balance_check():
    z = hdem_synth.synth_dem(16384, 16384)
    with backend.DeviceRaster.from_host(z) as dz:
        filled, dcodes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
        filled.free()
        with dcodes:
            dacc, stats = backend.flowacc_dev(dcodes)
            with dacc:
                codes, acc = dcodes.to_host(), dacc.to_host()
    assert balanced(codes, acc)
    assert int(acc[terminal_mask(codes)].sum(dtype=np.int64)) == codes.size
    assert stats["exits"] > 0 and stats["max_hops"] > 0


def test_host_and_device_paths_are_bit_equal_and_repeatable():
    codes = random_acyclic_codes(700, 900, seed=3, ramp=True)
    a = flowacc(codes)
    b = flowacc(codes)
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc:
        dev = hd.FlowAccumulation().apply_device(dc)
        with dev:
            assert dev.dtype == np.uint32
            c = dev.to_host()
    assert a.dtype == b.dtype == c.dtype == np.uint32
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_profiling_times_the_call_and_its_phases():
    ctx = backend.context()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        f = hd.FlowAccumulation()
        f.apply(random_acyclic_codes(300, 300, seed=5, ramp=True))
        st = ctx.profile_get(backend.K_FLOWACC)
    finally:
        ctx.profile(False)
    assert st["launches"] == 1 and st["ms"] > 0 and st["units"] == 300 * 300
    assert f.stats["ms_tile"] > 0 and f.stats["ms_forest"] > 0 and f.stats["ms_final"] > 0


# ---------------------------------------------------------------------------
# errors: bounded time, the context stays usable
# ---------------------------------------------------------------------------
def test_cycles_raise_and_the_next_call_is_correct():
    with pytest.raises(ValueError, match="cycle"):
        flowacc(np.array([[E, W_]], np.uint8))
    codes = np.zeros((256, 256), np.uint8)               # clockwise round a 200 x 200 rim
    y0, x0, n = 10, 20, 200
    codes[y0, x0:x0 + n - 1] = E
    codes[y0:y0 + n - 1, x0 + n - 1] = S
    codes[y0 + n - 1, x0 + 1:x0 + n] = W_
    codes[y0 + 1:y0 + n, x0] = N
    assert int((codes != 0).sum()) == 796
    with pytest.raises(ValueError, match="cycle"):
        flowacc(codes)
    cells = snake(130, 70)
    assert np.array_equal(flowacc(path_codes((130, 70), cells)), path_answer((130, 70), cells))


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code"):
        flowacc(codes)
    assert np.array_equal(flowacc(np.full((3, 5), S, np.uint8))[:, 0], [1, 2, 3])


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_flowacc_u8_dev, ctx.lib.hdem_flowacc_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, fake, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    assert np.array_equal(flowacc(np.full((1, 5), E, np.uint8))[0], [1, 2, 3, 4, 5])
