"""
Constructor arguments the reference's own pipeline never uses: CorrectNANValues with a
window other than 3 and BlanksFourier with a window other than 55, against outputs of the
imported reference (tests/golden/windows.npz, make_golden_windows.py).
"""
import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wz(golden, built):
    return golden("windows.npz")


@pytest.mark.parametrize("ws", [3, 5, 7])
def test_correct_nan_values_any_window(wz, ws):
    hs = wz["hs"].copy()
    got = hd.CorrectNANValues(window_size=ws).apply(hs)
    assert got is hs                                      # in place, like the reference
    assert np.array_equal(got, wz[f"fixed{ws}"], equal_nan=True)
    # the device form: the same cells, out of place
    dev = hd.CorrectNANValues(window_size=ws).apply_device(
        backend.DeviceRaster.from_host(wz["hs"])).to_host()
    assert np.array_equal(dev, wz[f"fixed{ws}"], equal_nan=True)


@pytest.mark.parametrize("ws", [15, 21, 35])
def test_blanks_fourier_any_window(wz, ws):
    found, modified = hd.BlanksFourier(window_size=ws).apply(wz["q"].copy())
    assert np.array_equal(found, wz[f"found{ws}"])
    assert found.sum() > 100
    # the reference multiplies in float64; here the float32 cell is kept or zeroed
    assert np.array_equal(modified, wz[f"modified{ws}"].astype(np.float32))


def test_window_limits(built):
    q = np.ones((300, 300), dtype=np.float32)
    with pytest.raises(hd.WindowSizeEvenError):
        hd.BlanksFourier(window_size=20).apply(q)
    with pytest.raises(hd.WindowSizeHighError):
        hd.BlanksFourier(window_size=301).apply(q)
    with pytest.raises(hd.WindowSizeHighError):
        hd.CorrectNANValues(window_size=5).apply(np.zeros((4, 9), dtype=np.float32))
    with pytest.raises(hd.WindowSizeEvenError):
        hd.CorrectNANValues(window_size=4).apply(np.zeros((9, 9), dtype=np.float32))
    with pytest.raises(ValueError):
        hd.CorrectNANValues(window_size=13).apply(np.zeros((40, 40), dtype=np.float32))
    with pytest.raises(ValueError):
        hd.BlanksFourier(window_size=5).apply(q)


@pytest.mark.parametrize("shape,ws", [((300, 1501), 55), ((97, 2050), 21), ((64, 470), 55),
                                      ((33, 513), 7)])
def test_blanks_fourier_across_block_seams(built, shape, ws):
    """Several 458-column blocks side by side and several 32-row segments on top of each
    other, widths that are no multiple of four: every cell against the NumPy oracle (cells
    within rounding of the threshold may fall either way; there are none in these cases
    unless the assert says so)."""
    from oracle import hdem_oracle_fourier as F
    rng = np.random.default_rng(shape[1] + ws)
    q = np.exp(rng.normal(0.0, 1.5, shape)).astype(np.float32)
    q[rng.random(shape) < 0.002] *= 200.0
    want, want_q, margin = F.blanks_fourier(q, ws)
    found, modified = hd.BlanksFourier(window_size=ws).apply(q.copy())
    diff = found != want
    borderline = np.abs(margin) <= 1e-6 * np.abs(q)
    assert not (diff & ~borderline).any(), f"{int((diff & ~borderline).sum())} cells differ"
    assert found.sum() > 20
    same = ~diff
    assert np.array_equal(modified[same], want_q.astype(np.float32)[same])


# ---------------------------------------------------------------------------
# The window rule at the C boundary: SlidingWindow's two refusals (too high before even,
# sliding_window.py:150-156), status and text, from every entry point that takes a window.
# Every call is refused, so no kernel runs.
# ---------------------------------------------------------------------------
H12, W14 = 12, 14
EVEN_TEXT = "Window size: {} cannot be an even number"
HIGH_TEXT = "Window size: {} cannot be higher than grid dimensions: ({}, {})"
# window -> status, text on the 12 x 14 raster; 16 is even and too high: the height wins
VARIABLE_WINDOWS = {4: (backend.WINDOW_EVEN, EVEN_TEXT.format(4)),
                    13: (backend.WINDOW_HIGH, HIGH_TEXT.format(13, H12, W14)),
                    16: (backend.WINDOW_HIGH, HIGH_TEXT.format(16, H12, W14))}


@pytest.fixture(scope="module")
def boundary(built):
    """A context, two distinct device buffers of zeros (float32 128 x 130: room for every
    shape and type the refused calls name) and 12 x 14 host arrays."""
    ctx = backend.context()
    a, b = (backend.DeviceRaster.empty((128, 130), np.float32, ctx) for _ in range(2))
    for r in (a, b):
        ctx.check(ctx.lib.hdem_memset_dev(ctx.handle, r.ptr, 0, r.nbytes))
    host = np.zeros((H12, W14), np.float32), np.empty((H12, W14), np.float32)
    yield ctx, a, b, host
    a.free()
    b.free()


def _status_and_text(ctx, name, *args):
    rc = getattr(ctx.lib, name)(ctx.handle, *args)
    return rc, ctx.lib.hdem_last_error().decode()


def _variable_window_calls(a, b, host):
    """name -> the call's arguments behind the context, as a function of the window."""
    hin, hout = (h.ctypes.data for h in host)
    return {
        "hdem_quadratic_f32_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
        "hdem_quadratic_f32": lambda ws: (hin, H12, W14, ws, hout),
        "hdem_groves_f32_dev": lambda ws: (a.ptr, a.ptr, H12, W14, ws, 1.5, 1, None, b.ptr),
        "hdem_groves_f32": lambda ws: (hin, hin, H12, W14, ws, 1.5, 1, hout),
        "hdem_correct_nan_f32_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
        "hdem_majority_f32_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
        "hdem_blanks_fourier_f32_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
        "hdem_isolated_points_u8_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
        "hdem_expand_u8_dev": lambda ws: (a.ptr, H12, W14, ws, b.ptr),
    }


def test_the_c_boundary_refuses_windows_as_sliding_window_does(boundary):
    ctx, a, b, host = boundary
    got, want = {}, {}
    for name, args in _variable_window_calls(a, b, host).items():
        for ws, expected in VARIABLE_WINDOWS.items():
            got[name, ws] = _status_and_text(ctx, name, *args(ws))
            want[name, ws] = expected
    # the operators whose window is fixed, on rasters one row too low for it; the destripe
    # checks its window against the spectrum's quadrants, (H / 2 - 10) x (W / 2 - 10)
    for name, args, window, shape in (
            ("hdem_tidying_lagoons_f32_dev", (a.ptr, 6, W14, b.ptr), 7, (6, W14)),
            ("hdem_lagoons_detection_f32_dev", (a.ptr, 10, W14, None, None, b.ptr), 11,
             (10, W14)),
            ("hdem_fourier_destripe_f32_dev", (a.ptr, H12, W14, b.ptr, None), 55, (0, 0)),
            ("hdem_fourier_destripe_f32_dev", (a.ptr, 2, 84, b.ptr, None), 55, (0, 32)),
            ("hdem_fourier_destripe_f32_dev", (a.ptr, 128, 130, b.ptr, None), 55, (54, 55))):
        got[name, shape] = _status_and_text(ctx, name, *args)
        want[name, shape] = (backend.WINDOW_HIGH, HIGH_TEXT.format(window, *shape))
    assert got == want
    # the refusals leave the context usable
    assert _status_and_text(ctx, "hdem_quadratic_f32_dev", a.ptr, H12, W14, 3, b.ptr)[0] == \
        backend.OK
    out = backend.DeviceRaster.wrap(b.ptr, (H12, W14), np.float32, ctx).to_host()
    assert np.array_equal(out, np.zeros((H12, W14), np.float32))
