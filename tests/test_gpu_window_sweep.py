"""
Every window size and launch path of the windowed stencil kernels, each against an
independent reference of the same operation: the float64 quadratic (oracle), SciPy's
morphology and convolution, and the NumPy restatements of CorrectNANValues / ExpandFilter /
IsolatedPoints, which tests/test_oracle_windows.py pins to the imported reference at these
window sizes (tests/golden/window_sweep.npz).

Where a case exists to reach one launch branch, the branch's condition is recomputed here
from the kernel's constants (mirrored below, with the line they come from) and asserted.
Every input is asserted to tell the plausible wrong answers apart (the neighbouring window,
the mirrored structure, the transposed size, one iteration more, another summation order).

Path                                                      test
groves_stream_kernel<9, *>; tiled groves_kernel<11..29>   test_quadratic_every_window,
FULL strips + general last strip column in one launch       test_groves_every_window
fused groves pass at every window                         test_groves_every_window
mask at base + 1 with W % 4 == 0 (fx = 0)                 test_groves_misaligned_mask
grey_dilation_kernel<0, 0, T>, float64 (31, 31)           test_grey_dilation_matches_scipy
erode_cross4_kernel / morph_kernel, iterations 1..4       test_erosion_cross_word_and_byte_paths
morph_kernel dilation mirror (p - s)                      test_erosion_and_closing_with_structures
correct_nan_ws_kernel at 9 and 11                         test_correct_nan_values_wide_windows
expand_kernel<0>, isolated_kernel, aligned16 == false     test_expand_every_path,
                                                            test_isolated_points_every_window
convolve_kernel, general odd weights                      test_convolve_general_weights_tight
"""
import numpy as np
import pytest
from scipy import ndimage

import hydrodem_amd as hd
from hydrodem_amd import backend
import oracle
from oracle import hdem_oracle_fourier as F
from oracle import hdem_oracle_lagoons as L
from test_gpu_parity import TOL, _groves_compare
from test_oracle_windows import sequential_fix

pytestmark = pytest.mark.gpu

# hdem_groves.hip, launch_ws: `if constexpr (WS == 15 || WS == 9 || WS == 3)` -- the
# streaming form; every other odd size up to WS_MAX takes the tiled groves_kernel<WS>
STREAM_WS = (3, 9, 15)
WS_MAX = 31                     # hdem_groves.hip `constexpr int WS_MAX = 31`
SW_COLS = 256                   # hdem_groves.hip `constexpr int SW_COLS = 256` (strip width)
STRIP_ROWS = range(96, 193)     # hdem_groves.hip launch_ws: `for (int cand = 96; cand <= 192`
WINDOWS = list(range(3, WS_MAX + 1, 2))


@pytest.fixture(scope="module", autouse=True)
def _lib(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


def _strips(W, mask_ptr=0):
    """(fx, sx) of hdem_groves.hip launch_ws: strip columns of the branch-free FULL form
    and in all; `fx = (W % 4 == 0 && ((uintptr_t)groves % 4 == 0)) ? W / SW_COLS : 0`."""
    fx = W // SW_COLS if W % 4 == 0 and mask_ptr % 4 == 0 else 0
    return fx, -(-W // SW_COLS)


def _at_offset(a, offset):
    """``a`` uploaded to device memory ``offset`` bytes past a 16-byte aligned address (a
    non-owning raster that keeps its buffer alive)."""
    a = np.ascontiguousarray(a)
    buf = backend.DeviceRaster.empty((1, a.nbytes + 64), np.uint8)
    assert buf.ptr % 16 == 0
    c = buf.ctx
    c.check(c.lib.hdem_memcpy_h2d(c.handle, buf.ptr + offset, a.ctypes.data, a.nbytes))
    return backend.DeviceRaster.wrap(buf.ptr + offset, a.shape, a.dtype, ctx=c, keepalive=buf)


def _bumpy_dem(h, w, seed=0):
    """Terrain with metre-scale bumps on 4 % of the cells: neighbouring windows fit
    different surfaces, and the groves threshold is crossed often."""
    rng = np.random.default_rng([h, w, seed])
    img = oracle.synth_dem(h, w)
    return (img + np.where(rng.random((h, w)) < 0.04, rng.uniform(1, 6, (h, w)), 0)
            ).astype(np.float32)


# --------------------------------------------------------------------------
# 1. QuadraticFilter and the groves pass at every odd window 3 .. 31
# --------------------------------------------------------------------------
PRIME_H = 601
FULL_AND_GENERAL_W = 1028      # W % 4 == 0, 256 < W, W % 256 != 0
ODD_W = 258                    # W % 4 != 0: every strip column takes the general form


@pytest.fixture(scope="module")
def prime_dem():
    return _bumpy_dem(PRIME_H, ODD_W)


def test_sweep_inputs_reach_their_branches(prime_dem):
    # the prime height leaves a short last strip at every strip height launch_ws may pick
    assert all(PRIME_H % rows for rows in STRIP_ROWS)
    assert _strips(ODD_W) == (0, 2)
    W = FULL_AND_GENERAL_W
    fx, sx = _strips(W)
    assert W % 4 == 0 and 256 < W and W % 256 and fx > 0 and sx > fx
    # neighbouring windows give answers far apart on these inputs
    for ws in WINDOWS:
        want = oracle.quadratic_exact64(prime_dem, ws)
        for other in (ws - 2, ws + 2):
            if 3 <= other <= WS_MAX:
                p = max(ws, other) // 2
                d = np.abs(oracle.quadratic_exact64(prime_dem, other) - want)[p:-p, p:-p]
                assert d.max() > 100 * TOL, (ws, other)


@pytest.mark.parametrize("ws", WINDOWS)
def test_quadratic_every_window(prime_dem, ws):
    cases = [prime_dem, _bumpy_dem(67, FULL_AND_GENERAL_W, ws), _bumpy_dem(ws, ws, ws),
             _bumpy_dem(ws, 300, ws), _bumpy_dem(300, ws, ws)]
    for dem in cases:
        want = oracle.quadratic_exact64(dem, ws)
        got = hd.QuadraticFilter(window_size=ws).apply(dem)
        err = np.abs(got.astype(np.float64) - want)
        assert err.max() <= TOL, (dem.shape, float(err.max()))
        # the device form, out of place
        dev = backend.quadratic_dev(backend.DeviceRaster.from_host(dem), ws).to_host()
        assert np.array_equal(dev, got), dem.shape


@pytest.mark.parametrize("ws", WINDOWS)
def test_groves_every_window(ws):
    """The fused pass (mask != null), three iterations, at every window: the prime-height
    raster (general strips only), FULL plus general strips in one launch, and a window-high
    and a window-wide raster."""
    for shape in [(PRIME_H, ODD_W), (67, FULL_AND_GENERAL_W), (ws, 300), (300, ws)]:
        img = _bumpy_dem(*shape, seed=ws + 1)
        groves = oracle.synth_groves(*shape).astype(np.uint8)
        want, stages = oracle.groves_exact64(img, groves, 3, ws=ws)
        if min(shape) > 2 * ws:
            assert stages[0][1].sum() > 0                 # the mask does something
        d = backend.groves_dev(backend.DeviceRaster.from_host(img),
                               backend.DeviceRaster.from_host(groves), window_size=ws,
                               iterations=3).to_host()
        excused = _groves_compare(d, want, [s[0] for s in stages])
        assert excused <= max(2, img.size // 20000), (shape, excused)
        host = backend.groves(img, groves, window_size=ws, iterations=3)
        assert np.array_equal(host, d)


@pytest.mark.parametrize("ws", [3, 9, 15, 11, 31])
def test_groves_misaligned_mask(ws):
    """The mask one byte past an aligned address while W % 4 == 0: the streaming launch
    runs every strip in the general form (fx = 0) instead of FULL strips.  Both forms do
    the same arithmetic per cell, so the result is the same bit for bit; the tiled kernel
    does not look at the alignment at all."""
    H, W = 133, 520
    img = _bumpy_dem(H, W, seed=ws)
    groves = oracle.synth_groves(H, W).astype(np.uint8)
    d_img = backend.DeviceRaster.from_host(img)
    aligned = backend.DeviceRaster.from_host(groves)
    shifted = _at_offset(groves, 1)
    if ws in STREAM_WS:
        assert _strips(W, aligned.ptr)[0] > 0 and _strips(W, shifted.ptr)[0] == 0
    a = backend.groves_dev(d_img, aligned, window_size=ws, iterations=3).to_host()
    b = backend.groves_dev(d_img, shifted, window_size=ws, iterations=3).to_host()
    assert np.array_equal(a, b)
    want, stages = oracle.groves_exact64(img, groves, 3, ws=ws)
    assert _groves_compare(b, want, [s[0] for s in stages]) <= 2


def test_window_33_is_refused_and_the_context_stays_usable():
    dem = _bumpy_dem(40, 50)
    with pytest.raises(ValueError):
        hd.QuadraticFilter(window_size=WS_MAX + 2).apply(dem)
    g = backend.DeviceRaster.from_host(oracle.synth_groves(40, 50).astype(np.uint8))
    with pytest.raises(ValueError):
        backend.groves_dev(backend.DeviceRaster.from_host(dem), g, window_size=WS_MAX + 2)
    got = hd.QuadraticFilter(window_size=9).apply(dem)
    assert np.abs(got - oracle.quadratic_exact64(dem, 9)).max() <= TOL


@pytest.mark.parametrize("ws", [9, 11, 21, 31])
def test_quadratic_against_the_reference_outputs(golden, ws):
    sz = golden("window_sweep.npz")
    got = hd.QuadraticFilter(window_size=ws).apply(sz["dem"])
    assert np.abs(got.astype(np.float64) - sz[f"quad{ws}"]).max() <= TOL


# --------------------------------------------------------------------------
# 2. grey dilation against scipy.ndimage.grey_dilation, bit for bit
# --------------------------------------------------------------------------
DILATION_SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (7, 5), (7, 7), (15, 3), (31, 31)]
DILATION_SHAPES = [(70, 97), (45, 130), (33, 65), (3, 5), (1, 40), (29, 1), (1, 1)]


def _dilation_input(shape, dtype):
    rng = np.random.default_rng(list(shape))
    if np.dtype(dtype).kind == "i":
        return rng.integers(-1000, 1000, shape).astype(dtype)
    return (rng.standard_normal(shape) * 100).astype(dtype)


def test_dilation_inputs_tell_sizes_apart():
    x = _dilation_input(DILATION_SHAPES[0], np.float32)
    for sy, sx in DILATION_SIZES:
        if sy != sx:
            assert not np.array_equal(ndimage.grey_dilation(x, size=(sy, sx)),
                                      ndimage.grey_dilation(x, size=(sx, sy)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
@pytest.mark.parametrize("size", DILATION_SIZES)
def test_grey_dilation_matches_scipy(size, dtype):
    for shape in DILATION_SHAPES:
        x = _dilation_input(shape, dtype)
        want = ndimage.grey_dilation(x, size=size)
        got = hd.GreyDilation(size=size).apply(x)
        assert got.dtype == want.dtype
        assert np.array_equal(got, want), (shape, size)


# --------------------------------------------------------------------------
# 3. binary erosion / closing against scipy.ndimage, bit for bit
# --------------------------------------------------------------------------
CROSS = ndimage.generate_binary_structure(2, 1)


def _structures():
    rng = np.random.default_rng(7)
    r7 = rng.random((7, 7)) < 0.5
    r7[3, 3] = False
    l3 = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], bool)
    return {"1x5": np.ones((1, 5), bool), "5x1": np.ones((5, 1), bool), "L3": l3,
            "rand7": r7, "ones5": np.ones((5, 5), bool)}


STRUCTS = _structures()


def _blobs(shape, seed=0, values=(1,)):
    """A mask of blobs and holes (both morphologies change it a lot), set cells carrying
    the byte values given."""
    rng = np.random.default_rng([seed, *shape])
    m = ndimage.binary_dilation(rng.random(shape) < 0.08, iterations=2)
    m &= ~(rng.random(shape) < 0.05)
    vals = np.asarray(values, np.uint8)[rng.integers(0, len(values), shape)]
    return np.where(m, vals, 0).astype(np.uint8)


def _erode(mask_dev, iterations, structure=None):
    return backend.binary_erosion_dev(mask_dev, iterations, structure).to_host()


def test_morphology_inputs_tell_answers_apart():
    m = _blobs((64, 92)) != 0
    for name, st in STRUCTS.items():
        if name in ("1x5", "5x1", "ones5"):
            continue                                   # symmetric on purpose
        mir = st[::-1, ::-1]
        assert not np.array_equal(ndimage.binary_closing(m, mir), ndimage.binary_closing(m, st))
        assert not np.array_equal(ndimage.binary_erosion(m, mir), ndimage.binary_erosion(m, st))
    for k in range(1, 5):
        assert not np.array_equal(ndimage.binary_erosion(m, iterations=k),
                                  ndimage.binary_erosion(m, iterations=k + 1))


@pytest.mark.parametrize("iterations", [1, 2, 3, 4])
def test_erosion_cross_word_and_byte_paths(iterations):
    """erode_n (hdem_lagoons.hip) takes erode_cross4_kernel when `cross && w % 4 == 0 &&
    ((uintptr_t)src | (uintptr_t)dst) % 4 == 0`, else morph_kernel: the same raster both
    ways (aligned, and one byte past an aligned address), and a width that is no multiple
    of 4.  Mask bytes 2, 128 and 255 are set cells too."""
    for shape in [(64, 92), (37, 200), (1, 64), (64, 1), (1, 61), (45, 77)]:
        m = _blobs(shape, iterations, values=(1, 2, 128, 255))
        want = ndimage.binary_erosion(m != 0, iterations=iterations)
        aligned = backend.DeviceRaster.from_host(m)
        shifted = _at_offset(m, 1)
        assert aligned.ptr % 4 == 0 and shifted.ptr % 4 == 1
        for dev in (aligned, shifted):
            got = _erode(dev, iterations)
            assert set(np.unique(got)) <= {0, 1}
            assert np.array_equal(got.view(bool), want), (shape, dev.ptr % 4)
        # the class's own path (default structure = the cross)
        got = hd.BinaryErosion(iterations=iterations).apply(m)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(STRUCTS))
def test_erosion_and_closing_with_structures(name):
    st = STRUCTS[name]
    for shape in [(64, 92), (45, 77), (1, 50), (50, 1)]:
        m = _blobs(shape, len(name), values=(1, 2, 128, 255))
        d = backend.DeviceRaster.from_host(m)
        for it in (1, 2):
            want = ndimage.binary_erosion(m != 0, st, iterations=it)
            assert np.array_equal(_erode(d, it, st).view(bool), want), (shape, it)
        want = ndimage.binary_closing(m != 0, st)
        got = backend.binary_closing_dev(d, st).to_host()
        assert np.array_equal(got.view(bool), want), shape
        assert np.array_equal(hd.BinaryClosing(structure=st).apply(m), want)


def test_structures_the_kernels_do_not_take():
    d = backend.DeviceRaster.from_host(_blobs((20, 24)))
    for st in (np.ones((9, 9), bool), np.ones((2, 3), bool), np.ones((3, 4), bool)):
        with pytest.raises(ValueError):
            backend.binary_erosion_dev(d, 1, st)
        with pytest.raises(ValueError):
            backend.binary_closing_dev(d, st)


# --------------------------------------------------------------------------
# 4. CorrectNANValues at windows 9 and 11
# --------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [9, 11])
def test_correct_nan_values_wide_windows(golden, ws):
    sz = golden("window_sweep.npz")
    hs = sz["hs"]
    want = L.correct_nan_values(hs, ws)
    assert np.array_equal(want, sz[f"fixed{ws}"], equal_nan=True)
    assert not np.array_equal(L.correct_nan_values(hs, ws - 2), want, equal_nan=True)
    assert not np.array_equal(sequential_fix(hs, ws), want, equal_nan=True)
    got = hd.CorrectNANValues(window_size=ws).apply(hs.copy())
    assert np.array_equal(got, want, equal_nan=True)
    dev = hd.CorrectNANValues(window_size=ws).apply_device(
        backend.DeviceRaster.from_host(hs)).to_host()
    assert np.array_equal(dev, want, equal_nan=True)
    # a second raster with different voids and a width that is no multiple of 4
    rng = np.random.default_rng(ws)
    hs2 = L.synth_hsheds(61, 83)
    hs2[rng.random(hs2.shape) < 0.3] = -9999.0
    hs2[20:40, 30:45] = -32768.0
    hs2 += np.where(hs2 >= 0, rng.uniform(0, 1, hs2.shape), 0).astype(np.float32)
    want2 = L.correct_nan_values(hs2, ws)
    assert not np.array_equal(sequential_fix(hs2, ws), want2, equal_nan=True)
    got2 = hd.CorrectNANValues(window_size=ws).apply_device(
        backend.DeviceRaster.from_host(hs2)).to_host()
    assert np.array_equal(got2, want2, equal_nan=True)


# --------------------------------------------------------------------------
# 5. ExpandFilter and IsolatedPoints, aligned and misaligned masks
# --------------------------------------------------------------------------
MARK_SHAPES = [(90, 110, 0.01), (64, 96, 0.01), (41, 203, 0.01), (120, 150, 0.0005)]


def _marks(shape, seed=0, density=0.01):
    """Scattered marks plus runs along rows and columns (they drive the incremental stores
    of expand_kernel), a block and border cells; sparse enough at the lowest density that
    a 31 x 31 window still sees single marks at its corners."""
    rng = np.random.default_rng([seed, *shape])
    h, w = shape
    m = (rng.random(shape) < density).astype(np.uint8)
    m[h // 4, 5:w // 2] = 1
    m[h // 3:h - 5, w // 2] = 1
    m[h // 2:h // 2 + 3, w - 20:w - 16] = 1
    m[h - 8, 2:5] = 1
    m[0, w // 3] = m[h - 1, 3] = m[h // 2, 0] = m[5, w - 1] = 1
    return m


# hdem_fourier.hip hdem_expand_u8_dev: reach 6 and 3 are compiled in, any other reach
# takes expand_kernel<0>; the 16-byte loads of for_nonzero need `aligned16(mask)`
EXPAND_COMPILED_REACH = (6, 3)


@pytest.mark.parametrize("ws", [3, 9, 11, 15, 21, 31, 7, 13])
def test_expand_every_path(golden, ws):
    for h, w, density in MARK_SHAPES:
        shape = (h, w)
        m = _marks(shape, ws, density)
        want = F.expand(m, ws).astype(np.uint8)
        assert not np.array_equal(F.expand(m, ws + 2), want)
        if density < 0.01:                   # the whole square, corners included, differs
            r = ws // 2
            square = F._box_sum((m > 0).astype(np.float64), ws) > 0.5
            assert (square[r:-r, r:-r] != want[r:-r, r:-r]).any()
        if ws > 3:
            assert not np.array_equal(F.expand(m, ws - 2), want)
        for offset in (0, 1, 4):
            d = _at_offset(m, offset)
            assert (d.ptr % 16 == 0) == (offset == 0)
            got = backend.expand_dev(d, ws).to_host()
            assert np.array_equal(got, want), (shape, offset)
    assert (ws // 2 in EXPAND_COMPILED_REACH) == (ws in (7, 13))
    if ws in (9, 21):
        sz = golden("window_sweep.npz")
        got = hd.ExpandFilter(window_size=ws).apply(sz["marks"].astype(np.float64))
        assert np.array_equal(got, sz[f"expand{ws}"])


@pytest.mark.parametrize("ws", [3, 5, 7, 11])
def test_isolated_points_every_window(golden, ws):
    for h, w, density in MARK_SHAPES[:3]:
        shape = (h, w)
        m = _marks(shape, ws, density)
        want = F.isolated_points(m, ws).astype(np.uint8)
        assert not np.array_equal(F.isolated_points(m, ws + 2), want)
        assert (want != m).any()
        for offset in (0, 1, 4):
            got = backend.isolated_points_dev(_at_offset(m, offset), ws).to_host()
            assert np.array_equal(got, want), (shape, offset)
    if ws == 5:
        sz = golden("window_sweep.npz")
        got = hd.IsolatedPoints(window_size=5).apply(sz["marks"].astype(np.float64))
        assert np.array_equal(got, sz["iso5"])


# --------------------------------------------------------------------------
# 6. general Convolve against scipy.ndimage.convolve
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wshape", [(1, 1), (1, 15), (15, 1), (3, 5), (7, 7), (15, 15)])
def test_convolve_general_weights_tight(wshape, dtype):
    rng = np.random.default_rng(list(wshape))
    w = rng.standard_normal(wshape)
    for shape in [(60, 70), (33, 129), (5, 7), (1, 9)]:
        x = oracle.synth_dem(max(shape[0], 16), max(shape[1], 16))[:shape[0], :shape[1]]
        x = np.ascontiguousarray(x, dtype=dtype)
        want = ndimage.convolve(x, w) / w.size
        got = hd.Convolve(w).apply(x)
        assert got.dtype == want.dtype == dtype
        if dtype == np.float32:
            bar = np.spacing(np.abs(want))              # one float32 ulp of the result
        else:
            bar = 4 * np.finfo(np.float64).eps * np.abs(want).max()
        assert (np.abs(got - want) <= bar).all(), (shape, float(np.abs(got - want).max()))
        # the flipped weights are a different answer on this raster
        if w.size > 1 and shape[0] > 1 and shape[1] > 1:
            assert not np.allclose(ndimage.convolve(x, w[::-1, ::-1]) / w.size, want)
