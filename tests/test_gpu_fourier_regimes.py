"""
The Fourier destripe where its kernels branch, on the MI355X: the inputs of
tests/fourier_cases.py against the float64 oracle (oracle/hdem_oracle_fourier.py on the raster
cast to float64).  tests/test_fourier_cases.py holds every predicate used here to the oracle
alone; in particular no case has a cell within 5 * FFT_RTOL * max|F| of its threshold in either
pass of either quadrant, so every mask comparison is ``np.array_equal`` with no excuse.

  300 x 1930   quadrant 140 x 955: three block columns, the middle one in the FULL form of
               hollow_detect4_body, five segments.  The second pass skips 7 of the 15 blocks of
               the first quadrant and all of the second.  The weak pair at (70, 305) is found
               only because the skip looks R rows above its segment, the one at (112, 462)
               only because it looks at the R columns of context left of its block's outputs;
               that one is found by a FULL block with ``total`` and a skip table.
  130 x 4000   quadrant 55 x 1990: five block columns, three of them FULL, one of those skipped
               in both segments, one finding a second-pass pair; 55 rows are the window itself
  4000 x 130   quadrant 1990 x 55: one block column of 63 segments, three of them visited
  130 x 130, 131 x 131, 130 x 131, 131 x 130
               the smallest rasters the destripe accepts, quadrants of exactly 55 x 55, both
               parities; striped terrain, second-pass peaks in the second quadrant
  1024 x 2048  2^21 cells: sum_partial_kernel reads every second cell and sum_final_kernel
               divides by the sampled count; the split inverse (powers of two)
  1031 x 2039  the same step with a last sample short of the end; rocFFT's 2-D inverse
  256 x 256, 300 x 1930, 141 x 155, 256 x 512, 512 x 256
               the state of one context (plans, work buffer, transposed intermediate, scratch,
               all keyed on the shape) across destripes and transforms of changing shape
  (1, 1) ... (1000, 2)
               FourierTransform / FourierITransform with a side of 1 or 2

Measured on the MI355X, error against the float64 oracle (bar):
  300 x 1930 2.0e-5 m, 130 x 4000 1.5e-5 m, 4000 x 130 1.0e-5 m (1.4e-4, 1.4e-4, 1.2e-4 m); the
  four smallest rasters 5.5e-6 ... 6.6e-6 m (1.1e-4 m)
  1024 x 2048 at 8 000 m: e32 4.215e-6 m, error 2.465e-4 m, bar 2.610e-4 m, of which half an ulp
                          of the output is 2.441e-4 m; at 100 m 7.4e-6 m (1.1e-4 m)
  1031 x 2039 at 8 000 m: e32 9.377e-6 m, error 2.506e-4 m, bar 2.817e-4 m; at 100 m 1.1e-5 m
  the split inverse against the 2-D plan at 256 x 256: 7.6e-6 m (2e-5 m)
Every degenerate shape is planned and transformed by rocFFT within FFT_RTOL: the wrappers needed
no other route and refuse none of them.

The value-only mutants of hdem_fourier.hip that were run against this file and
tests/test_gpu_fourier.py, each built once in a scratch copy and run once.  Each changes what
is computed and never an address: the two skip mutants read a sub-range of the occupancy
cells, the load mutant keeps the clamped address, the plans mutant is met only by shapes of
the same cell count AND the same quadrant and occupancy sizes (256 x 512 / 512 x 256,
130 x 4000 / 4000 x 130, 130 x 131 / 131 x 130, 2 x 1000 / 1000 x 2), so every buffer keeps its
size.  No HIP call failed under any of them, and all 15 tests of tests/test_gpu_fourier.py
passed under all five.
  the skip's rows without +- R (``r_lo = y0 >> 5, r_hi = (y1 - 1) >> 5``) -> 4 of 19:
      test_destripe_matches_the_oracle_where_the_detection_branches at 300 x 1930 (306 mask
      cells, from (64, 308): the dilated pair at (70, 305)), 130 x 4000 and 4000 x 130, and
      test_the_steps_alone_are_what_they_should_be at 300 x 1930
  the skip's columns from the output columns only -> 2: the same two tests at 300 x 1930 (356
      mask cells, from (106, 457): the pair at (112, 462))
  ``load4`` of the FULL form keeping a clamped row (``keep = want``) -> 5: the oracle test at
      300 x 1930 and 130 x 4000 (16 668 and 34 934 mask cells), both cases of
      test_destripe_level_from_every_second_cell (their masks) and the steps alone at
      300 x 1930; the rasters without a FULL block pass
  ``sum_final_kernel`` given ``n`` in place of the sampled count -> 2: both cases of
      test_destripe_level_from_every_second_cell, error 2.63e-3 m at 1024 x 2048 and 7.19e-3 m
      at 1031 x 2039 against bars of 2.6e-4 and 2.8e-4 m; masks and every other test pass
  ``ensure_plans`` keeping the state when H * W is unchanged -> 4: the oracle test at
      4000 x 130 (behind 130 x 4000) and 131 x 130 (behind 130 x 131),
      test_one_context_through_changing_shapes_and_transforms at step 10 (512 x 256 behind
      256 x 512) and test_transform_wrappers_with_a_side_of_one_or_two at 1000 x 2

Durations (``pytest --durations=0``, the file alone, 19 tests in 10.6 s of which the CPU oracle
is most): the two level cases 1.5 and 1.4 s; the oracle test 1.2, 0.9 and 0.7 s at the three
noise rasters and 0.6 s in all at the four smallest; the setup of the steps alone 0.9 s; the
seven degenerate shapes 2.5 s in all, which is rocFFT making plans; the changing shapes on one
context 0.17 s; the inverse switch 0.03 s.
"""
import contextlib
import functools

import numpy as np
import pytest
from scipy import fftpack

import filter_regimes as fr
import fourier_cases as fc
import hydrodem_amd as hd
from hydrodem_amd import backend

pytestmark = pytest.mark.gpu

FFT_RTOL = fc.FFT_RTOL
SPLIT_AGAINST_2D = 2e-5     # test_destripe_power_of_two_sizes_take_the_split_inverse


@pytest.fixture(scope="module", autouse=True)
def _lib(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


def by_shape(shape):
    return f"{shape[0]}x{shape[1]}"


@contextlib.contextmanager
def fresh_context():
    ctx = backend.Context()
    try:
        yield ctx
    finally:
        ctx.close()


def destripe_dev(ctx, dem):
    """(elevations, mask) of the device form, written into rasters of the caller's that held
    NaN and 0xFF: whatever comes back was written by the call."""
    with backend.DeviceRaster.from_host(dem, ctx=ctx) as d, \
            backend.DeviceRaster.from_host(np.full(dem.shape, np.nan, np.float32), ctx=ctx) as out, \
            backend.DeviceRaster.from_host(np.full(dem.shape, 0xFF, np.uint8), ctx=ctx) as mask:
        assert backend.fourier_destripe_dev(d, out=out, mask=mask) is out
        return out.to_host(), mask.to_host()


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        assert g.tobytes() == w.tobytes(), \
            f"{what}: result {k} differs in {int((g != w).sum())} cells"


# ---------------------------------------------------------------------------
# 1. wide, thin and smallest rasters against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.ORACLE_CASES)
def test_destripe_matches_the_oracle_where_the_detection_branches(name):
    case = fc.oracle_case(name)
    out, mask = backend.fourier_destripe(case.dem, return_mask=True)
    assert out.dtype == np.float32 and out.shape == case.shape and mask.dtype == np.uint8
    wrong = mask != case.mask
    assert not wrong.any(), f"{int(wrong.sum())} mask cells differ, the first at " \
                            f"{tuple(np.argwhere(wrong)[0])} (shifted coordinates)"
    err, bar = float(np.abs(out.astype(np.float64) - case.want).max()), fr.bar(case.dem)
    print(f"\n{name}: error {err:.3e} m against a bar of {bar:.3e} m")
    assert err <= bar
    # the device form into the caller's rasters, and the operator of the filter chain
    same_bytes(destripe_dev(backend.context(), case.dem), (out, mask), "device form")
    f = hd.DetectApplyFourier(keep_mask=True)
    got = f.apply(case.dem)
    assert f.mask.dtype == np.float64
    same_bytes((got, f.mask.astype(np.uint8)), (out, mask), "DetectApplyFourier")
    assert np.array_equal(f.mask, case.mask)


# ---------------------------------------------------------------------------
# 2. the level at step == 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fc.LEVEL_SHAPES, ids=by_shape)
def test_destripe_level_from_every_second_cell(shape):
    """From 2^21 cells on the level is the mean of every step-th cell, here every second one.
    At 8 000 m the error is the complex64 rounding of the transform of dem - level, which e32
    measures on the CPU's own complex64 chain, plus the rounding of the float32 output; the
    factor 4 is for rocFFT and fftpack being different algorithms of that precision.  A level
    of half the mean (the sum divided by all cells) is at 2.3e-3 and 8.0e-3 m in that chain
    (tests/test_fourier_cases.py).  The same raster at 100 m against the bar of the regimes."""
    assert fc.level_step(shape) == 2
    high, low = fc.LEVELS
    case = fc.level_case(shape, high)
    out, mask = backend.fourier_destripe(case.dem, return_mask=True)
    assert np.array_equal(mask, case.mask)
    e32 = fc.complex64_error(shape, high)
    half_ulp = 0.5 * fr.ulp_of_max(out)
    err, bar = float(np.abs(out.astype(np.float64) - case.want).max()), half_ulp + 4.0 * e32
    print(f"\n{by_shape(shape)} at {high:g} m: e32 {e32:.3e} m, error {err:.3e} m, bar {bar:.3e} m "
          f"(half an ulp of the output {half_ulp:.3e} m)")
    assert err <= bar
    case = fc.level_case(shape, low)
    out, mask = backend.fourier_destripe(case.dem, return_mask=True)
    assert np.array_equal(mask, case.mask)
    err, bar = float(np.abs(out.astype(np.float64) - case.want).max()), fr.bar(case.dem)
    print(f"{by_shape(shape)} at {low:g} m: error {err:.3e} m, bar {bar:.3e} m")
    assert err <= bar


# ---------------------------------------------------------------------------
# 3. the state a context keeps between Fourier calls
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spectrum_input(shape, dtype):
    rng = np.random.default_rng(shape[0])
    data = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    data.setflags(write=False)
    return data


def _destripe_step(shape):
    return lambda ctx: destripe_dev(ctx, fc.state_case(shape).dem)


def _transform_step(shape, dtype, directions):
    def run(ctx):
        got = []
        with backend.DeviceRaster.from_host(_spectrum_input(shape, dtype), ctx=ctx) as raster:
            for inverse in directions:
                assert backend.fft2_dev(raster, inverse=inverse) is raster
                got.append(raster.to_host())
        return tuple(got)
    return run


TRANSFORMS = {"forward 141x155": ((141, 155), np.complex64, (False,)),
              # the destripe's own shape: the state is kept and the plans are shared
              "forward, inverse 256x256": ((256, 256), np.complex64, (False, True)),
              # a plan of its own, made for the call
              "double 96x80": ((96, 80), np.complex128, (False, True))}
STEPS = {
    "destripe 256x256": _destripe_step((256, 256)),             # the split inverse
    "destripe 300x1930": _destripe_step((300, 1930)),           # larger scratch, state rebuilt
    "destripe 256x512": _destripe_step((256, 512)),
    "destripe 512x256": _destripe_step((512, 256)),             # the same cell count
    **{name: _transform_step(*args) for name, args in TRANSFORMS.items()},
}
ORDER = ("destripe 256x256", "destripe 300x1930", "destripe 256x256", "forward 141x155",
         "destripe 256x256", "forward, inverse 256x256", "destripe 256x256", "double 96x80",
         "destripe 256x256", "destripe 256x512", "destripe 512x256", "destripe 256x512",
         "destripe 256x256")


@pytest.fixture(scope="module")
def alone():
    """Every step's results from a fresh context of its own."""
    results = {}
    for name, step in STEPS.items():
        with fresh_context() as ctx:
            results[name] = step(ctx)
    return results


def test_the_steps_alone_are_what_they_should_be(alone):
    """The references of the next test against the oracle and fftpack, so that `the same as
    on a fresh context` means `right`."""
    for shape in fc.STATE_SHAPES + ((300, 1930),):
        case = fc.state_case(shape)
        out, mask = alone[f"destripe {by_shape(shape)}"]
        assert np.array_equal(mask, case.mask), shape
        assert np.abs(out.astype(np.float64) - case.want).max() <= fr.bar(case.dem), shape
    for name, (shape, dtype, directions) in TRANSFORMS.items():
        # (relative to the largest magnitude: the bar of test_fft_matches_fftpack, and for
        # double precision the same with float64's epsilon in place of float32's)
        rtol = FFT_RTOL if dtype == np.complex64 else FFT_RTOL * 2.0 ** -29
        data = _spectrum_input(shape, dtype)
        want = fftpack.fft2(data.astype(np.complex128))
        assert alone[name][0].dtype == dtype
        assert np.abs(alone[name][0] - want).max() <= rtol * np.abs(want).max(), name
        if len(directions) > 1:         # the inverse is unnormalised
            back = alone[name][1] / data.size
            assert np.abs(back - data).max() <= rtol * np.abs(data).max(), name


def test_one_context_through_changing_shapes_and_transforms(alone):
    with fresh_context() as ctx:
        for k, name in enumerate(ORDER):
            same_bytes(STEPS[name](ctx), alone[name], f"step {k}, {name}")


def test_the_2d_inverse_switch_is_read_on_every_call(alone, monkeypatch):
    """HDEM_FFT_2D_INVERSE is an experiment's switch read by every call: set for one call of
    three on one context, it changes that call alone, and only to rounding."""
    name = "destripe 256x256"
    with fresh_context() as ctx:
        same_bytes(STEPS[name](ctx), alone[name], "before")
        monkeypatch.setenv("HDEM_FFT_2D_INVERSE", "1")
        out, mask = STEPS[name](ctx)
        monkeypatch.delenv("HDEM_FFT_2D_INVERSE")
        assert np.array_equal(mask, alone[name][1])
        diff = float(np.abs(out.astype(np.float64) - alone[name][0]).max())
        print(f"\nsplit inverse against the 2-D plan: {diff:.3e} m")
        assert diff <= SPLIT_AGAINST_2D
        same_bytes(STEPS[name](ctx), alone[name], "after")
        monkeypatch.setenv("HDEM_FFT_2D_INVERSE", "1")
        with fresh_context() as other:
            same_bytes((out, mask), STEPS[name](other), "the 2-D inverse on a fresh context")


# ---------------------------------------------------------------------------
# 4. the transform wrappers at degenerate sides
# ---------------------------------------------------------------------------
DEGENERATE = ((1, 1), (1, 64), (64, 1), (2, 2), (3, 5), (2, 1000), (1000, 2))


@pytest.mark.parametrize("shape", DEGENERATE, ids=by_shape)
def test_transform_wrappers_with_a_side_of_one_or_two(shape):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(shape) * 10 + 100).astype(np.float32)
    want = fftpack.fft2(x.astype(np.float64))
    got = hd.FourierTransform().apply(x)
    assert got.dtype == np.complex64 and got.shape == shape
    assert np.abs(got - want).max() <= FFT_RTOL * np.abs(want).max()
    spec = want.astype(np.complex64)
    back = hd.FourierITransform().apply(spec)
    assert back.dtype == np.complex64 and back.shape == shape
    want_back = fftpack.ifft2(spec.astype(np.complex128))
    assert np.abs(back - want_back).max() <= FFT_RTOL * np.abs(want_back).max()
    assert np.abs(back.real - x).max() <= FFT_RTOL * np.abs(x).max()
