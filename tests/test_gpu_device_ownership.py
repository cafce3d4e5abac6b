"""
The table of tests/test_device_ownership.py on the real library: the same calls on the same
small rasters, the same list holding every raster ``DeviceRaster.empty`` makes.  A call that
succeeds has freed what it did not hand over.  The failures are those the library itself
answers with a status code, before or after its kernels ran -- an even window, a window
larger than the raster, a byte that is no D8 code, the two-cell cycle ``[[E, W]]``, seeds of
another shape; nothing is injected.  After each of them the operator runs once on valid
input and gives the answer the other GPU tests hold it to, so a block that was freed on the
failure and comes back from the cache does no harm.
"""
import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend
from hydrodem_amd.filters import ComposedFilter, ComposedFilterResults
from oracle import c_oracle
from oracle import hdem_oracle_fourier as F
from oracle import hdem_oracle_lagoons as L
from test_device_ownership import ROWS, Tracker, _three, operands, run_row
from test_flats import resolve_flats_bfs
from test_flowacc import acc_kahn
from test_gpu_flowtrace import assert_same, reference
from test_watersheds import labels_doubling

pytestmark = pytest.mark.gpu
TOL = 1e-4      # metres: the quadratic filter and the destripe against their oracles


@pytest.fixture
def tracker(built, monkeypatch):
    assert backend.device_count() >= 1
    return Tracker(monkeypatch)


@pytest.mark.parametrize("row", [r for r in ROWS if not r.rejected],
                         ids=[r.name for r in ROWS if not r.rejected])
def test_a_call_frees_what_it_does_not_hand_over(row, tracker):
    run_row(row, tracker, False)


def _host(raster):
    with raster:
        return raster.to_host()


def _up(array):
    return backend.DeviceRaster.from_host(array)


def correct_nan(o):
    hs = o.hs.copy()
    assert hd.CorrectNANValues().apply(hs) is hs
    assert np.array_equal(hs, L.correct_nan_values(o.hs), equal_nan=True)


def majority(o):
    fixed = L.correct_nan_values(o.hs)
    want = L.majority_filter(fixed, 11)
    assert np.array_equal(hd.MajorityFilter(window_size=11).apply(fixed), want)
    with _up(fixed) as img:
        assert np.array_equal(_host(backend.majority_dev(img, 11)), want)


def destripe(o):
    want, want_mask, _ = F.detect_apply_fourier(o.striped)
    with _up(o.striped) as dem, _up(np.zeros(o.striped.shape, np.uint8)) as mask:
        got = _host(backend.fourier_destripe_dev(dem, mask=mask))
        assert np.array_equal(mask.to_host(), want_mask)
    assert np.abs(got - want).max() <= TOL
    with _up(o.striped) as dem:
        got = _host(hd.DetectApplyFourier().apply_device(dem))
    assert np.abs(got - want).max() <= TOL


def chain(cls):
    def check(o):
        members = _three(cls, hd.QuadraticFilter(window_size=15))
        smooth = c_oracle.boxmean3(o.dem, True)
        fitted = hd.QuadraticFilter(window_size=15).apply(smooth)
        assert np.abs(fitted - c_oracle.quadratic_ref(smooth, 15)).max() <= TOL
        with _up(o.dem) as dem:
            got = _host(members.apply_device(dem))
        assert np.array_equal(got, c_oracle.d8(fitted))
        if cls is ComposedFilterResults:
            assert np.array_equal(members.results["PostProcessingFinal"], smooth)
            assert np.array_equal(members.results["QuadraticFilter"], fitted)
            members.results.release()
    return check


def flowacc(o):
    with _up(o.codes) as codes:
        got, _ = backend.flowacc_dev(codes)
        assert np.array_equal(_host(got), acc_kahn(o.codes))


def watershed(seeded=False, compact=False):
    def check(o):
        seeds = o.seeds if seeded else None
        with _up(o.codes) as codes, backend.on_device(seeds) as d_seeds:
            got, outlets, _ = backend.watershed_dev(codes, d_seeds, compact)
        got = _host(got)
        if compact:                      # label k stands for the outlet outlets[k - 1]
            got = outlets[got.astype(np.int64) - 1].astype(np.int64) + 1
        assert np.array_equal(got, labels_doubling(o.codes, seeds))
    return check


def flowtrace(o):
    with _up(o.codes) as codes:
        got, _ = backend.flowtrace_dev(codes, want=("stop", "distance"))
    assert_same({name: _host(raster) for name, raster in got.items()}, reference(o.codes))


def resolve_flats(o):
    want_out, want_dist = resolve_flats_bfs(o.dem, o.codes)
    with _up(o.codes) as codes, _up(o.dem) as dem:
        out, dist, _ = backend.resolve_flats_dev(codes, dem, want_distance=True)
    assert np.array_equal(_host(out), want_out) and np.array_equal(_host(dist), want_dist)


def quadratic(o):
    with _up(o.dem) as dem:
        got = _host(backend.quadratic_dev(dem, 15))
    assert np.abs(got.astype(np.float64) - c_oracle.quadratic_ref(o.dem, 15)).max() <= TOL


# rejected row -> (what the library's status becomes, the operator on valid input)
REJECTED = {
    "CorrectNANValues.apply[even window]": (hd.WindowSizeEvenError, correct_nan),
    "MajorityFilter.apply[window too high]": (hd.WindowSizeHighError, majority),
    "DetectApplyFourier.apply_device[window too high]": (hd.WindowSizeHighError, destripe),
    "ComposedFilter.apply_device[the second member raises]":
        (hd.WindowSizeEvenError, chain(ComposedFilter)),
    "ComposedFilterResults.apply_device[the second member raises]":
        (hd.WindowSizeEvenError, chain(ComposedFilterResults)),
    "flowacc_dev[no D8 code]": (ValueError, flowacc),
    "flowacc_dev[cycle]": (ValueError, flowacc),
    "watershed_dev[compact, no D8 code]": (ValueError, watershed(compact=True)),
    "watershed_dev[cycle]": (ValueError, watershed()),
    "watershed_dev[seeds of another shape]": (ValueError, watershed(seeded=True)),
    "flowtrace_dev[no D8 code]": (ValueError, flowtrace),
    "flowtrace_dev[cycle]": (ValueError, flowtrace),
    "resolve_flats_dev[no D8 code]": (ValueError, resolve_flats),
    "majority_dev[even window]": (hd.WindowSizeEvenError, majority),
    "quadratic_dev[even window]": (hd.WindowSizeEvenError, quadratic),
}


def test_every_rejected_row_has_its_valid_call():
    assert set(REJECTED) == {row.name for row in ROWS if row.rejected}


@pytest.mark.parametrize("row", [r for r in ROWS if r.rejected],
                         ids=[r.name for r in ROWS if r.rejected])
def test_a_rejected_call_frees_everything_and_the_next_call_is_right(row, tracker):
    raises, valid = REJECTED[row.name]
    run_row(row, tracker, True, raises=raises)
    valid(operands())
