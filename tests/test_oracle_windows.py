"""
The oracles of the window-sweep GPU tests (tests/test_gpu_window_sweep.py) against outputs
of the imported reference at window sizes its own pipeline never uses
(tests/golden/window_sweep.npz, make_golden_window_sweep.py).  CPU only.
"""
import numpy as np
import pytest

import oracle
from oracle import hdem_oracle_fourier as F
from oracle import hdem_oracle_lagoons as L


@pytest.fixture(scope="module")
def sz(golden):
    return golden("window_sweep.npz")


@pytest.mark.parametrize("ws", [9, 11, 21, 31])
def test_quadratic_exact64_within_reference_rounding(sz, ws):
    dem, want = sz["dem"], sz[f"quad{ws}"]
    got = oracle.quadratic_exact64(dem, ws)
    assert np.abs(got - want).max() < 1e-4            # the reference sums s1 in float32
    p = ws // 2                                       # border ring unchanged
    inner = np.ones(dem.shape, bool)
    inner[p:-p, p:-p] = False
    assert np.array_equal(want[inner], dem[inner])
    # the input tells this window from its neighbours
    for other in (ws - 2, ws + 2):
        assert np.abs(oracle.quadratic_exact64(dem, other)[15:-15, 15:-15] -
                      got[15:-15, 15:-15]).max() > 100 * 1e-4


def _valid_counts(hs, ws):
    """Valid (>= 0) neighbours of every centre whose ws x ws window fits."""
    ok = (hs >= 0).astype(np.int64)
    r = ws // 2
    h, w = hs.shape
    n = np.zeros((h - 2 * r, w - 2 * r), np.int64)
    for dy in range(ws):
        for dx in range(ws):
            n += ok[dy:dy + h - 2 * r, dx:dx + w - 2 * r]
    return n - ok[r:h - r, r:w - r]


def sequential_fix(hs, ws):
    """CorrectNANValues with the valid neighbours summed one by one from 0 in float32 --
    the plausible wrong order (NumPy sums 8 or more values in 8 running sums)."""
    out = np.array(hs, copy=True)
    r = ws // 2
    h, w = hs.shape
    for y, x in zip(*np.nonzero(hs[r:h - r, r:w - r] < 0)):
        win = hs[y:y + ws, x:x + ws].copy()
        win[r, r] = np.nan
        nb = win[win >= 0]
        s = np.float32(0)
        for v in nb:
            s = np.float32(s + v)
        out[y + r, x + r] = np.float32(float(s) / len(nb)) if len(nb) else np.nan
    return out


@pytest.mark.parametrize("ws", [9, 11])
def test_correct_nan_values_is_bit_exact(sz, ws):
    hs = sz["hs"]
    got = L.correct_nan_values(hs, ws)
    assert np.array_equal(got, sz[f"fixed{ws}"], equal_nan=True)
    # voids whose window holds no valid value, fewer than 8, and more than 8 but not a
    # multiple of 8 (every shape of NumPy's float32 sum)
    r = ws // 2
    void = hs[r:-r, r:-r] < 0
    n = _valid_counts(hs, ws)[void]
    assert (n == 0).any() and ((n > 0) & (n < 8)).any() and ((n > 8) & (n % 8 != 0)).any()
    assert np.isnan(got[r:-r, r:-r][void]).sum() == (n == 0).sum()
    # the input tells NumPy's summation order from the sequential one
    assert not np.array_equal(sequential_fix(hs, ws), got, equal_nan=True)


@pytest.mark.parametrize("ws", [9, 21])
def test_expand_is_bit_exact(sz, ws):
    got = F.expand(sz["marks"], ws)
    assert np.array_equal(got, sz[f"expand{ws}"])
    assert not np.array_equal(F.expand(sz["marks"], ws + 2), got)


def test_isolated_points_is_bit_exact(sz):
    m = sz["marks"]
    got = F.isolated_points(m, 5)
    assert np.array_equal(got, sz["iso5"])
    assert got.sum() < m.sum()
    assert not np.array_equal(F.isolated_points(m, 3), got)
