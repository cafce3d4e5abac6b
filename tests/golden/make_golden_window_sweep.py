"""
Regenerates tests/golden/window_sweep.npz.  RUNS ONLY IN THE BUILD CONTAINER (see
make_golden.py): outputs of the imported reference at window sizes its own pipeline never
uses -- QuadraticFilter(9, 11, 21, 31), CorrectNANValues(9, 11), ExpandFilter(9, 21) and
IsolatedPoints(5) -- on small seeded inputs, so that the oracles the window-sweep GPU tests
compare against (tests/test_gpu_window_sweep.py) are pinned at those sizes too
(tests/test_oracle_windows.py).

    python tests/golden/make_golden_window_sweep.py
"""
import os
import sys
import warnings

import numpy as np

REF = "/root/reference/cguerrero"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "hydrodem"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from filters.custom_filters import (QuadraticFilter, CorrectNANValues,  # noqa: E402
                                    ExpandFilter, IsolatedPoints)
from oracle.hdem_oracle_np import synth_dem  # noqa: E402
from oracle.hdem_oracle_lagoons import synth_hsheds  # noqa: E402


def sweep_inputs():
    """The seeded inputs (stored with the outputs)."""
    rng = np.random.default_rng(2026)
    # terrain with metre-scale bumps: neighbouring window sizes fit different surfaces
    dem = synth_dem(100, 120)
    dem = (dem + np.where(rng.random(dem.shape) < 0.05, rng.uniform(1, 4, dem.shape), 0)
           ).astype(np.float32)
    # voids: scattered, a region where most cells are void (windows with fewer than 8
    # valid values) and a 14 x 16 block where an 11 x 11 window holds none
    hs = synth_hsheds(80, 100)
    hs[rng.random(hs.shape) < 0.03] = -32768.0
    dense = rng.random((22, 30)) < 0.96
    hs[20:42, 30:60][dense] = -32768.0
    hs[52:66, 62:78] = -32768.0
    hs[8, 70] = np.nan
    # fractional elevations: sums of integer metres are exact in any order, these are not
    valid = hs >= 0
    hs[valid] += rng.uniform(0, 1, int(valid.sum())).astype(np.float32)
    # marks: runs along rows and columns, a block, isolated points, border cells
    m = (rng.random((90, 110)) < 0.01).astype(np.float64)
    m[20, 10:40] = 1
    m[50:80, 60] = 1
    m[30:33, 80:84] = 1
    m[70, 20:23] = 1
    m[0, 50] = m[89, 3] = m[45, 0] = m[12, 109] = 1
    return dem, hs, m


def main():
    warnings.simplefilter("ignore")
    dem, hs, m = sweep_inputs()
    out = {"dem": dem, "hs": hs, "marks": m.astype(np.uint8)}
    for ws in (9, 11, 21, 31):
        out[f"quad{ws}"] = QuadraticFilter(window_size=ws).apply(dem.copy())
        print("QuadraticFilter", ws, out[f"quad{ws}"].dtype)
    for ws in (9, 11):
        out[f"fixed{ws}"] = CorrectNANValues(window_size=ws).apply(hs.copy())
        print("CorrectNANValues", ws, "changed", int((out[f"fixed{ws}"] != hs).sum()),
              "NaN", int(np.isnan(out[f"fixed{ws}"]).sum()))
    for ws in (9, 21):
        out[f"expand{ws}"] = ExpandFilter(window_size=ws).apply(m.copy()).astype(np.uint8)
        print("ExpandFilter", ws, "set", int(out[f"expand{ws}"].sum()))
    out["iso5"] = IsolatedPoints(window_size=5).apply(m.copy()).astype(np.uint8)
    print("IsolatedPoints 5 cleared", int(m.sum() - out["iso5"].sum()))
    path = os.path.join(HERE, "window_sweep.npz")
    np.savez_compressed(path, **out)
    print("window_sweep.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
