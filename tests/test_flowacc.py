"""
D8 flow accumulation (``FlowAccumulation``, ``hdem_flowacc_u8``): the CPU half.

The three host references live here and are used by tests/test_gpu_flowacc.py:
  (a) ``acc_brute``   walk every cell's path (bounded by H*W steps) -- tiny grids;
  (b) ``acc_kahn``    NumPy Kahn peeling over a frontier -- up to 4096^2;
  (c) ``balanced``    the local balance ``acc == 1 + sum of the donors' acc`` in int64 over
                      8 shifted slices, row band by row band -- any size.  For acyclic codes
                      its solution is unique, so (c) alone proves a result exact.
No GPU here: the references agree with each other, the operator is importable from the
package and the drop-in ``filters``, rejects what it must without a device, and the
library exports its entry points.
"""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle.hdem_oracle_np import D8_CODES, D8_OFFSETS, d8_flow_direction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE_OFFSETS = tuple(zip(D8_CODES, D8_OFFSETS))      # (code, (dy, dx))


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def receivers(codes):
    """Flat receiver index of every cell, -1 where it is terminal (code 0 or pointing
    outside).  ValueError on a byte that is not a D8 code."""
    codes = np.asarray(codes, dtype=np.uint8)
    h, w = codes.shape
    valid = np.isin(codes, (0,) + D8_CODES)
    if not valid.all():
        raise ValueError(f"invalid D8 code in {int((~valid).sum())} cells")
    rec = np.full(h * w, -1, np.int64)
    yy, xx = np.indices((h, w), dtype=np.int64)
    for code, (dy, dx) in CODE_OFFSETS:
        ny, nx = yy + dy, xx + dx
        ok = (codes == code) & (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        rec[ok.ravel()] = (ny * w + nx)[ok]
    return rec


def acc_brute(codes):
    """(a): every cell's path walked to its end, all cells in step; a path longer than
    H*W cells is a cycle."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    acc = np.zeros(n, np.int64)
    pos = np.arange(n, dtype=np.int64)
    for _ in range(n):
        np.add.at(acc, pos, 1)
        pos = rec[pos]
        pos = pos[pos >= 0]
        if not pos.size:
            return acc.reshape(codes.shape)
    raise ValueError("flow directions form a cycle")


def acc_kahn(codes):
    """(b): peel the cells whose donors are all done, one frontier at a time."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    indeg = np.bincount(rec[rec >= 0], minlength=n)
    acc = np.ones(n, np.int64)
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        r = rec[frontier]
        keep = r >= 0
        f, r = frontier[keep], r[keep]
        np.add.at(acc, r, acc[f])
        np.subtract.at(indeg, r, 1)
        cand = np.unique(r)
        frontier = cand[indeg[cand] == 0]
    if done != n:
        raise ValueError(f"flow directions form a cycle: {n - done} cells never drain")
    return acc.reshape(codes.shape)


def balanced(codes, acc, band=1024):
    """(c): ``acc == 1 + sum(acc[d])`` over the donors d of every cell, in int64."""
    codes = np.asarray(codes, dtype=np.uint8)
    h, w = codes.shape
    if acc.shape != codes.shape:
        return False
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        want = np.ones((r1 - r0, w), np.int64)
        for code, (dy, dx) in CODE_OFFSETS:
            # donors at rows y with y + dy in [r0, r1), columns with x + dx inside
            y0, y1 = max(0, r0 - dy), min(h, r1 - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = np.where(codes[y0:y1, x0:x1] == code,
                           acc[y0:y1, x0:x1].astype(np.int64), 0)
            want[y0 + dy - r0:y1 + dy - r0, x0 + dx:x1 + dx] += src
        if not np.array_equal(want, acc[r0:r1].astype(np.int64)):
            return False
    return True


def terminal_mask(codes):
    return (receivers(codes) < 0).reshape(np.shape(codes))


def random_acyclic_codes(h, w, seed, ramp=False):
    """D8 of a random float raster (optionally on a tilted ramp, for long paths that cross
    tiles), with the border cells given random codes among: 0, pointing outside, pointing
    to a strictly lower neighbour.  Every step lowers z, so the codes are acyclic."""
    rng = np.random.default_rng(seed)
    z = rng.random((h, w), dtype=np.float32)
    if ramp:
        yy, xx = np.indices((h, w), dtype=np.float32)
        z = (yy + 0.7 * xx) * np.float32(0.5) + z
    codes = d8_flow_direction(z) if h > 2 and w > 2 else np.zeros((h, w), np.uint8)
    for y in range(h):
        xs = range(w) if y in (0, h - 1) else (0, w - 1) if w > 1 else (0,)
        for x in xs:
            choices = [0]
            for code, (dy, dx) in CODE_OFFSETS:
                ny, nx = y + dy, x + dx
                if not (0 <= ny < h and 0 <= nx < w) or z[ny, nx] < z[y, x]:
                    choices.append(code)
            codes[y, x] = choices[rng.integers(len(choices))]
    return codes


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    a = acc_brute(codes)
    b = acc_kahn(codes)
    assert np.array_equal(a, b)
    assert balanced(codes, b, band=5)
    assert a[terminal_mask(codes)].sum() == codes.size
    wrong = b.copy()
    wrong.flat[wrong.size // 2] += 1
    assert not balanced(codes, wrong, band=5)


def test_references_on_a_row_and_a_cycle():
    row = np.full((1, 50), 1, np.uint8)
    assert np.array_equal(acc_kahn(row)[0], np.arange(1, 51))
    assert np.array_equal(acc_brute(row)[0], np.arange(1, 51))
    pair = np.array([[1, 16]], np.uint8)                 # E then W: a 2-cycle
    with pytest.raises(ValueError):
        acc_kahn(pair)
    with pytest.raises(ValueError):
        acc_brute(pair)
    with pytest.raises(ValueError):
        receivers(np.array([[3]], np.uint8))


def test_random_codes_are_valid_and_reach_outside():
    codes = random_acyclic_codes(30, 30, seed=7)
    assert np.isin(codes, (0,) + D8_CODES).all()
    rec = receivers(codes)
    # some border cells point outside the raster (terminal although non-zero)
    assert ((rec < 0) & (codes.ravel() != 0)).any()


# ---------------------------------------------------------------------------
# the operator without a device
# ---------------------------------------------------------------------------
def test_flowaccumulation_is_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd.filters import custom_filters
    assert hd.FlowAccumulation is custom_filters.FlowAccumulation
    assert issubclass(hd.FlowAccumulation, hd.Filter)
    assert hd.FlowAccumulation.auto_device is True


def test_flowaccumulation_resolves_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import FlowAccumulation
        import hydrodem_amd
        assert FlowAccumulation is hydrodem_amd.FlowAccumulation
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_flowaccumulation_rejects_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    f = hd.FlowAccumulation()
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    with pytest.raises(ValueError, match="uint8"):
        f.apply(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        f.apply(np.zeros((2, 4, 4), np.uint8))


def test_library_exports_the_flowacc_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_flowacc_u8") and hasattr(lib, "hdem_flowacc_u8_dev")
    assert {"hdem_flowacc_u8", "hdem_flowacc_u8_dev"} <= set(backend.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    enums = dict(re.findall(r"\b(HDEM_K_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert int(enums["HDEM_K_FLOWACC"]) == backend.K_FLOWACC == 20
    assert int(enums["HDEM_K_COUNT"]) == 21
    # int64 + 3 int32 + 3 float
    assert ctypes.sizeof(backend.FlowAccStats) == 32
    assert backend.FlowAccStats.ms_tile.offset == 20
