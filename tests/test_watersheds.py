"""
D8 watershed labelling (``Watersheds``, ``hdem_watershed_u8``): the CPU half.

The host references live here and are used by tests/test_gpu_watersheds.py:
  (a) ``labels_walk``      every cell walked to its stop one step at a time -- tiny grids;
  (b) ``labels_doubling``  pointer doubling on the flat receiver array, ceil(log2 n) + 1
                           rounds, ``ValueError`` if a cell has not reached a stop;
  (c) ``outlet_labels_hold``  the local property "a terminal cell holds its own index + 1,
                           every other cell holds its receiver's label", band by band -- any
                           size.  On acyclic codes it has one solution, so it is a proof.
A stop is a terminal cell or, with seeds, a seeded cell.  No GPU here: the references agree
with each other and with the flow-accumulation reference on basin areas, the operator is
importable from the package and the drop-in ``filters``, rejects what it must without a
device, and the library exports its entry points.
"""
import ctypes
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_flowacc import (CODE_OFFSETS, acc_kahn, random_acyclic_codes, receivers,
                          terminal_mask)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)]


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def _stops(codes, seeds):
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    stop = rec < 0
    if seeds is not None:
        seeds = np.asarray(seeds)
        assert seeds.shape == codes.shape
        stop = stop | (seeds.ravel() != 0)
    return codes, rec, stop


def _label_of(stop_cell, seeds):
    if seeds is None:
        return (stop_cell + 1).astype(np.uint32)
    return np.asarray(seeds).ravel()[stop_cell].astype(np.uint32)


def labels_walk(codes, seeds=None):
    """(a): all cells step down their paths together until each stands on a stop; a path
    longer than H*W cells is a cycle."""
    codes, rec, stop = _stops(codes, seeds)
    n = rec.size
    pos = np.arange(n, dtype=np.int64)
    for _ in range(n + 1):
        moving = ~stop[pos]
        if not moving.any():
            return _label_of(pos, seeds).reshape(codes.shape)
        pos[moving] = rec[pos[moving]]
    raise ValueError(f"flow directions form a cycle: {int(moving.sum())} cells never resolve")


def labels_doubling(codes, seeds=None):
    """(b): ptr <- ptr[ptr], a stop pointing at itself."""
    codes, rec, stop = _stops(codes, seeds)
    n = rec.size
    ptr = np.where(stop, np.arange(n, dtype=np.int64), rec)
    for _ in range(math.ceil(math.log2(n)) + 1):
        ptr = ptr[ptr]
    lost = ~stop[ptr]
    if lost.any():
        raise ValueError(f"flow directions form a cycle: {int(lost.sum())} cells never resolve")
    return _label_of(ptr, seeds).reshape(codes.shape)


def outlet_labels_hold(codes, labels, band=1024):
    """(c): (every cell satisfies the local property, number of terminal cells)."""
    codes = np.asarray(codes, dtype=np.uint8)
    h, w = codes.shape
    if labels.shape != codes.shape:
        return False, 0
    ok, terminals = True, 0
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        c = codes[r0:r1]
        # the label each cell must hold; a cell that no case below touches is terminal
        own = (np.arange(r0, r1, dtype=np.int64)[:, None] * w
               + np.arange(w, dtype=np.int64)[None, :] + 1)
        want = own.copy()
        has_receiver = np.zeros(want.shape, bool)
        for code, (dy, dx) in CODE_OFFSETS:
            y0, y1 = max(r0, -dy), min(r1, h - dy)       # rows whose receiver is inside
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            sel = c[y0 - r0:y1 - r0, x0:x1] == code
            tgt = labels[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            sub = want[y0 - r0:y1 - r0, x0:x1]
            sub[sel] = tgt[sel]
            has_receiver[y0 - r0:y1 - r0, x0:x1] |= sel
        terminals += int(has_receiver.size - has_receiver.sum())
        ok = ok and np.array_equal(want, labels[r0:r1])
    return ok, terminals


def random_seeds(shape, seed, every=50):
    """About one seeded cell per ``every`` cells (at least one), labels up to 2^32 - 1."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    seeds = np.zeros(n, np.uint32)
    where = rng.choice(n, size=max(1, n // every), replace=False)
    seeds[where] = rng.integers(1, 2 ** 32, size=where.size, dtype=np.uint64).astype(np.uint32)
    seeds[where[0]] = 2 ** 32 - 1
    return seeds.reshape(shape)


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    a, b = labels_walk(codes), labels_doubling(codes)
    assert a.dtype == b.dtype == np.uint32
    assert np.array_equal(a, b)
    term = terminal_mask(codes)
    flat = np.arange(codes.size).reshape(shape) + 1
    assert np.array_equal(b[term], flat[term]) and b.min() >= 1
    # basin areas are the flow accumulation at the outlets
    labels, counts = np.unique(b, return_counts=True)
    assert np.array_equal(labels, flat[term])
    assert np.array_equal(counts, acc_kahn(codes)[term])
    ok, terminals = outlet_labels_hold(codes, b, band=5)
    assert ok and terminals == int(term.sum())
    if codes.size > 1 and not term.all():
        wrong = b.copy()
        y, x = np.argwhere(~term)[0]
        wrong[y, x] = wrong[y, x] % codes.size + 1       # another cell's label
        assert not outlet_labels_hold(codes, wrong, band=5)[0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_references_agree_with_pour_points(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    seeds = random_seeds(shape, seed=shape[0] + shape[1], every=10)
    a, b = labels_walk(codes, seeds), labels_doubling(codes, seeds)
    assert np.array_equal(a, b)
    assert np.array_equal(b[seeds != 0], seeds[seeds != 0])      # a seed labels itself
    assert b.max() == 2 ** 32 - 1
    unseeded_terminal = terminal_mask(codes) & (seeds == 0)
    assert not b[unseeded_terminal].any()


def test_references_on_a_row_nested_seeds_and_cycles():
    row = np.full((1, 50), 1, np.uint8)
    assert np.array_equal(labels_walk(row)[0], np.full(50, 50))
    assert np.array_equal(labels_doubling(row)[0], np.full(50, 50))
    seeds = np.zeros((1, 50), np.uint32)
    seeds[0, 10], seeds[0, 30] = 7, 9                    # nested: upstream takes the upper
    want = np.array([7] * 11 + [9] * 20 + [0] * 19)
    assert np.array_equal(labels_walk(row, seeds)[0], want)
    assert np.array_equal(labels_doubling(row, seeds)[0], want)
    pair = np.array([[1, 16, 16]], np.uint8)             # E then W: a 2-cycle and a donor
    with pytest.raises(ValueError, match="3 cells never resolve"):
        labels_doubling(pair)
    with pytest.raises(ValueError, match="cycle"):
        labels_walk(pair)
    # a loop that holds a seeded cell resolves there
    seeds = np.array([[0, 5, 0]], np.uint32)
    assert np.array_equal(labels_doubling(pair, seeds), [[5, 5, 5]])
    assert np.array_equal(labels_walk(pair, seeds), [[5, 5, 5]])
    with pytest.raises(ValueError, match="2 cells never resolve"):
        labels_doubling(np.array([[1, 16, 0]], np.uint8), np.array([[0, 0, 5]], np.uint32))


# ---------------------------------------------------------------------------
# the operator without a device
# ---------------------------------------------------------------------------
def test_watersheds_is_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd.filters import custom_filters
    assert hd.Watersheds is custom_filters.Watersheds
    assert issubclass(hd.Watersheds, hd.Filter)
    assert hd.Watersheds.auto_device is True
    w = hd.Watersheds()
    assert w.labels == "outlet" and w.outlets is None and w.stats == {}


def test_watersheds_resolves_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import Watersheds
        import hydrodem_amd
        assert Watersheds is hydrodem_amd.Watersheds
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_watersheds_rejects_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    f = hd.Watersheds()
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    with pytest.raises(ValueError, match="uint8"):
        f.apply(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="2-D"):
        f.apply(np.zeros((2, 4, 4), np.uint8))
    with pytest.raises(ValueError, match=r"seeds are \(3, 4\)"):
        hd.Watersheds(pour_points=np.zeros((3, 4), np.uint32)).apply(codes)
    with pytest.raises(ValueError, match="integer dtype"):
        hd.Watersheds(pour_points=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="fit uint32"):
        hd.Watersheds(pour_points=np.full((4, 4), -1, np.int64))
    with pytest.raises(ValueError, match="fit uint32"):
        hd.Watersheds(pour_points=np.full((4, 4), 2 ** 32, np.int64))
    with pytest.raises(ValueError, match="2-D"):
        hd.Watersheds(pour_points=np.zeros(4, np.uint32))
    with pytest.raises(ValueError, match="label 0"):
        hd.Watersheds(pour_points=[(1, 1, 0)])
    with pytest.raises(ValueError, match="label"):
        hd.Watersheds(pour_points=[(1, 1, 2 ** 32)])
    with pytest.raises(ValueError, match="outside"):
        hd.Watersheds(pour_points=[(1, 1), (4, 0)]).apply(codes)
    with pytest.raises(ValueError, match="outside"):
        hd.Watersheds(pour_points=[(0, -1)]).apply(codes)
    with pytest.raises(ValueError, match=r"\(row, col\)"):
        hd.Watersheds(pour_points=[(1, 1, 1, 1)])
    with pytest.raises(ValueError, match="compact"):
        hd.Watersheds(pour_points=[(1, 1)], labels="compact")
    with pytest.raises(ValueError, match="labels is"):
        hd.Watersheds(labels="dense")
    # the backend's own checks come before the device too
    with pytest.raises(ValueError, match="uint32"):
        backend.watershed(codes, seeds=np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="compact"):
        backend.watershed(codes, seeds=np.zeros((4, 4), np.uint32), compact=True)


def test_pour_point_lists_become_seeds():
    import hydrodem_amd as hd
    w = hd.Watersheds(pour_points=[(0, 1), (2, 3), (1, 1, 2 ** 32 - 1)])
    seeds = w._host_seeds((3, 4))                        # pylint: disable=protected-access
    want = np.zeros((3, 4), np.uint32)
    want[0, 1], want[2, 3], want[1, 1] = 1, 2, 2 ** 32 - 1
    assert seeds.dtype == np.uint32 and np.array_equal(seeds, want)
    w = hd.Watersheds(pour_points=np.array([[0, 3], [2 ** 32 - 1, 0]], np.int64))
    assert np.array_equal(w._host_seeds((2, 2)),         # pylint: disable=protected-access
                          np.array([[0, 3], [2 ** 32 - 1, 0]], np.uint32))


def test_library_exports_the_watershed_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_watershed_u8") and hasattr(lib, "hdem_watershed_u8_dev")
    assert {"hdem_watershed_u8", "hdem_watershed_u8_dev"} <= set(backend.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    enums = dict(re.findall(r"\b(HDEM_K_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert int(enums["HDEM_K_COUNT"]) == 21              # the call has no kernel id
    written = re.search(r"\}\s*hdem_watershed_stats;\s*/\*\s*sizeof == (\d+)\s*\*/", header)
    assert written and ctypes.sizeof(backend.WatershedStats) == int(written.group(1))
    assert backend.WatershedStats.struct_size.offset == 0
    assert backend.WatershedStats().struct_size == ctypes.sizeof(backend.WatershedStats)
    assert int(re.search(r"#define HDEM_WS_COMPACT (\d+)", header).group(1)) == backend.WS_COMPACT
