"""
Longest upstream D8 flow length (``UpstreamFlowLength``, ``hdem_upstream_u8``): the CPU half.

``up(c)``, the (cardinal, diagonal) steps of the longest D8 path that ends in ``c``, is
``(0, 0)`` for a cell without a donor and else the greatest ``up(d) + step(d)`` over the
donors ``d`` of ``c``; pairs are ordered by ``ncard + ndiag * sqrt(2)``, decided in integers.

The host references live here and are used by tests/test_gpu_upstream.py:
  ``longer``          the exact order, vectorised;
  ``upstream_kahn``   NumPy Kahn peeling over a frontier, the exact max per receiver;
  ``upstream_brute``  every cell walks down carrying its pair -- tiny grids;
  ``upstream_holds``  the local equation at every cell, row band by row band -- any size.  For
                      acyclic codes its solution is unique, so it alone proves a result exact.
No GPU here: the references agree with each other and tell a wrong order from the right one,
the operator is importable from the package and the drop-in ``filters``, rejects what it must
without a device, and the library exports its entry points.
"""
import ctypes
import math
import os
import subprocess
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest

from test_flowacc import CODE_OFFSETS, random_acyclic_codes, receivers
from test_flowtrace import distance_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAGONAL = (2, 8, 32, 128)
U32 = 2 ** 32 - 1


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def longer(a1, b1, a2, b2):
    """``a1 + b1 * sqrt(2) > a2 + b2 * sqrt(2)`` exactly, element by element: with
    ``da = a1 - a2`` and ``db = b1 - b2``, both >= 0: unless both are 0; both <= 0: no; mixed
    signs: ``da^2`` against ``2 db^2`` -- in int64 where that cannot overflow, in Python
    integers elsewhere."""
    da = np.asarray(a1).astype(np.int64) - np.asarray(a2).astype(np.int64)
    db = np.asarray(b1).astype(np.int64) - np.asarray(b2).astype(np.int64)
    shape = np.broadcast(da, db).shape
    da, db = np.broadcast_to(da, shape).ravel(), np.broadcast_to(db, shape).ravel()
    out = (da >= 0) & (db >= 0) & ((da | db) != 0)
    mixed = ((da > 0) & (db < 0)) | ((da < 0) & (db > 0))
    if mixed.any():
        small = mixed & (np.abs(da) < 2 ** 31) & (np.abs(db) < 2 ** 30)
        sa, sb = np.where(small, da, 0), np.where(small, db, 0)
        card = sa * sa > 2 * sb * sb
        out = np.where(small, np.where(da > 0, card, ~card), out)
        for at in np.flatnonzero(mixed & ~small):
            x, y = int(da[at]), int(db[at])
            out[at] = (x * x > 2 * y * y) == (x > 0)
    return out.reshape(shape)


# sqrt(2) between two fractions 1e-40 apart: |da + db sqrt(2)| >= 1 / (|da| + |db| sqrt(2))
# > 1e-11 for differences below 2^33, so the two bounds give the same sign
_ROOT2_LO = Fraction(math.isqrt(2 * 10 ** 80), 10 ** 40)
_ROOT2_HI = _ROOT2_LO + Fraction(1, 10 ** 40)


def longer_by_fractions(a1, b1, a2, b2):
    da, db = int(a1) - int(a2), int(b1) - int(b2)
    lo, hi = da + db * _ROOT2_LO, da + db * _ROOT2_HI
    if da == 0 and db == 0:
        return False
    assert (lo > 0) == (hi > 0) and lo != 0 and hi != 0
    return lo > 0


def steps_of(codes):
    """(cardinal, diagonal) step of every cell's code, flat int64 (a terminal cell's is not
    used)."""
    diag = np.isin(np.asarray(codes, np.uint8), DIAGONAL).ravel()
    return (~diag).astype(np.int64), diag.astype(np.int64)


def _raise_to(nc, nd, r, cand_c, cand_d, order=longer):
    """``(nc, nd)[r] = max(itself, candidate)`` for receivers ``r`` that may repeat: the
    candidates of one receiver are taken one at a time."""
    by = np.argsort(r, kind="stable")
    r, cand_c, cand_d = r[by], cand_c[by], cand_d[by]
    first = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    rank = np.arange(r.size) - np.repeat(first, np.diff(np.r_[first, r.size]))
    for k in range(int(rank.max()) + 1 if r.size else 0):
        sel = rank == k
        rr, cc, dd = r[sel], cand_c[sel], cand_d[sel]
        win = order(cc, dd, nc[rr], nd[rr])
        nc[rr[win]], nd[rr[win]] = cc[win], dd[win]


def upstream_kahn(codes, order=longer):
    """Peel the cells whose donors are all done, one frontier at a time, each receiver taking
    the greatest ``up(d) + step(d)`` in ``order``: (ncard, ndiag) as int64 rasters."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    sc, sd = steps_of(codes)
    n = rec.size
    indeg = np.bincount(rec[rec >= 0], minlength=n)
    nc, nd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        r = rec[frontier]
        keep = r >= 0
        f, r = frontier[keep], r[keep]
        _raise_to(nc, nd, r, nc[f] + sc[f], nd[f] + sd[f], order)
        np.subtract.at(indeg, r, 1)
        cand = np.unique(r)
        frontier = cand[indeg[cand] == 0]
    if done != n:
        raise ValueError(f"flow directions form a cycle: {n - done} cells never drain")
    return nc.reshape(codes.shape), nd.reshape(codes.shape)


def most_steps(a1, b1, a2, b2):
    """The wrong order that "the path with most steps wins" would be."""
    return (np.asarray(a1) + np.asarray(b1)) > (np.asarray(a2) + np.asarray(b2))


def upstream_brute(codes):
    """Every cell walks down its path carrying the steps taken so far, all cells in step, and
    leaves them wherever they beat what is there; a path longer than H*W cells is a cycle.
    Plain Python integers."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes).tolist()
    sc, sd = (s.tolist() for s in steps_of(codes))
    n = len(rec)
    up = [(0, 0)] * n
    walkers = [(c, 0, 0) for c in range(n)]
    for _ in range(n):
        moved = []
        for c, a, b in walkers:
            if rec[c] < 0:
                continue
            a, b, c = a + sc[c], b + sd[c], rec[c]
            da, db = a - up[c][0], b - up[c][1]
            if (da >= 0 and db >= 0 and (da or db)) or \
                    (da * db < 0 and (da * da > 2 * db * db) == (da > 0)):
                up[c] = (a, b)
            moved.append((c, a, b))
        walkers = moved
        if not walkers:
            nc = np.array([p[0] for p in up], np.int64).reshape(codes.shape)
            nd = np.array([p[1] for p in up], np.int64).reshape(codes.shape)
            return nc, nd
    raise ValueError("flow directions form a cycle")


def upstream_holds(codes, ncard, ndiag, band=1024):
    """``up(c) == max(up(d) + step(d))`` over the donors d of every cell, ``(0, 0)`` without
    one, in the exact order."""
    codes = np.asarray(codes, dtype=np.uint8)
    h, w = codes.shape
    if ncard.shape != codes.shape or ndiag.shape != codes.shape:
        return False
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        want_c = np.zeros((r1 - r0, w), np.int64)
        want_d = np.zeros((r1 - r0, w), np.int64)
        for code, (dy, dx) in CODE_OFFSETS:
            # donors at rows y with y + dy in [r0, r1), columns with x + dx inside
            y0, y1 = max(0, r0 - dy), min(h, r1 - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            gives = codes[y0:y1, x0:x1] == code
            diag = int(code in DIAGONAL)
            cc = ncard[y0:y1, x0:x1].astype(np.int64) + (1 - diag)
            dd = ndiag[y0:y1, x0:x1].astype(np.int64) + diag
            to = (slice(y0 + dy - r0, y1 + dy - r0), slice(x0 + dx, x1 + dx))
            win = gives & longer(cc, dd, want_c[to], want_d[to])
            want_c[to] = np.where(win, cc, want_c[to])
            want_d[to] = np.where(win, dd, want_d[to])
        if not (np.array_equal(want_c, ncard[r0:r1].astype(np.int64)) and
                np.array_equal(want_d, ndiag[r0:r1].astype(np.int64))):
            return False
    return True


def length_of(ncard, ndiag, cellsize=1.0):
    """The float32 length raster of the C ABI's definition."""
    cs = float(cellsize)
    return (ncard.astype(np.float64) * cs +
            ndiag.astype(np.float64) * (cs * np.sqrt(2.0))).astype(np.float32)


# ---------------------------------------------------------------------------
# the order
# ---------------------------------------------------------------------------
TRAPS = [((8119, 0), (0, 5741)), ((1393, 0), (0, 985)), ((8120, 0), (0, 5741)),
         ((U32, 0), (0, U32)), ((0, U32), (U32, 0)), ((U32, 0), (0, 3037000500)),
         ((U32, 0), (0, 3037000499)), ((U32, 1), (0, U32)), ((0, 0), (0, 0)),
         ((5, 7), (5, 7)), ((5, 7), (6, 7)), ((5, 8), (6, 7)), ((7, 5), (5, 6))]


def test_the_order_is_exact_where_float32_keys_tie():
    (a1, b1), (a2, b2) = TRAPS[0]
    assert length_of(np.array([a1]), np.array([b1])) == length_of(np.array([a2]), np.array([b2]))
    assert 5741 * 5741 * 2 > 8119 * 8119                      # 5741 sqrt(2) = 8119.00006
    assert longer(a2, b2, a1, b1) and not longer(a1, b1, a2, b2)
    assert longer(8120, 0, 0, 5741)
    assert longer(0, 985, 1393, 0) and not longer(1393, 0, 0, 985)    # 985 sqrt(2) = 1393.0004


def test_the_order_against_fractions():
    rng = np.random.default_rng(11)
    pairs = [(*p, *q) for p, q in TRAPS] + [(*q, *p) for p, q in TRAPS]
    for top in (4, 100, 2 ** 16, 2 ** 31, 2 ** 32):
        pairs += [tuple(int(v) for v in rng.integers(0, top, 4)) for _ in range(300)]
    # near-ties: a1 about b2 * sqrt(2)
    for b in rng.integers(1, 2 ** 32 // 2, 300):
        a = int(int(b) * math.sqrt(2.0))
        pairs += [(a + k, 0, 0, int(b)) for k in (-1, 0, 1, 2) if 0 <= a + k <= U32]
    q = np.array(pairs, dtype=np.int64)
    got = longer(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    want = [longer_by_fractions(*p) for p in pairs]
    assert got.tolist() == want
    for p, g in zip(pairs[:40], want[:40]):                    # and one pair at a time
        assert bool(longer(*p)) == g
    # antisymmetric, and translation-invariant: max(p, q) + s = max(p + s, q + s)
    back = longer(q[:, 2], q[:, 3], q[:, 0], q[:, 1])
    same = (q[:, 0] == q[:, 2]) & (q[:, 1] == q[:, 3])
    assert np.array_equal(got ^ back, ~same)
    small = q[(q < 2 ** 31).all(axis=1)]
    s = rng.integers(0, 2 ** 31, (small.shape[0], 2))
    assert np.array_equal(longer(small[:, 0], small[:, 1], small[:, 2], small[:, 3]),
                          longer(small[:, 0] + s[:, 0], small[:, 1] + s[:, 1],
                                 small[:, 2] + s[:, 0], small[:, 3] + s[:, 1]))


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    a = upstream_brute(codes)
    b = upstream_kahn(codes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert upstream_holds(codes, *b, band=5)
    if codes.size > 1 and (b[0] + b[1]).any():
        at = np.unravel_index(np.argmax(b[0] + b[1]), codes.shape)
        for k in (0, 1):
            wrong = [b[0].copy(), b[1].copy()]
            wrong[k][at] += 1
            assert not upstream_holds(codes, *wrong, band=5)


def test_references_on_a_row_a_diagonal_and_a_cycle():
    row = np.full((1, 50), 1, np.uint8)
    for ref in (upstream_kahn, upstream_brute):
        nc, nd = ref(row)
        assert np.array_equal(nc[0], np.arange(50)) and not nd.any()
        nc, nd = ref(np.full((30, 40), 2, np.uint8))          # all SE
        yy, xx = np.indices((30, 40))
        assert np.array_equal(nd, np.minimum(yy, xx)) and not nc.any()
        with pytest.raises(ValueError):
            ref(np.array([[1, 16]], np.uint8))                 # E then W: a 2-cycle
    assert upstream_holds(row, np.arange(50)[None, :], np.zeros((1, 50), np.int64))
    assert not upstream_holds(row, np.arange(50)[None, :], np.zeros((2, 50), np.int64))
    with pytest.raises(ValueError):
        upstream_kahn(np.array([[3]], np.uint8))


@pytest.mark.parametrize("shape,changed", [((65, 65), 986), ((4097, 300), 257921)])
def test_most_steps_wins_is_detectably_wrong(shape, changed):
    """A diagonal step is worth sqrt(2) cardinal ones: choosing the donor by the number of
    steps gives other pairs, which the exact references and the local equation tell apart."""
    codes = random_acyclic_codes(*shape, seed=shape[0] * 7 + shape[1], ramp=True)
    right = upstream_kahn(codes)
    wrong = upstream_kahn(codes, order=most_steps)
    differ = (right[0] != wrong[0]) | (right[1] != wrong[1])
    print("cells that differ:", int(differ.sum()))
    assert differ.sum() > 0
    assert int(differ.sum()) == changed
    assert upstream_holds(codes, *right)
    assert not upstream_holds(codes, *wrong)


def test_the_length_formula_is_the_flow_traces():
    rng = np.random.default_rng(3)
    nc = rng.integers(0, 2 ** 32, (40, 50)).astype(np.uint32)
    nd = rng.integers(0, 2 ** 32, (40, 50)).astype(np.uint32)
    nc[0, :4], nd[0, :4] = (8119, 0, 1, 0), (0, 5741, 0, 1)
    stop = np.ones(nc.shape, np.uint32)
    for cs in (1.0, 30.0, 0.1):
        assert np.array_equal(length_of(nc, nd, cs), distance_of(stop, nc, nd, cs))
    assert length_of(nc, nd).dtype == np.float32


# ---------------------------------------------------------------------------
# the operator without a device
# ---------------------------------------------------------------------------
def test_the_operator_is_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd import upstream
    from hydrodem_amd.filters import custom_filters
    assert hd.UpstreamFlowLength is custom_filters.UpstreamFlowLength
    assert issubclass(hd.UpstreamFlowLength, hd.Filter)
    assert hd.UpstreamFlowLength.auto_device is True
    f = hd.UpstreamFlowLength()
    assert f.cellsize == 1.0 and f.keep_partial_results is False
    assert f.stats == {} and f.ncard is None and f.ndiag is None
    with pytest.raises(TypeError):
        hd.UpstreamFlowLength(30.0)                            # keyword-only
    assert {"upstream_args", "upstream", "upstream_dev"} <= set(dir(upstream))


def test_the_operator_resolves_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import UpstreamFlowLength
        import hydrodem_amd
        assert UpstreamFlowLength is hydrodem_amd.UpstreamFlowLength
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operator_rejects_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend, upstream

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    f = hd.UpstreamFlowLength()
    with pytest.raises(hd.NumpyArrayExpectedError):
        f.apply([[1, 2], [4, 8]])
    ctx = backend.Context.__new__(backend.Context)             # a context that is never used
    ctx.lib, ctx.handle, ctx.device = None, ctypes.c_void_p(1), 0
    for form, wrap in (("apply", lambda a: a),
                       ("apply_device",
                        lambda a: backend.DeviceRaster.wrap(0x10000, a.shape, a.dtype, ctx=ctx))):
        run = getattr(f, form)
        with pytest.raises(ValueError, match="uint8 D8 codes, got float32"):
            run(wrap(np.zeros((4, 4), np.float32)))
        with pytest.raises(ValueError, match="a 2-D raster, got 3 dimensions"):
            run(wrap(np.zeros((2, 4, 4), np.uint8)))
        with pytest.raises(ValueError, match="a 2-D raster, got 1 dimensions"):
            run(wrap(np.zeros(4, np.uint8)))
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cellsize must be finite and positive"):
            hd.UpstreamFlowLength(cellsize=bad)
        g = hd.UpstreamFlowLength()
        g.cellsize = bad                                       # a mutable operand attribute
        with pytest.raises(ValueError, match="cellsize must be finite and positive"):
            g.apply(codes)
        with pytest.raises(ValueError, match="cellsize must be finite and positive"):
            upstream.upstream(codes, cellsize=bad)
    with pytest.raises(ValueError, match="cellsize is a number"):
        hd.UpstreamFlowLength(cellsize="wide")
    with pytest.raises(ValueError, match="unknown upstream flow length outputs"):
        upstream.upstream(codes, want=("length", "source"))
    with pytest.raises(ValueError, match="no output wanted"):
        upstream.upstream(codes, want=())
    with pytest.raises(ValueError, match="codes is a NumPy array"):
        upstream.upstream([[1]])


def test_library_exports_the_upstream_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_upstream_u8") and hasattr(lib, "hdem_upstream_u8_dev")
    assert backend.SIGNATURES["hdem_upstream_u8"] == backend.SIGNATURES["hdem_upstream_u8_dev"]
    stats = backend._UpstreamStats                  # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 48
    assert stats().struct_size == 48
    assert stats.exits.offset == 8 and stats.heads.offset == 16 and stats.ms_tile.offset == 32
    assert set(stats().as_dict()) == {"max_hops", "exits", "heads", "tile_h", "tile_w",
                                      "ms_tile", "ms_forest", "ms_final"}
    # no kernel id of its own
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    assert "HDEM_K_UPSTREAM" not in header and "sizeof == 48" in header
