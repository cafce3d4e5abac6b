"""
Weighted D8 flow accumulation (``WeightedFlowAccumulation``, ``hdem_flowsum_u8``): the CPU half.

The host references live here and are used by tests/test_gpu_flowsum.py:
  (a) ``wsum_brute``  walk every cell's path (bounded by H*W steps), adding the cell's own
                      quantised weight to every cell on it -- tiny grids;
  (b) ``wsum_kahn``   NumPy Kahn peeling over a frontier, int64 -- any size a test uses.
No GPU here: the references agree with each other, the quantiser gives the hand values of the
contract, the operator is importable from the package and the drop-in ``filters``, rejects
what it must without a device, and the header and the library carry the entry points.
"""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_flowacc import acc_kahn, random_acyclic_codes, receivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def wsum_brute(codes, q):
    """(a): every cell carries its own weight down its path, all cells in step; a path longer
    than H*W cells is a cycle."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    total = np.zeros(n, np.int64)
    pos = np.arange(n, dtype=np.int64)
    carried = np.asarray(q, dtype=np.int64).ravel().copy()
    for _ in range(n):
        np.add.at(total, pos, carried)
        pos = rec[pos]
        keep = pos >= 0
        pos, carried = pos[keep], carried[keep]
        if not pos.size:
            return total.reshape(codes.shape)
    raise ValueError("flow directions form a cycle")


def wsum_kahn(codes, q):
    """(b): peel the cells whose donors are all done, one frontier at a time; int64."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    n = rec.size
    indeg = np.bincount(rec[rec >= 0], minlength=n)
    total = np.asarray(q, dtype=np.int64).ravel().copy()
    assert total.size == n
    frontier = np.flatnonzero(indeg == 0)
    done = 0
    while frontier.size:
        done += frontier.size
        r = rec[frontier]
        keep = r >= 0
        f, r = frontier[keep], r[keep]
        np.add.at(total, r, total[f])
        np.subtract.at(indeg, r, 1)
        cand = np.unique(r)
        frontier = cand[indeg[cand] == 0]
    if done != n:
        raise ValueError(f"flow directions form a cycle: {n - done} cells never drain")
    return total.reshape(codes.shape)


def downstream_union(codes, cells):
    """The mask of every cell on the D8 path of one of ``cells`` (flat indices), the cells
    themselves included, walked one path at a time."""
    rec = receivers(codes)
    mask = np.zeros(rec.size, np.uint8)
    for c in cells:
        steps = 0
        while c >= 0 and steps <= rec.size:
            mask[c] = 1
            c = rec[c]
            steps += 1
    return mask.reshape(np.shape(codes))


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 3), (17, 23), (40, 9), (9, 40)])
@pytest.mark.parametrize("ramp", [False, True])
def test_references_agree_on_random_acyclic_codes(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    rng = np.random.default_rng(shape[0] + 31 * shape[1])
    q = rng.integers(0, 2 ** 31, size=shape, dtype=np.int64)
    a, b = wsum_brute(codes, q), wsum_kahn(codes, q)
    assert a.dtype == b.dtype == np.int64
    assert np.array_equal(a, b)
    # every weight ends in exactly one terminal cell
    assert int(b.ravel()[receivers(codes) < 0].sum()) == int(q.sum())
    ones = np.ones(shape, np.int64)
    assert np.array_equal(wsum_kahn(codes, ones), acc_kahn(codes))
    assert np.array_equal(wsum_brute(codes, ones), acc_kahn(codes))


def test_references_on_a_row_a_cycle_and_marked_points():
    row = np.full((1, 50), 1, np.uint8)
    q = np.full((1, 50), 2 ** 31 - 1, np.int64)
    want = np.arange(1, 51, dtype=np.int64) * (2 ** 31 - 1)
    assert np.array_equal(wsum_kahn(row, q)[0], want)
    assert np.array_equal(wsum_brute(row, q)[0], want)
    assert want[-1] > 2 ** 32
    pair = np.array([[1, 16]], np.uint8)                 # E then W: a 2-cycle
    with pytest.raises(ValueError):
        wsum_kahn(pair, np.ones((1, 2), np.int64))
    with pytest.raises(ValueError):
        wsum_brute(pair, np.ones((1, 2), np.int64))
    codes = random_acyclic_codes(30, 41, seed=11, ramp=True)
    cells = np.random.default_rng(2).choice(codes.size, 5, replace=False)
    marks = np.zeros(codes.size, np.int64)
    marks[cells] = 1
    assert np.array_equal(wsum_kahn(codes, marks.reshape(codes.shape)) >= 1,
                          downstream_union(codes, cells) == 1)


# ---------------------------------------------------------------------------
# the quantiser, against hand values
# ---------------------------------------------------------------------------
def f32(*values):
    return np.array(values, np.float32)


def test_the_quantiser_rounds_once_to_nearest_even():
    from hydrodem_amd import flowsum
    assert flowsum.Q_MAX == 2 ** 31 - 1
    q = flowsum.quantise(f32(0.5, 1.5, 2.5, 3.5, 0.49999997, 2.5000002), 0)
    assert q.dtype == np.int64 and q.tolist() == [0, 2, 2, 4, 0, 3]
    # ties at frac_bits 16: (k + 0.5) / 65536 is exact in float32
    ties = f32(0.5 / 65536, 1.5 / 65536, 2.5 / 65536, (2 ** 20 + 0.5) / 65536,
               (2 ** 20 + 1.5) / 65536)
    assert flowsum.quantise(ties, 16).tolist() == [0, 2, 2, 2 ** 20, 2 ** 20 + 2]
    assert flowsum.quantise(f32(1.0, 0.1, 99.99), 16).tolist() == \
        [65536, 6554, int(np.rint(np.float64(np.float32(99.99)) * 65536))]
    assert flowsum.quantise(f32(1.0), 30).tolist() == [2 ** 30]
    # the float32 0.1 is 13421773 * 2^-27: its product with 2^30 is an integer already
    assert flowsum.quantise(f32(0.1), 30).tolist() == [13421773 * 8]


def test_the_quantiser_on_negative_zero_nan_and_the_bound():
    from hydrodem_amd import flowsum
    q = flowsum.quantise(f32(-0.0, 0.0, np.nan), 16)
    assert q.tolist() == [0, 0, 0]
    # the float32 neighbours of 2^31 at frac_bits 0, and of 2^15 at frac_bits 16
    below, at = np.nextafter(np.float32(2 ** 31), np.float32(0)), np.float32(2 ** 31)
    assert flowsum.quantise(f32(below, at), 0).tolist() == [2 ** 31 - 128, 2 ** 31]
    assert 2 ** 31 - 128 <= flowsum.Q_MAX < 2 ** 31
    below = np.nextafter(np.float32(2 ** 15), np.float32(0))
    q = flowsum.quantise(f32(below, 2 ** 15), 16).tolist()
    assert below == (2 ** 24 - 1) / 2.0 ** 9
    assert q == [2 ** 31 - 128, 2 ** 31] and q[0] <= flowsum.Q_MAX < q[1]
    # integer weights are taken as they are, on both sides of the bound
    q = flowsum.quantise(np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32))
    assert q.dtype == np.int64 and q.tolist() == [0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    assert q[1] <= flowsum.Q_MAX < q[2]
    assert flowsum.quantise(np.array([0, 255], np.uint8)).tolist() == [0, 255]


def test_the_threshold_in_units_of_q():
    from hydrodem_amd import flowsum
    assert flowsum.threshold_units(1, 0) == 1
    assert flowsum.threshold_units(2.5, 0) == 3
    assert flowsum.threshold_units(2.5, 16) == 163840
    assert flowsum.threshold_units(2.0 ** -16, 16) == 1
    assert flowsum.threshold_units(2.0 ** -17, 16) == 1            # ceil
    for bad in (0, -1, float("nan"), float("inf"), 2.0 ** 63):
        with pytest.raises(ValueError, match="threshold"):
            flowsum.threshold_units(bad, 0)
    with pytest.raises(ValueError, match="threshold is a number"):
        flowsum.threshold_units("high", 0)


# ---------------------------------------------------------------------------
# the operator without a device
# ---------------------------------------------------------------------------
def test_the_operator_is_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd import flowsum
    from hydrodem_amd.filters import custom_filters
    assert hd.WeightedFlowAccumulation is custom_filters.WeightedFlowAccumulation
    assert issubclass(hd.WeightedFlowAccumulation, hd.Filter)
    assert hd.WeightedFlowAccumulation.auto_device is True
    assert {"flowsum_args", "flowsum", "flowsum_dev"} <= set(dir(flowsum))
    w = np.ones((4, 4), np.float32)
    f = hd.WeightedFlowAccumulation(w)
    assert f.frac_bits == 16 and f.output == "value" and f.threshold is None
    assert f.dtype == np.float32 and f.stats == {} and f.weights is w
    assert hd.WeightedFlowAccumulation(w, output="sum").dtype == np.int64
    assert hd.WeightedFlowAccumulation(w, 16, "mask", 2.5).dtype == np.uint8
    assert hd.WeightedFlowAccumulation(w.astype(np.uint8), 0, "sum").dtype == np.int64
    assert hd.WeightedFlowAccumulation(w.astype(np.uint32), frac_bits=0).dtype == np.float32
    # FlowAccumulation is what it was
    assert hd.FlowAccumulation().stats == {}


def test_the_operator_resolves_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import WeightedFlowAccumulation
        import hydrodem_amd
        assert WeightedFlowAccumulation is hydrodem_amd.WeightedFlowAccumulation
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operator_rejects_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend, flowsum

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    w = np.ones((4, 4), np.float32)
    make = hd.WeightedFlowAccumulation
    with pytest.raises(ValueError, match="needs the weights"):
        make(None)
    with pytest.raises(ValueError, match="weights is a NumPy array or a DeviceRaster"):
        make([[1.0]])
    with pytest.raises(ValueError, match="got float64"):
        make(w.astype(np.float64))                              # refused, not narrowed
    with pytest.raises(ValueError, match="got int32"):
        make(w.astype(np.int32))
    with pytest.raises(ValueError, match="weights is a 2-D raster"):
        make(np.ones(4, np.float32))
    for bad in (-1, 31, 1.5, True, None):
        with pytest.raises(ValueError, match="frac_bits is an integer in 0 ... 30"):
            make(w, frac_bits=bad)
    with pytest.raises(ValueError, match="integer weights take frac_bits 0, got 16"):
        make(w.astype(np.uint8))
    with pytest.raises(ValueError, match="integer weights take frac_bits 0, got 1"):
        make(w.astype(np.uint32), 1)
    with pytest.raises(ValueError, match="output is one of"):
        make(w, output="mean")
    with pytest.raises(ValueError, match="output is one of"):
        make(w, output=("sum", "value"))
    with pytest.raises(ValueError, match="mask needs a threshold"):
        make(w, output="mask")
    with pytest.raises(ValueError, match="a threshold goes with the mask"):
        make(w, output="sum", threshold=3)
    for bad in (0, -2.0, 2.0 ** -18, float("nan")):            # ceil(2^-18 * 2^16) = 1 is fine
        if bad == 2.0 ** -18:
            assert make(w, 16, "mask", bad).threshold == bad
            continue
        with pytest.raises(ValueError, match="threshold"):
            make(w, 16, "mask", bad)

    f = make(w)
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
        with pytest.raises(ValueError, match=r"the weights are \(4, 4\), the codes \(4, 5\)"):
            run(wrap(np.zeros((4, 5), np.uint8)))
        g = make(w)
        g.frac_bits = 31                                       # a mutable operand attribute
        with pytest.raises(ValueError, match="frac_bits is an integer in 0 ... 30"):
            getattr(g, form)(wrap(codes))
    with pytest.raises(ValueError, match="unknown weighted flow accumulation outputs"):
        flowsum.flowsum(codes, w, want=("sum", "mean"))
    with pytest.raises(ValueError, match="no output wanted"):
        flowsum.flowsum(codes, w, want=())
    with pytest.raises(ValueError, match="codes is a NumPy array"):
        flowsum.flowsum([[1]], w)
    with pytest.raises(ValueError, match="weights is a NumPy array"):
        flowsum.flowsum(codes, [[1.0]])
    assert flowsum.flowsum_args(codes, w, 16, ("mask", "sum"), 1.5) == \
        (1, 16, 98304, ("sum", "mask"))
    assert flowsum.flowsum_args(codes, w.astype(np.uint32), 0, "value", None) == \
        (2, 0, 0, ("value",))
    assert flowsum.flowsum_args(codes, w.astype(np.uint8), 0, "sum", None)[0] == 3


# ---------------------------------------------------------------------------
# the header and the library
# ---------------------------------------------------------------------------
def test_the_header_declares_the_entry_points():
    from hydrodem_amd import backend, flowsum
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("hdem_flowsum_u8", "hdem_flowsum_u8_dev"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", plain)
        assert proto, name
        args = [" ".join(a.split()) for a in proto.group(1).split(",")]
        assert args == ["hdem_ctx *ctx", "const uint8_t *d8", "int H", "int W",
                        "const void *weights", "int weight_type", "int frac_bits",
                        "int64_t threshold", "int64_t *sum", "float *value", "uint8_t *mask",
                        "hdem_flowsum_stats *stats"]
        assert len(backend.SIGNATURES[name]) == len(args)
    assert backend.SIGNATURES["hdem_flowsum_u8"] == backend.SIGNATURES["hdem_flowsum_u8_dev"]
    types = {k: int(v) for k, v in re.findall(r"\b(HDEM_FLOWSUM_[A-Z0-9]+)\s*=\s*(\d+)", header)}
    assert types == {"HDEM_FLOWSUM_F32": 1, "HDEM_FLOWSUM_U32": 2, "HDEM_FLOWSUM_U8": 3}
    zonal = {k: int(v) for k, v in re.findall(r"\bHDEM_ZONAL_([A-Z0-9]+)\s*=\s*(\d+)", header)}
    assert all(zonal[k.rsplit("_", 1)[1]] == v for k, v in types.items())
    assert {np.dtype(np.float32): 1, np.dtype(np.uint32): 2,
            np.dtype(np.uint8): 3} == flowsum.WEIGHT_TYPES
    # the struct, its sizeof note, and no kernel id of its own
    assert re.search(r"\}\s*hdem_flowsum_stats;\s*/\* sizeof == 48 \*/", header)
    enums = dict(re.findall(r"\b(HDEM_K_[A-Z0-9_]+)\s*=\s*(\d+)", header))
    assert int(enums["HDEM_K_COUNT"]) == 21 and "HDEM_K_FLOWSUM" not in header
    stats = backend._FlowSumStats                    # pylint: disable=protected-access
    assert ctypes.sizeof(stats) == 48 and stats().struct_size == 48
    assert stats.exits.offset == 8 and stats.nan_weights.offset == 16
    assert stats.ms_tile.offset == 32
    assert set(stats().as_dict()) == {"max_hops", "exits", "nan_weights", "tile_h", "tile_w",
                                      "ms_tile", "ms_forest", "ms_final"}
    # the unweighted ABI is what it was
    assert ctypes.sizeof(backend.FlowAccStats) == 32
    assert len(backend.SIGNATURES["hdem_flowacc_u8"]) == 6


def test_the_library_exports_the_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    assert hasattr(lib, "hdem_flowsum_u8") and hasattr(lib, "hdem_flowsum_u8_dev")
    assert hasattr(lib, "hdem_flowacc_u8") and hasattr(lib, "hdem_flowacc_u8_dev")
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile")).read()
    assert "hdem_flowsum.hip" in makefile
    # the argument checks that come before the context is used: a null context first
    lib = backend.load_library()
    for name in ("hdem_flowsum_u8", "hdem_flowsum_u8_dev"):
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
