"""
Downstream D8 path sums and extremes (``FlowPathSum``, ``FlowPathExtreme``,
``hdem_flowpath_u8``): the CPU half.

Write the D8 path of ``c`` as ``p_0 = c -> ... -> p_k = s(c)``, its first stop as the flow trace
defines one (tests/test_flowtrace.py).  The sum is ``S(c) = sum(q[p_i], i < k)``, the quantised
cost of the step leaving each cell, 0 at a stop; the extreme is the least / greatest present
value over ``p_0 ... p_k``, both ends included, as a (key, holder) word of
tests/test_upextreme.py.  The host references live here and are used by
tests/test_gpu_flowpath.py:
  (a) ``sum_walk`` / ``extreme_walk``          all cells step down their paths together;
  (b) ``sum_doubling`` / ``extreme_doubling``  pointer doubling on the flat receiver array with
                                               the payload beside the pointer, ``ValueError`` on
                                               a cycle;
  (c) ``sum_holds`` / ``extreme_holds``        the local property, vectorised over every cell:
                                               a stop holds (own index + 1 or 0 when dry, 0) or
                                               its own word, any other cell its receiver's stop
                                               and ``q[c] + S[rec[c]]`` or
                                               ``best(word[c], E[rec[c]])``.  On acyclic codes
                                               that has one solution, so (c) is a proof.
``value_of`` is the NumPy formula of the float raster.  No GPU here: the references agree with
each other and with the flow trace's, ``quantise_steps`` gives the hand values, the operators
are importable from the package and the drop-in ``filters``, reject what they must without a
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

from hydrodem_amd import flowpath as fp
from test_flowacc import acc_kahn, random_acyclic_codes, receivers
from test_flowtrace import SHAPES, trace_doubling
from test_upextreme import IDENTITY, split_words, words_of
from test_watersheds import random_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, SE, S, SW, W_, NW, N, NE = 1, 2, 4, 8, 16, 32, 64, 128
Q_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def _setup(codes, streams):
    """codes, flat receivers, stop cells, stream cells (None without streams)."""
    codes = np.asarray(codes, dtype=np.uint8)
    rec = receivers(codes)
    stop = rec < 0
    stream = None
    if streams is not None:
        streams = np.asarray(streams)
        assert streams.shape == codes.shape
        stream = streams.ravel() != 0
        stop = stop | stream
    return codes, rec, stop, stream


def _stop_raster(shape, at, stream):
    stop = at + 1
    if stream is not None:
        stop[~stream[at]] = 0                            # ended in a dry terminal cell
    return stop.astype(np.uint32).reshape(shape)


def _rounds(n):
    return math.ceil(math.log2(n)) + 1 if n > 1 else 1


def _best(mode):
    return np.minimum if mode == "min" else np.maximum


def sum_walk(codes, q, streams=None):
    """(a): (stop, S), all cells stepping together until each stands on a stop."""
    codes, rec, stop, stream = _setup(codes, streams)
    q = np.asarray(q, dtype=np.int64).ravel()
    n = rec.size
    pos = np.arange(n, dtype=np.int64)
    total = np.zeros(n, np.int64)
    for _ in range(n + 1):
        moving = ~stop[pos]
        if not moving.any():
            return _stop_raster(codes.shape, pos, stream), total.reshape(codes.shape)
        total[moving] += q[pos[moving]]
        pos[moving] = rec[pos[moving]]
    raise ValueError(f"flow directions form a cycle: {int(moving.sum())} cells never resolve")


def sum_doubling(codes, q, streams=None):
    """(b): pointer doubling with the sum as payload, a stop pointing at itself with 0."""
    codes, rec, stop, stream = _setup(codes, streams)
    q = np.asarray(q, dtype=np.int64).ravel()
    n = rec.size
    ptr = np.where(stop, np.arange(n, dtype=np.int64), rec)
    total = np.where(stop, 0, q)
    for _ in range(_rounds(n)):
        total, ptr = total + total[ptr], ptr[ptr]
    lost = ~stop[ptr]
    if lost.any():
        raise ValueError(f"flow directions form a cycle: {int(lost.sum())} cells never resolve")
    return _stop_raster(codes.shape, ptr, stream), total.reshape(codes.shape)


def _local_stop(rec, is_stop, stream, stop):
    own = np.arange(rec.size, dtype=np.int64) + 1
    at_stop = own if stream is None else np.where(stream, own, 0)
    return np.where(is_stop, at_stop, stop.ravel().astype(np.int64)[np.maximum(rec, 0)])


def sum_holds(codes, q, stop, total, streams=None):
    """(c): ``S[c] = q[c] + S[rec[c]]`` with stops holding 0, and the stop handed down."""
    codes, rec, is_stop, stream = _setup(codes, streams)
    if stop.shape != codes.shape or total.shape != codes.shape:
        return False
    q = np.asarray(q, dtype=np.int64).ravel()
    flat = total.ravel().astype(np.int64)
    want = np.where(is_stop, 0, q + flat[np.maximum(rec, 0)])
    return bool(np.array_equal(want, flat)
                and np.array_equal(_local_stop(rec, is_stop, stream, stop), stop.ravel()))


def extreme_walk(codes, values, mode, streams=None):
    """(a): (stop, extreme, where), every cell reducing the words it steps on."""
    codes, rec, stop, stream = _setup(codes, streams)
    words = words_of(values, mode)
    n = rec.size
    pos = np.arange(n, dtype=np.int64)
    total = words.copy()
    for _ in range(n + 1):
        moving = ~stop[pos]
        if not moving.any():
            return (_stop_raster(codes.shape, pos, stream),
                    *split_words(total, mode, np.asarray(values).dtype, codes.shape))
        pos[moving] = rec[pos[moving]]
        total[moving] = _best(mode)(total[moving], words[pos[moving]])
    raise ValueError(f"flow directions form a cycle: {int(moving.sum())} cells never resolve")


def extreme_doubling(codes, values, mode, streams=None):
    """(b): pointer doubling, a word covering its cell to its pointee inclusively."""
    codes, rec, stop, stream = _setup(codes, streams)
    words = words_of(values, mode)
    n = rec.size
    ptr = np.where(stop, np.arange(n, dtype=np.int64), rec)
    total = _best(mode)(words, words[ptr])
    for _ in range(_rounds(n)):
        total, ptr = _best(mode)(total, total[ptr]), ptr[ptr]
    lost = ~stop[ptr]
    if lost.any():
        raise ValueError(f"flow directions form a cycle: {int(lost.sum())} cells never resolve")
    return (_stop_raster(codes.shape, ptr, stream),
            *split_words(total, mode, np.asarray(values).dtype, codes.shape))


def join_words(extreme, where, mode):
    """The flat uint64 words of an (extreme, where) pair: ``split_words`` backwards."""
    words = words_of(extreme, mode)                      # the key of the extreme, a wrong holder
    holder = where.ravel().astype(np.uint64)
    low = holder if mode == "min" else (~holder & np.uint64(0xFFFFFFFF))
    words = (words >> np.uint64(32)) << np.uint64(32) | low
    words[where.ravel() == 0xFFFFFFFF] = IDENTITY[mode]
    return words


def extreme_holds(codes, values, mode, stop, extreme, where, streams=None):
    """(c): ``E[c] = best(word[c], E[rec[c]])``, a stop holding its own word."""
    codes, rec, is_stop, stream = _setup(codes, streams)
    if not stop.shape == extreme.shape == where.shape == codes.shape:
        return False
    own = words_of(values, mode)
    got = join_words(extreme, where, mode)
    want = np.where(is_stop, own, _best(mode)(own, got[np.maximum(rec, 0)]))
    return bool(np.array_equal(want, got)
                and np.array_equal(_local_stop(rec, is_stop, stream, stop), stop.ravel()))


def value_of(stop, total, frac_bits):
    """The float32 value raster of the C ABI's definition; NaN where unreached."""
    v = (total.astype(np.float64) * 2.0 ** -frac_bits).astype(np.float32)
    v[stop == 0] = np.nan
    return v


def stream_sets(codes):
    """The three stream kinds as masks: none, a mask, an accumulation against a threshold."""
    shape = codes.shape
    return (None, random_seeds(shape, seed=sum(shape), every=10) != 0, acc_kahn(codes) >= 3)


def random_values(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint32:
        return rng.integers(0, 5, shape).astype(np.uint32)      # many ties
    v = rng.integers(-3, 4, shape).astype(np.float32)
    v[rng.random(shape) < 0.2] = np.nan
    v[rng.random(shape) < 0.1] = -0.0
    return v


# ---------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ramp", [False, True], ids=["noise", "ramp"])
def test_the_sum_references_agree(shape, ramp):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=ramp)
    q = np.random.default_rng(sum(shape)).integers(0, Q_MAX + 1, shape)
    for streams in stream_sets(codes):
        a, b = sum_walk(codes, q, streams), sum_doubling(codes, q, streams)
        assert a[0].dtype == b[0].dtype == np.uint32 and a[1].dtype == b[1].dtype == np.int64
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert sum_holds(codes, q, *b, streams=streams)
        assert np.array_equal(b[0], trace_doubling(codes, streams)[0])
        stops = (receivers(codes) < 0).reshape(shape)
        if streams is not None:
            stops |= streams
        assert not b[1][stops].any()
        if codes.size > 100:
            wrong = b[1].copy()
            wrong.flat[np.flatnonzero(~stops.ravel())[0]] += 1
            assert not sum_holds(codes, q, b[0], wrong, streams=streams)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint32], ids=["f32", "u32"])
def test_the_extreme_references_agree(shape, mode, dtype):
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=True)
    values = random_values(shape, dtype, seed=sum(shape))
    for streams in stream_sets(codes):
        a = extreme_walk(codes, values, mode, streams)
        b = extreme_doubling(codes, values, mode, streams)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert b[1].dtype == dtype and b[2].dtype == np.uint32
        assert extreme_holds(codes, values, mode, *b, streams=streams)
        assert np.array_equal(b[0], trace_doubling(codes, streams)[0])
        if codes.size > 100:
            wrong = b[2].copy()
            cell = np.flatnonzero(wrong.ravel() != 0xFFFFFFFF)[0]
            wrong.flat[cell] = (wrong.flat[cell] + 1) % codes.size
            assert not extreme_holds(codes, values, mode, b[0], b[1], wrong, streams=streams)


def test_the_references_on_a_row_with_written_out_answers():
    row = np.full((1, 6), E, np.uint8)
    q = np.array([[1, 2, 4, 8, 16, 32]])
    for fn in (sum_walk, sum_doubling):
        stop, total = fn(row, q)
        assert np.array_equal(stop, [[6] * 6])
        assert np.array_equal(total, [[31, 30, 28, 24, 16, 0]])      # the stop's own cost is out
        streams = np.array([[0, 0, 1, 0, 0, 0]], np.uint8)
        stop, total = fn(row, q, streams)
        assert np.array_equal(stop, [[3, 3, 3, 0, 0, 0]])
        assert np.array_equal(total, [[3, 2, 0, 24, 16, 0]])         # unreached: to the terminal
        assert np.array_equal(value_of(stop, total, 1),
                              np.array([[1.5, 1, 0, np.nan, np.nan, np.nan]], np.float32),
                              equal_nan=True)
    v = np.array([[3, np.nan, 1, -0.0, 0.0, 1]], np.float32)
    for fn in (extreme_walk, extreme_doubling):
        stop, extreme, where = fn(row, v, "min")
        assert np.array_equal(where, [[3, 3, 3, 3, 4, 5]])           # -0.0 below +0.0
        assert np.array_equal(extreme.view(np.uint32),
                              np.array([[-0.0, -0.0, -0.0, -0.0, 0.0, 1]], np.float32).view(np.uint32))
        stop, extreme, where = fn(row, v, "max")
        assert np.array_equal(where, [[0, 2, 2, 5, 5, 5]])           # ties: the smallest index
        assert np.array_equal(extreme, [[3, 1, 1, 1, 1, 1]])
        streams = np.array([[0, 1, 0, 0, 0, 0]], np.uint8)
        stop, extreme, where = fn(row, v, "max", streams)
        assert np.array_equal(stop, [[2, 2, 0, 0, 0, 0]])
        assert np.array_equal(where, [[0, 0xFFFFFFFF, 2, 5, 5, 5]])  # the stop is a NaN
        assert np.isnan(extreme[0, 1]) and extreme[0, 0] == 3
    pair = np.array([[E, W_, W_]], np.uint8)
    for fn in (sum_walk, sum_doubling):
        with pytest.raises(ValueError, match="cycle"):
            fn(pair, np.ones((1, 3)))
    for fn in (extreme_walk, extreme_doubling):
        with pytest.raises(ValueError, match="cycle"):
            fn(pair, np.ones((1, 3), np.float32), "min")


@pytest.mark.parametrize("shape", SHAPES + [(130, 70)])
@pytest.mark.parametrize("frac_bits", [0, 16])
def test_the_uniform_table_without_weights_gives_the_flow_distance_in_integers(shape, frac_bits):
    cs = 30.0
    codes = random_acyclic_codes(*shape, seed=shape[0] * 100 + shape[1], ramp=True)
    q = fp.quantise_steps(codes, None, "length", fp.step_lengths(shape[0], cs), frac_bits)
    card = int(np.rint(cs * 2.0 ** frac_bits))
    diag = int(np.rint((cs * np.sqrt(2.0)) * 2.0 ** frac_bits))
    for streams in stream_sets(codes):
        stop, total = sum_doubling(codes, q, streams)
        tstop, nc, nd = trace_doubling(codes, streams)
        assert np.array_equal(stop, tstop)
        assert np.array_equal(total, nc.astype(np.int64) * card + nd.astype(np.int64) * diag)


# ---------------------------------------------------------------------------
# the quantisation and the tables
# ---------------------------------------------------------------------------
def test_quantise_steps_against_hand_values():
    codes = np.array([[E, SE, S], [0, N, NE], [W_, SW, NW]], np.uint8)
    table = np.array([[2.0, 3.0, 5.0], [0.5, 0.25, 1.5], [10.0, 20.0, 30.0]])
    q = fp.quantise_steps(codes, None, "length", table, 2)
    assert q.dtype == np.int64
    assert np.array_equal(q, [[8, 20, 12], [0, 1, 6], [40, 120, 120]])       # code 0: no step
    w8 = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 255]], np.uint8)
    assert np.array_equal(fp.quantise_steps(codes, w8, "step", None, 0), w8)
    assert np.array_equal(fp.quantise_steps(codes, w8, "length", table, 1),
                          [[4, 20, 18], [0, 2, 18], [140, 480, 15300]])
    w32 = np.array([[0, 1, 2 ** 32 - 1]], np.uint32)
    assert np.array_equal(fp.quantise_steps(codes[:1], w32, "step"), [[0, 1, 2 ** 32 - 1]])
    wf = np.array([[0.5, 2.5, 3.5], [np.nan, -0.0, 1e-9], [1.25, 0.75, 32767.99999]], np.float32)
    assert np.array_equal(fp.quantise_steps(codes, wf, "step", None, 0),
                          [[0, 2, 4], [0, 0, 0], [1, 1, 32768]])             # ties to even
    assert np.array_equal(fp.quantise_steps(codes, wf, "step", None, 16)[0],
                          [32768, 163840, 229376])
    assert fp.quantise_steps(codes, wf, "step", None, 30)[2, 0] == 5 * 2 ** 28
    # per length: one rounding in the product, then the exact scaling, then rint
    third = np.array([[1.0 / 3.0]], np.float32)
    length = np.array([[0.1, 1.0, 1.0]])
    product = np.float64(third[0, 0]) * 0.1
    assert fp.quantise_steps(np.array([[E]], np.uint8), third, "length", length, 30)[0, 0] == \
        int(np.rint(product * 2.0 ** 30))
    assert fp.quantise_steps(np.array([[E]], np.uint8), np.array([[np.nan]], np.float32),
                             "length", length, 4)[0, 0] == 0
    with pytest.raises(ValueError, match="needs the weights"):
        fp.quantise_steps(codes, None, "step")
    with pytest.raises(ValueError, match="per is one of"):
        fp.quantise_steps(codes, w8, "cell")
    with pytest.raises(ValueError, match="frac_bits"):
        fp.quantise_steps(codes, wf, "step", None, 31)
    with pytest.raises(ValueError, match="3 rows"):
        fp.quantise_steps(codes, None, "length", table[:2], 0)


def test_the_step_length_tables():
    t = fp.step_lengths(3, 30.0)
    assert t.dtype == np.float64 and t.shape == (3, 3)
    assert np.array_equal(t, [[30.0, 30.0, 30.0 * np.sqrt(2.0)]] * 3)
    g = fp.geographic_step_lengths(4, 60.0, 0.5, 0.25)
    assert g.dtype == np.float64 and g.shape == (4, 3)
    radius = 6371008.8
    lat = np.radians(np.array([59.75, 59.25, 58.75, 58.25]))
    assert np.array_equal(g[:, 0], radius * np.cos(lat) * np.radians(0.25))
    assert np.array_equal(g[:, 1], np.full(4, radius * np.radians(0.5)))
    assert np.array_equal(g[:, 2], np.hypot(g[:, 0], g[:, 1]))
    assert (np.diff(g[:, 0]) > 0).all()                  # wider towards the equator
    assert abs(g[0, 1] - 55597.5) < 1.0                  # half a degree of latitude, metres
    one = fp.geographic_step_lengths(1, 0.5, 1.0, 1.0, radius=1.0)
    assert one[0, 0] == np.cos(0.0) * np.radians(1.0) == one[0, 1]
    for bad in (dict(height=0), dict(height=2.0), dict(dlat=0.0), dict(dlon=-1.0),
                dict(radius=0.0), dict(lat_top=float("nan")), dict(lat_top=90.0, dlat=0.0),
                dict(lat_top=95.0), dict(height=400, lat_top=80.0, dlat=0.5)):
        args = dict(height=4, lat_top=60.0, dlat=0.5, dlon=0.25)
        args.update(bad)
        with pytest.raises(ValueError):
            fp.geographic_step_lengths(**args)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rows"):
            fp.step_lengths(bad)
    with pytest.raises(ValueError, match="cellsize"):
        fp.step_lengths(3, 0.0)


# ---------------------------------------------------------------------------
# the operators without a device
# ---------------------------------------------------------------------------
def test_the_operators_are_exported_by_the_package():
    import hydrodem_amd as hd
    from hydrodem_amd.filters import custom_filters
    for name in ("FlowPathSum", "FlowPathExtreme"):
        cls = getattr(hd, name)
        assert cls is getattr(custom_filters, name)
        assert issubclass(cls, hd.Filter) and cls.auto_device is True
    w = np.ones((2, 2), np.float32)
    f = hd.FlowPathSum(w)
    assert f.weights is w and f.per == "step" and f.frac_bits == 16 and f.output == "value"
    assert f.streams is None and f.threshold is None and f.stats == {} and f.stop is None
    assert f.dtype == np.float32 and f.cellsize == 1.0 and f.step_lengths is None
    assert hd.FlowPathSum(w, output="sum").dtype == np.int64
    g = hd.FlowPathSum(per="length", cellsize=30.0, streams=np.ones((2, 2), bool))
    assert g.weights is None and g.streams.dtype == np.uint8       # a bool mask goes as bytes
    table = fp.step_lengths(2, 5.0)
    assert np.array_equal(hd.FlowPathSum(per="length", step_lengths=table).step_lengths, table)
    e = hd.FlowPathExtreme(w)
    assert e.values is w and e.mode == "min" and e.output == "extreme" and e.dtype == np.float32
    assert hd.FlowPathExtreme(w.astype(np.uint32), "max").dtype == np.uint32
    assert hd.FlowPathExtreme(w, output="where").dtype == np.uint32
    assert fp.MODES == {"sum": 0, "min": 1, "max": 2} and fp.PERS == {"step": 0, "length": 1}
    assert fp.Q_MAX == Q_MAX


def test_the_operators_resolve_through_the_dropin():
    dropin = os.path.join(ROOT, "hydrodem_amd", "dropin")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        sys.path.insert(0, {dropin!r})
        from filters.custom_filters import FlowPathSum, FlowPathExtreme
        import hydrodem_amd
        assert FlowPathSum is hydrodem_amd.FlowPathSum
        assert FlowPathExtreme is hydrodem_amd.FlowPathExtreme
        print("ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_operators_reject_bad_input_without_a_device(monkeypatch):
    import hydrodem_amd as hd
    from hydrodem_amd import backend

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(backend, "context", no_device)
    codes = np.ones((4, 4), np.uint8)
    mask = np.zeros((4, 4), np.uint8)
    acc = np.ones((4, 4), np.uint32)
    wf = np.ones((4, 4), np.float32)
    w8 = np.ones((4, 4), np.uint8)
    # the codes
    for f in (hd.FlowPathSum(wf), hd.FlowPathSum(per="length"), hd.FlowPathExtreme(wf),
              hd.FlowPathExtreme(acc, "max", streams=mask)):
        with pytest.raises(hd.NumpyArrayExpectedError):
            f.apply([[1, 2], [4, 8]])
        with pytest.raises(ValueError, match="uint8"):
            f.apply(np.zeros((4, 4), np.float32))
        with pytest.raises(ValueError, match="2-D"):
            f.apply(np.zeros((2, 4, 4), np.uint8))
    # the weights and the values
    with pytest.raises(ValueError, match="needs the weights"):
        hd.FlowPathSum()
    with pytest.raises(ValueError, match="needs the weights"):
        hd.FlowPathSum(None, per="step")
    with pytest.raises(ValueError, match="NumPy array or a DeviceRaster"):
        hd.FlowPathSum([[1.0]])
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowPathSum(wf.astype(np.float64))
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowPathSum(wf.astype(np.int32))
    with pytest.raises(ValueError, match="2-D"):
        hd.FlowPathSum(np.ones(4, np.float32))
    with pytest.raises(ValueError, match=r"weights are \(3, 4\)"):
        hd.FlowPathSum(np.ones((3, 4), np.float32)).apply(codes)
    with pytest.raises(ValueError, match="needs the values"):
        hd.FlowPathExtreme(None)
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowPathExtreme(w8)
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowPathExtreme(wf.astype(np.float64))
    with pytest.raises(ValueError, match=r"values are \(4, 5\)"):
        hd.FlowPathExtreme(np.ones((4, 5), np.float32)).apply(codes)
    # per, frac_bits, the table, the cell size
    for bad in ("cell", None, 1):
        with pytest.raises(ValueError, match="per is one of"):
            hd.FlowPathSum(wf, per=bad)
    for bad in (-1, 31, 1.5, True, None):
        with pytest.raises(ValueError, match="frac_bits"):
            hd.FlowPathSum(wf, frac_bits=bad)
    with pytest.raises(ValueError, match="integer weights per step take frac_bits 0"):
        hd.FlowPathSum(w8)
    with pytest.raises(ValueError, match="integer weights per step take frac_bits 0"):
        hd.FlowPathSum(acc, frac_bits=4)
    hd.FlowPathSum(w8, frac_bits=0)
    hd.FlowPathSum(w8, per="length", frac_bits=8)        # per length they take any
    with pytest.raises(ValueError, match="go with per='length'"):
        hd.FlowPathSum(wf, step_lengths=fp.step_lengths(4))
    with pytest.raises(ValueError, match=r"\(rows, 3\)"):
        hd.FlowPathSum(per="length", step_lengths=np.ones((4, 2)))
    with pytest.raises(ValueError, match=r"\(rows, 3\)"):
        hd.FlowPathSum(per="length", step_lengths="wide")
    for bad in (0.0, -1.0, np.nan, np.inf):
        table = fp.step_lengths(4)
        table[2, 1] = bad
        with pytest.raises(ValueError, match="1 entries that are not finite and positive.*row 2"):
            hd.FlowPathSum(per="length", step_lengths=table)
    with pytest.raises(ValueError, match="the codes have 4 rows"):
        hd.FlowPathSum(per="length", step_lengths=fp.step_lengths(5)).apply(codes)
    for bad in (0, -30.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="cellsize"):
            hd.FlowPathSum(per="length", cellsize=bad)
    # the outputs and the mode
    for bad in ("stop", "extreme", "mask", None):
        with pytest.raises(ValueError, match="output is one of"):
            hd.FlowPathSum(wf, output=bad)
    for bad in ("stop", "sum", "value", None):
        with pytest.raises(ValueError, match="output is one of"):
            hd.FlowPathExtreme(wf, output=bad)
    for bad in ("sum", "mean", None, 0):
        with pytest.raises(ValueError, match="mode is one of"):
            hd.FlowPathExtreme(wf, bad)
    # the streams and the threshold, as the flow trace words them
    with pytest.raises(ValueError, match="NumPy array or a DeviceRaster"):
        hd.FlowPathSum(wf, streams=[[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="dtype"):
        hd.FlowPathSum(wf, streams=np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match=r"streams are \(3, 4\)"):
        hd.FlowPathSum(wf, streams=np.zeros((3, 4), np.uint8)).apply(codes)
    with pytest.raises(ValueError, match="needs a threshold"):
        hd.FlowPathSum(wf, streams=acc)
    with pytest.raises(ValueError, match="takes no threshold"):
        hd.FlowPathExtreme(wf, streams=mask, threshold=1)
    with pytest.raises(ValueError, match="threshold needs"):
        hd.FlowPathExtreme(wf, threshold=1)
    for bad in (0, -1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="threshold is an integer"):
            hd.FlowPathSum(wf, streams=acc, threshold=bad)
    with pytest.raises(TypeError):
        hd.FlowPathSum(wf, "length")                     # keyword-only
    # the binding's own checks come before the device too
    with pytest.raises(ValueError, match="uint8 D8 codes"):
        fp.flowpath(codes.astype(np.int32), wf)
    with pytest.raises(ValueError, match="NumPy array"):
        fp.flowpath([[1]], wf)
    with pytest.raises(ValueError, match="unknown flow path outputs"):
        fp.flowpath(codes, wf, want=("extreme",))
    with pytest.raises(ValueError, match="unknown flow path outputs"):
        fp.flowpath(codes, wf, "min", want=("sum",))
    with pytest.raises(ValueError, match="no output wanted"):
        fp.flowpath_args(codes, None, None, "sum", wf, "step", None, 16, ())
    with pytest.raises(ValueError, match="mode is one of"):
        fp.flowpath(codes, wf, "mean")
    with pytest.raises(ValueError, match="belong to mode 'sum'"):
        fp.flowpath(codes, wf, "min", per="length")
    with pytest.raises(ValueError, match="belong to mode 'sum'"):
        fp.flowpath(codes, wf, "max", step_len=fp.step_lengths(4))
    with pytest.raises(ValueError, match="needs step_lengths"):
        fp.flowpath(codes, wf, per="length")
    with pytest.raises(ValueError, match="float32 or uint32"):
        fp.flowpath(codes, w8, "min")
    # what the checks hand to the C call
    assert fp.flowpath_args(codes, acc, 7, "sum", None, "length", fp.step_lengths(4), 3,
                            ("value", "stop"))[:6] == (2, 7, 0, 0, 1, 3)
    got = fp.flowpath_args(codes, mask, None, "max", acc, "step", None, 0, "where")
    assert got == (1, 0, 2, 2, 0, 0, None, ("where",))


NAMES = ("hdem_flowpath_u8", "hdem_flowpath_u8_dev")


def test_the_header_declares_the_entry_points():
    from hydrodem_amd import backend
    header = open(os.path.join(ROOT, "include", "hydrodem_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(backend.SIGNATURES[name]) == 20
    assert backend.SIGNATURES[NAMES[0]] == backend.SIGNATURES[NAMES[1]]
    enums = dict(re.findall(r"\b(HDEM_[A-Z0-9_]+)\s*=\s*(\d+)", code))
    assert int(enums["HDEM_K_COUNT"]) == 21              # the call has no kernel id
    assert {m: int(enums["HDEM_FLOWPATH_" + m.upper()]) for m in fp.MODES} == fp.MODES
    assert {p: int(enums["HDEM_FLOWPATH_PER_" + p.upper()]) for p in fp.PERS} == fp.PERS
    types = {np.dtype(np.float32): "F32", np.dtype(np.uint32): "U32", np.dtype(np.uint8): "U8"}
    for dtype, number in fp.VALUE_TYPES.items():
        assert int(enums["HDEM_FLOWPATH_" + types[dtype]]) == number
        assert int(enums["HDEM_FLOWSUM_" + types[dtype]]) == number   # numbered as flowsum's
    assert int(enums["HDEM_FLOWPATH_NONE"]) == fp.VALUE_NONE == 0
    written = re.search(r"\}\s*hdem_flowpath_stats;\s*/\*\s*sizeof == (\d+)\s*\*/", header)
    assert written and ctypes.sizeof(backend._FlowPathStats) == int(written.group(1)) == 72
    assert backend._FlowPathStats.struct_size.offset == 0
    assert backend._FlowPathStats().struct_size == 72
    fields = re.search(r"typedef struct hdem_flowpath_stats \{(.*?)\}", code, flags=re.S).group(1)
    declared = re.findall(r"\b([a-z_0-9]+)\s*[;,]", fields)
    assert declared == [n for n, _ in backend._FlowPathStats._fields_]
    assert set(backend._FlowPathStats().as_dict()) == {
        "forest_rounds", "stops", "unreached", "exits", "nan_weights", "absent", "tile_h",
        "tile_w", "ms_tile", "ms_forest", "ms_final"}


def test_the_library_exports_the_entry_points(built):
    from hydrodem_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name)
    lib = backend.load_library()
    for name in NAMES:                                   # the shared prologue, without a device
        rc = getattr(lib, name)(*[t() for t in backend.SIGNATURES[name]])
        assert rc == backend.BAD_ARG and lib.hdem_last_error() == b"ctx is null"
    makefile = open(os.path.join(ROOT, "hydrodem_amd", "csrc", "Makefile")).read()
    assert "hdem_flowpath.hip" in makefile
