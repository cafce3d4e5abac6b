"""
D-infinity flow direction, accumulation and weighted accumulation (``hdem_dinf_f32`` /
``hdem_dinfacc_u32`` / ``hdem_dinfsum_u32`` and their ``_dev`` twins), distance down and distance
up (``hdem_dinfdist_u32``, ``hdem_dinfdistup_u32``: one symbol each that takes device pointers by
a flag): the binding, written once for host arrays and device rasters with the two sides of
:mod:`hydrodem_amd.backend`, and the host helpers for the D-infinity word.

The word, one uint32 per cell: ``q`` in bits 0-15 (0 ... 32768, the share of the diagonal
receiver in units of 2^-15), the facet in bits 16-19 (0: no outflow; 1 ... 8 as in Tarboton 1997,
``FACETS``).  ``include/hydrodem_hip.h`` (A20, A21, A22, A26, A27) has the contract.
"""
# pylint: disable=protected-access,too-many-arguments

import contextlib
import ctypes
import math

import numpy as np

from . import backend
from .flowsum import WEIGHT_TYPES, Q_MAX

Q_ONE = 32768               # q of "everything to the diagonal receiver"
# facet -> ((dy, dx) of the cardinal receiver e1, of the diagonal receiver e2, ac, af); north is
# row - 1
FACETS = {1: ((0, 1), (-1, 1), 0, 1), 2: ((-1, 0), (-1, 1), 1, -1),
          3: ((-1, 0), (-1, -1), 1, 1), 4: ((0, -1), (-1, -1), 2, -1),
          5: ((0, -1), (1, -1), 2, 1), 6: ((1, 0), (1, -1), 3, -1),
          7: ((1, 0), (1, 1), 3, 1), 8: ((0, 1), (1, 1), 4, -1)}
# ESRI D8 code -> (facet, q) of its canonical word, and its multiple of pi / 4
D8_WORDS = {1: (1, 0), 64: (2, 0), 16: (4, 0), 4: (6, 0),
            128: (1, Q_ONE), 32: (3, Q_ONE), 8: (5, Q_ONE), 2: (7, Q_ONE)}
D8_EIGHTHS = {1: 0, 128: 1, 64: 2, 32: 3, 16: 4, 8: 5, 4: 6, 2: 7}
OUTPUTS = (("sum", np.int64), ("value", np.float32))    # in the order of the C ABI's pointers
EXTRAS = ("angle", "slope")                             # float32, optional, of the direction
TOTAL_LIMIT = 2 ** 48       # the quantised weights of a raster sum to less than this
ON_DEVICE = 0x40000000      # HDEM_ON_DEVICE
DIST_KINDS = {"horizontal": 0, "vertical": 1, "surface": 2}         # HDEM_DD_*
DIST_STATISTICS = {"average": 0, "minimum": 1, "maximum": 2}


# ---------------------------------------------------------------------------
# the word on the host
# ---------------------------------------------------------------------------
def pack(facet, q):
    """The uint32 words of ``facet`` (0 ... 8) and ``q`` (0 ... 32768; 0 where the facet is 0)."""
    facet, q = np.asarray(facet), np.asarray(q)
    if np.any((facet < 0) | (facet > 8)):
        raise ValueError("a facet is 0 ... 8")
    if np.any((q < 0) | (q > Q_ONE)):
        raise ValueError(f"q is 0 ... {Q_ONE}")
    if np.any((facet == 0) & (q != 0)):
        raise ValueError("facet 0 goes with q 0")
    return (facet.astype(np.uint32) << np.uint32(16)) | q.astype(np.uint32)


def unpack(words):
    """``(facet, q)`` of uint32 words: a uint8 and a uint32 array."""
    words = np.asarray(words)
    if words.dtype != np.uint32:
        raise ValueError(f"D-infinity words are uint32, got {words.dtype}")
    return ((words >> np.uint32(16)) & np.uint32(15)).astype(np.uint8), words & np.uint32(0xFFFF)


def words_from_d8(codes):
    """The canonical words of uint8 ESRI D8 codes: one receiver each, 0 for code 0."""
    codes = np.asarray(codes)
    if codes.dtype != np.uint8:
        raise ValueError(f"D8 codes are uint8, got {codes.dtype}")
    table = np.full(256, 0xFFFFFFFF, np.uint32)
    table[0] = 0
    for code, (facet, q) in D8_WORDS.items():
        table[code] = (facet << 16) | q
    words = table[codes]
    bad = int((words == 0xFFFFFFFF).sum())
    if bad:
        raise ValueError(f"invalid D8 code in {bad} cells: a code is 0 or one of 1, 2, 4, ..., 128")
    return words


def angle_of(words, dx=1.0, dy=1.0):
    """The flow angle the words stand for, float64 radians counter-clockwise from east, -1 where
    the facet is 0: ``af * r + ac * pi / 2`` with ``r = q / 32768 * atan2(d2, d1)``.  (The angle
    output of the direction operator is the unquantised one.)"""
    facet, q = unpack(words)
    dx, dy = backend._cellsize(dx), backend._cellsize(dy)
    out = np.full(facet.shape, -1.0)
    for k, ((ey, _), _, ac, af) in FACETS.items():
        theta = math.atan2(dy, dx) if ey == 0 else math.atan2(dx, dy)
        a = af * (q / float(Q_ONE) * theta) + ac * (math.pi / 2)
        out = np.where(facet == k, np.where(a >= 2 * math.pi, 0.0, a), out)
    return out


# ---------------------------------------------------------------------------
# argument checks (no device)
# ---------------------------------------------------------------------------
def cellsizes(cellsize):
    """``cellsize`` as ``(dx, dy)``: one number for square cells, or a ``(dx, dy)`` pair."""
    if isinstance(cellsize, (tuple, list)):
        if len(cellsize) != 2:
            raise ValueError(f"cellsize is a number or a (dx, dy) pair, got {cellsize!r}")
        return backend._cellsize(cellsize[0]), backend._cellsize(cellsize[1])
    size = backend._cellsize(cellsize)
    return size, size


def dinf_args(dem, cellsize=1.0, fallback=None, want=()):
    """The checks of the direction that need no device: ``dem`` and ``fallback`` are anything
    with ``dtype`` and ``shape``.  Returns ``(dx, dy)`` and ``want`` in the ABI's order."""
    shape = backend._check(dem, np.float32, "D-infinity flow direction takes", "a float32 DEM",
                           flat="D-infinity flow direction takes")
    dx, dy = cellsizes(cellsize)
    if fallback is not None:
        backend._check(fallback, np.uint8, "the fallback is", "uint8 D8 codes",
                       like=("the dem", shape))
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in EXTRAS]
    if unknown:
        raise ValueError(f"unknown D-infinity outputs {unknown}: choose among {list(EXTRAS)}")
    return (dx, dy), tuple(n for n in EXTRAS if n in want)


def check_frac_bits(frac_bits):
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= 16:
        raise ValueError(f"frac_bits is an integer in 0 ... 16, got {frac_bits!r}")
    return int(frac_bits)


def dinfacc_args(words, frac_bits=16, want=("value",)):
    """The checks of the accumulation that need no device.  Returns ``frac_bits`` and ``want``
    as a tuple in the ABI's order."""
    if words is None:
        raise ValueError("D-infinity flow accumulation needs the words it routes along")
    backend._check(words, np.uint32, "D-infinity flow accumulation takes",
                   "uint32 D-infinity words", flat="D-infinity flow accumulation takes")
    frac_bits = check_frac_bits(frac_bits)
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown D-infinity accumulation outputs {unknown}: choose among "
                         f"{names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    return frac_bits, want


def quantise(weights, frac_bits=16):
    """q(w) as the weighted accumulation computes it, int64: ``w << frac_bits`` for uint8 and
    uint32 weights, ``rint(float64(w) * 2^frac_bits)`` for float32 ones (the product is exact:
    one rounding, to nearest even), 0 for a NaN.  Range checks are the caller's."""
    weights = np.asarray(weights)
    if weights.dtype != np.float32:
        return weights.astype(np.int64) << np.int64(frac_bits)
    scaled = np.rint(weights.astype(np.float64) * 2.0 ** frac_bits)
    return np.where(np.isnan(scaled), 0.0, scaled).astype(np.int64)


def dinfsum_args(words, weights, frac_bits=16, want=("value",)):
    """The checks of the weighted accumulation that need no device: ``words`` and ``weights`` are
    anything with ``dtype`` and ``shape``.  Returns the weight type and ``frac_bits`` for the C
    call and ``want`` as a tuple in the ABI's order."""
    if words is None:
        raise ValueError("weighted D-infinity flow accumulation needs the words it routes along")
    shape = backend._check(words, np.uint32, "weighted D-infinity flow accumulation takes",
                           "uint32 D-infinity words",
                           flat="weighted D-infinity flow accumulation takes")
    if weights is None:
        raise ValueError("weighted D-infinity flow accumulation needs the weights it sums")
    if np.dtype(weights.dtype) not in WEIGHT_TYPES:
        raise ValueError("the weights are float32, uint32 or uint8, got "
                         f"{np.dtype(weights.dtype)}")
    backend._check(weights, None, "the weights are", like=("the words", shape))
    most = 30 if np.dtype(weights.dtype) == np.float32 else 16
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= most:
        raise ValueError(f"frac_bits is an integer in 0 ... {most} for {np.dtype(weights.dtype)} "
                         f"weights, got {frac_bits!r}")
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown D-infinity accumulation outputs {unknown}: choose among "
                         f"{names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    return WEIGHT_TYPES[np.dtype(weights.dtype)], int(frac_bits), want


# ---------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------
def _dinf(side, dem, cellsize, fallback, want, out):
    if dem is None:
        raise ValueError("D-infinity flow direction needs the dem it is derived from")
    dem = side.take("dem", dem, required=True)
    fallback = side.take("fallback", fallback)
    (dx, dy), want = dinf_args(dem, cellsize, fallback, want)
    if out is not None:
        backend._check(out, np.uint32, "out is", like=("the dem", tuple(dem.shape)))
    c = side.context(dem)
    st = backend._DInfStats()
    with contextlib.ExitStack() as stack:
        words = side.result(stack, out, dem.shape, np.uint32, c)
        extras = {name: side.result(stack, None, dem.shape, np.float32, c) for name in want}
        side.call(c, "hdem_dinf_f32", side.address(dem), *dem.shape, side.address(fallback),
                  dx, dy, side.address(words),
                  *[side.address(extras.get(name)) for name in EXTRAS], 0, ctypes.byref(st))
    return words, extras, st.as_dict()


def dinf_dev(dem, cellsize=1.0, fallback=None, want=(), out=None):
    """D-infinity flow direction of a float32 device raster (``hdem_dinf_f32_dev``): the uint32
    words, ``{name: DeviceRaster}`` for the float32 extras in ``want`` (``angle``, ``slope``)
    and the stats dict (``no_flow``, ``fallback_cells``, ``ms_total``).  ``cellsize``: a number
    or ``(dx, dy)``.  ``fallback``: uint8 D8 codes for the cells no facet drains.  ``out``: a
    uint32 raster to write the words into.  Synchronises (the call reads its counters)."""
    return _dinf(backend._DEVICE, dem, cellsize, fallback, want, out)


def dinf(dem, cellsize=1.0, fallback=None, want=()):
    """D-infinity flow direction of host arrays (``hdem_dinf_f32``; see :func:`dinf_dev`)."""
    return _dinf(backend._HOST, dem, cellsize, fallback, want, None)


def _dinfacc(side, words, frac_bits, want, out):
    words = side.take("words", words, required=True)
    frac_bits, want = dinfacc_args(words, frac_bits, want)
    out = dict(out or {})
    for name, dtype in OUTPUTS:
        if name in out:
            if name not in want:
                raise ValueError(f"out has {name}, which is not wanted")
            backend._check(out[name], dtype, f"out[{name!r}] is",
                           like=("the words", tuple(words.shape)))
    c = side.context(words)
    st = backend._DInfAccStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), words.shape, dtype, c)
                for name, dtype in OUTPUTS if name in want}
        side.call(c, "hdem_dinfacc_u32", side.address(words), *words.shape, frac_bits,
                  *[side.address(outs.get(name)) for name, _ in OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def dinfacc_dev(words, frac_bits=16, want=("value",), out=None):
    """D-infinity flow accumulation of a uint32 word raster (``hdem_dinfacc_u32_dev``):
    ``A[c] = 2^frac_bits`` plus the shares its donors send it, in integers.  ``want``: ``sum``
    (int64 ``A``) and / or ``value`` (float32 ``A * 2^-frac_bits``, in cells).  ``out``:
    ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the stats
    dict.  Synchronises once per round."""
    return _dinfacc(backend._DEVICE, words, frac_bits, want, out)


def dinfacc(words, frac_bits=16, want=("value",)):
    """D-infinity flow accumulation of host arrays (``hdem_dinfacc_u32``; see
    :func:`dinfacc_dev`): ``{name: ndarray}`` and the stats dict."""
    return _dinfacc(backend._HOST, words, frac_bits, want, None)


def _dinfsum(side, words, weights, frac_bits, want, out):
    words = side.take("words", words, required=True)
    weights = side.take("weights", weights, required=True)
    weight_type, frac_bits, want = dinfsum_args(words, weights, frac_bits, want)
    out = dict(out or {})
    for name, dtype in OUTPUTS:
        if name in out:
            if name not in want:
                raise ValueError(f"out has {name}, which is not wanted")
            backend._check(out[name], dtype, f"out[{name!r}] is",
                           like=("the words", tuple(words.shape)))
    c = side.context(words)
    st = backend._DInfSumStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), words.shape, dtype, c)
                for name, dtype in OUTPUTS if name in want}
        side.call(c, "hdem_dinfsum_u32", side.address(words), *words.shape,
                  side.address(weights), weight_type, frac_bits,
                  *[side.address(outs.get(name)) for name, _ in OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def dinfsum_dev(words, weights, frac_bits=16, want=("value",), out=None):
    """Weighted D-infinity flow accumulation of a uint32 word raster (``hdem_dinfsum_u32_dev``):
    ``A[c] = q(w[c])`` plus the shares its donors send it, in integers.  ``weights``: a uint8,
    uint32 (``q = w << frac_bits``, ``frac_bits`` 0 ... 16) or float32 raster
    (``q = rint(w * 2^frac_bits)``, ``frac_bits`` 0 ... 30).  ``want``: ``sum`` (int64 ``A``)
    and / or ``value`` (float32 ``A * 2^-frac_bits``, in weight units).  ``out``:
    ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the stats dict
    (the accumulation's, ``nan_weights``, ``bad_weights``, ``total``).  Synchronises once per
    round."""
    return _dinfsum(backend._DEVICE, words, weights, frac_bits, want, out)


def dinfsum(words, weights, frac_bits=16, want=("value",)):
    """Weighted D-infinity flow accumulation of host arrays (``hdem_dinfsum_u32``; see
    :func:`dinfsum_dev`): ``{name: ndarray}`` and the stats dict."""
    return _dinfsum(backend._HOST, words, weights, frac_bits, want, None)


# ---------------------------------------------------------------------------
# distance down (A26): one C symbol, host or device pointers by a flag
# ---------------------------------------------------------------------------
def dinfdist_args(words, streams=None, threshold=None, dem=None, cellsize=1.0,
                  kind="horizontal", statistic="average"):
    """The checks of the distance down that need no device: ``words``, ``streams`` and ``dem``
    are anything with ``dtype`` and ``shape``.  Returns the kind, the statistic, the stream kind
    and the threshold for the C call, and ``(dx, dy)``."""
    if words is None:
        raise ValueError("D-infinity distance down needs the words it follows")
    shape = backend._check(words, np.uint32, "D-infinity distance down takes",
                           "uint32 D-infinity words", flat="D-infinity distance down takes")
    if shape[0] * shape[1] > 0xFFFFFFFF:
        raise ValueError(f"D-infinity distance down works in uint32: {shape[0]} x {shape[1]} "
                         "cells is more than 2^32 - 1")
    if not isinstance(kind, str) or kind not in DIST_KINDS:
        raise ValueError(f"kind is one of {list(DIST_KINDS)}, got {kind!r}")
    if not isinstance(statistic, str) or statistic not in DIST_STATISTICS:
        raise ValueError(f"statistic is one of {list(DIST_STATISTICS)}, got {statistic!r}")
    if streams is None:
        stream_kind = backend.FT_STREAMS_NONE
        if threshold is not None:
            raise ValueError("a threshold needs the uint32 raster it applies to")
        threshold = 0
    else:
        backend._check(streams, None, "streams are", like=("the words", shape))
        if np.dtype(streams.dtype) == np.uint8:
            stream_kind = backend.FT_STREAMS_MASK_U8
            if threshold is not None:
                raise ValueError("a uint8 stream mask takes no threshold")
            threshold = 0
        elif np.dtype(streams.dtype) == np.uint32:
            stream_kind = backend.FT_STREAMS_ACC_U32
            if threshold is None:
                raise ValueError("a uint32 stream raster needs a threshold")
            if isinstance(threshold, bool) or int(threshold) != threshold or \
                    not 1 <= int(threshold) <= 0xFFFFFFFF:
                raise ValueError(f"threshold is an integer in 1 ... 2^32 - 1, got {threshold!r}")
            threshold = int(threshold)
        else:
            raise ValueError("streams are a uint8 mask or a uint32 raster with a threshold, "
                             f"got {streams.dtype}")
    if kind == "horizontal":
        if dem is not None:
            raise ValueError("the horizontal distance takes no dem")
    elif dem is None:
        raise ValueError(f"the {kind} distance needs the dem it is measured on")
    else:
        backend._check(dem, np.float32, "the dem is", like=("the words", shape))
    return DIST_KINDS[kind], DIST_STATISTICS[statistic], stream_kind, threshold, \
        cellsizes(cellsize)


def _dinfdist(side, words, streams, threshold, dem, cellsize, kind, statistic, out):
    words = side.take("words", words, required=True)
    streams, dem = side.take("streams", streams, mask=True), side.take("dem", dem)
    kind, statistic, stream_kind, threshold, (dx, dy) = dinfdist_args(
        words, streams, threshold, dem, cellsize, kind, statistic)
    if out is not None:
        backend._check(out, np.float32, "out is", like=("the words", tuple(words.shape)))
    c = side.context(words)
    st = backend._DInfDistStats()
    with contextlib.ExitStack() as stack:
        distance = side.result(stack, out, words.shape, np.float32, c)
        c.check(c.lib.hdem_dinfdist_u32(
            c.handle, side.address(words), *words.shape, side.address(streams), stream_kind,
            threshold, side.address(dem), dx, dy, kind, statistic, side.address(distance),
            ON_DEVICE if side.device else 0, ctypes.byref(st)))
    return distance, st.as_dict()


def dinfdist_dev(words, streams=None, threshold=None, dem=None, cellsize=1.0, kind="horizontal",
                 statistic="average", out=None):
    """D-infinity distance down of a uint32 word raster (``hdem_dinfdist_u32`` with
    ``HDEM_ON_DEVICE``): for every cell the distance along its D-infinity paths to the stop set,
    float32, NaN where a path ends without a stop.  ``streams``: ``None`` (the stops are the cells
    with facet 0), a uint8 mask raster, or a uint32 raster with ``threshold`` (a stop where
    ``>= threshold``).  ``kind``: ``horizontal``, ``vertical`` or ``surface`` (the last two need
    the float32 ``dem``); ``statistic``: ``average`` (weighted by the flow proportions),
    ``minimum`` or ``maximum``.  ``cellsize``: a number or ``(dx, dy)``.  ``out``: a float32 raster
    to write into.  Returns the raster and the stats dict.  Synchronises once per round."""
    return _dinfdist(backend._DEVICE, words, streams, threshold, dem, cellsize, kind, statistic,
                     out)


def dinfdist(words, streams=None, threshold=None, dem=None, cellsize=1.0, kind="horizontal",
             statistic="average"):
    """D-infinity distance down of host arrays (``hdem_dinfdist_u32``; see :func:`dinfdist_dev`):
    the float32 array and the stats dict.  A bool ``streams`` array is a mask."""
    return _dinfdist(backend._HOST, words, streams, threshold, dem, cellsize, kind, statistic,
                     None)


# ---------------------------------------------------------------------------
# distance up (A27): one C symbol, host or device pointers by a flag
# ---------------------------------------------------------------------------
def min_share_of(min_proportion=None, min_share=None):
    """``min_share`` of the C call, 1 ... 32768 in units of 2^-15: the integer given as
    ``min_share``, or ``max(1, ceil(min_proportion * 32768))`` of a ``min_proportion`` in (0, 1]
    (0.5 when neither is given)."""
    if min_share is not None:
        if min_proportion is not None:
            raise ValueError("give min_proportion or min_share, not both")
        if isinstance(min_share, bool) or not isinstance(min_share, (int, np.integer)) or \
                not 1 <= int(min_share) <= Q_ONE:
            raise ValueError(f"min_share is an integer in 1 ... {Q_ONE}, got {min_share!r}")
        return int(min_share)
    if min_proportion is None:
        min_proportion = 0.5
    if isinstance(min_proportion, bool) or \
            not isinstance(min_proportion, (int, float, np.integer, np.floating)) or \
            not 0.0 < float(min_proportion) <= 1.0:
        raise ValueError(f"min_proportion is a number in (0, 1], got {min_proportion!r}")
    return max(1, math.ceil(float(min_proportion) * Q_ONE))


def dinfdistup_args(words, dem=None, cellsize=1.0, kind="horizontal", statistic="average",
                    min_proportion=None, min_share=None):
    """The checks of the distance up that need no device: ``words`` and ``dem`` are anything
    with ``dtype`` and ``shape``.  Returns the kind, the statistic and ``min_share`` for the C
    call, and ``(dx, dy)``."""
    if words is None:
        raise ValueError("D-infinity distance up needs the words it follows")
    shape = backend._check(words, np.uint32, "D-infinity distance up takes",
                           "uint32 D-infinity words", flat="D-infinity distance up takes")
    if shape[0] * shape[1] > 0xFFFFFFFF:
        raise ValueError(f"D-infinity distance up works in uint32: {shape[0]} x {shape[1]} "
                         "cells is more than 2^32 - 1")
    if not isinstance(kind, str) or kind not in DIST_KINDS:
        raise ValueError(f"kind is one of {list(DIST_KINDS)}, got {kind!r}")
    if not isinstance(statistic, str) or statistic not in DIST_STATISTICS:
        raise ValueError(f"statistic is one of {list(DIST_STATISTICS)}, got {statistic!r}")
    share = min_share_of(min_proportion, min_share)
    if kind == "horizontal":
        if dem is not None:
            raise ValueError("the horizontal distance takes no dem")
    elif dem is None:
        raise ValueError(f"the {kind} distance needs the dem it is measured on")
    else:
        backend._check(dem, np.float32, "the dem is", like=("the words", shape))
    return DIST_KINDS[kind], DIST_STATISTICS[statistic], share, cellsizes(cellsize)


def _dinfdistup(side, words, dem, cellsize, kind, statistic, min_proportion, min_share, out):
    words = side.take("words", words, required=True)
    dem = side.take("dem", dem)
    kind, statistic, share, (dx, dy) = dinfdistup_args(words, dem, cellsize, kind, statistic,
                                                       min_proportion, min_share)
    if out is not None:
        backend._check(out, np.float32, "out is", like=("the words", tuple(words.shape)))
    c = side.context(words)
    st = backend._DInfDistUpStats()
    with contextlib.ExitStack() as stack:
        distance = side.result(stack, out, words.shape, np.float32, c)
        c.check(c.lib.hdem_dinfdistup_u32(
            c.handle, side.address(words), *words.shape, side.address(dem), dx, dy, kind,
            statistic, share, side.address(distance), ON_DEVICE if side.device else 0,
            ctypes.byref(st)))
    return distance, st.as_dict()


def dinfdistup_dev(words, dem=None, cellsize=1.0, kind="horizontal", statistic="average",
                   min_proportion=None, out=None, *, min_share=None):
    """D-infinity distance up of a uint32 word raster (``hdem_dinfdistup_u32`` with
    ``HDEM_ON_DEVICE``): for every cell the distance up its D-infinity paths to the ridge,
    float32, over the neighbours that send it at least ``min_proportion`` of their flow; 0 in a
    cell that no neighbour does.  ``kind``: ``horizontal``, ``vertical`` or ``surface`` (the last
    two need the float32 ``dem``); ``statistic``: ``average`` (weighted by the entering shares),
    ``minimum`` or ``maximum``.  ``min_proportion``: a number in (0, 1], 0.5 by default, taken as
    ``min_share = max(1, ceil(min_proportion * 32768))``; ``min_share=`` gives the integer itself
    (1 ... 32768), and not both.  ``cellsize``: a number or ``(dx, dy)``.  ``out``: a float32
    raster to write into.  Returns the raster and the stats dict.  Synchronises once per round."""
    return _dinfdistup(backend._DEVICE, words, dem, cellsize, kind, statistic, min_proportion,
                       min_share, out)


def dinfdistup(words, dem=None, cellsize=1.0, kind="horizontal", statistic="average",
               min_proportion=None, *, min_share=None):
    """D-infinity distance up of host arrays (``hdem_dinfdistup_u32``; see
    :func:`dinfdistup_dev`): the float32 array and the stats dict."""
    return _dinfdistup(backend._HOST, words, dem, cellsize, kind, statistic, min_proportion,
                       min_share, None)
