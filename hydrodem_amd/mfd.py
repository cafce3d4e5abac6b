"""
Multiple-flow-direction (MFD) flow direction and accumulation (``hdem_mfd_f32`` /
``hdem_mfdacc_u64``): the binding, written once for host arrays and device rasters with the two
sides of :mod:`hydrodem_amd.backend`, and the host helpers for the MFD word.

The two C entry points have no ``_dev`` twin: they take host pointers by default and device
pointers with ``HDEM_ON_DEVICE`` in their flags, which this module passes itself.

The word, one uint64 per cell: bit 59 "has outflow" (a word without it is 0), the main
receiver's direction ``m`` in bits 56-58, and seven 8-bit shares ``p_1 ... p_7`` in bits 0-55:
``p_j`` is the share, in units of 2^-8, of the neighbour in direction ``(m + j) & 7``; the main
receiver takes the rest.  Directions count counter-clockwise from east (``DIRECTIONS``); north is
row - 1.  ``include/hydrodem_hip.h`` (A24, A25) has the contract.
"""
# pylint: disable=protected-access,too-many-arguments

import contextlib
import ctypes
import math

import numpy as np

from . import backend
from .dinf import OUTPUTS, TOTAL_LIMIT, cellsizes, check_frac_bits  # noqa: F401
from .flowsum import WEIGHT_TYPES

ON_DEVICE = 0x40000000                                   # HDEM_ON_DEVICE
HAS_FLOW = 1 << 59
# direction -> (dy, dx): 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE
DIRECTIONS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))
# ESRI D8 code -> direction: bit b of a code is direction (8 - b) & 7
D8_DIRECTIONS = {1: 0, 128: 1, 64: 2, 32: 3, 16: 4, 8: 5, 4: 6, 2: 7}
EXTRAS = ("slope",)                                      # float32, optional, of the direction
EXPONENTS = (0.25, 16.0)                                 # the range of the exponent
# method -> (exponent, w_card, w_diag); None: the caller's exponent
PRESETS = {"freeman": (1.1, 1.0, 1.0),
           "quinn": (1.0, 0.5, 0.35355339059327373),
           "holmgren": (None, 1.0, 1.0)}


# ---------------------------------------------------------------------------
# the word on the host
# ---------------------------------------------------------------------------
def pack(flow, main, shares):
    """The uint64 words of ``flow`` (bool), ``main`` (0 ... 7) and ``shares`` (``(..., 7)``,
    0 ... 255 each, at most 255 in all; ``shares[..., j - 1]`` is ``p_j``).  Where ``flow`` is
    false the word is 0, and ``main`` and ``shares`` must be 0 there."""
    flow, main, shares = np.asarray(flow, bool), np.asarray(main), np.asarray(shares)
    if shares.shape[-1:] != (7,):
        raise ValueError(f"shares has seven fields in its last axis, got shape {shares.shape}")
    if np.any((main < 0) | (main > 7)):
        raise ValueError("a main direction is 0 ... 7")
    if np.any((shares < 0) | (shares > 255)) or np.any(shares.sum(axis=-1) > 255):
        raise ValueError("a share is 0 ... 255 and the seven of a cell sum to at most 255")
    if np.any(~flow & ((main != 0) | shares.any(axis=-1))):
        raise ValueError("a cell without outflow has main 0 and no shares")
    words = np.uint64(HAS_FLOW) | (main.astype(np.uint64) << np.uint64(56))
    for j in range(7):
        words = words | (shares[..., j].astype(np.uint64) << np.uint64(8 * j))
    return np.where(flow, words, np.uint64(0))


def unpack(words):
    """``(flow, main, shares)`` of uint64 words: bool, uint8 and a ``(..., 7)`` uint8 array."""
    words = np.asarray(words)
    if words.dtype != np.uint64:
        raise ValueError(f"MFD words are uint64, got {words.dtype}")
    shares = np.stack([((words >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.uint8)
                       for j in range(7)], axis=-1)
    return ((words >> np.uint64(59)) & np.uint64(1)).astype(bool), \
        ((words >> np.uint64(56)) & np.uint64(7)).astype(np.uint8), shares


def invalid(words):
    """Where uint64 words are not valid MFD words: not 0, and bit 59 clear, a bit of 60-63 set or
    shares that sum to more than 255."""
    words = np.asarray(words)
    _, _, shares = unpack(words)
    return (words != 0) & (((words >> np.uint64(59)) != 1) |
                           (shares.astype(np.int64).sum(axis=-1) > 255))


def words_from_d8(codes):
    """The canonical words of uint8 ESRI D8 codes: one receiver each, 0 for code 0."""
    codes = np.asarray(codes)
    if codes.dtype != np.uint8:
        raise ValueError(f"D8 codes are uint8, got {codes.dtype}")
    bad_word = np.uint64(0xFFFFFFFFFFFFFFFF)
    table = np.full(256, bad_word, np.uint64)
    table[0] = 0
    for code, d in D8_DIRECTIONS.items():
        table[code] = HAS_FLOW | (d << 56)
    words = table[codes]
    bad = int((words == bad_word).sum())
    if bad:
        raise ValueError(f"invalid D8 code in {bad} cells: a code is 0 or one of 1, 2, 4, ..., 128")
    return words


def shares_of(words):
    """The shares of valid words by direction, ``(..., 8)`` int64 in units of 2^-8, with the main
    receiver's implicit share (256 minus the others) filled in; all 0 where the word is 0."""
    flow, main, shares = unpack(words)
    out = np.zeros(flow.shape + (8,), np.int64)
    main = main.astype(np.int64)
    for j in range(1, 8):
        np.put_along_axis(out, ((main + j) & 7)[..., None],
                          shares[..., j - 1].astype(np.int64)[..., None], axis=-1)
    rest = 256 - shares.astype(np.int64).sum(axis=-1)
    np.put_along_axis(out, main[..., None], rest[..., None], axis=-1)
    return np.where(flow[..., None], out, 0)


# ---------------------------------------------------------------------------
# argument checks (no device)
# ---------------------------------------------------------------------------
def _positive(name, value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a number, got {value!r}") from None
    if not math.isfinite(value) or value <= 0:
        raise ValueError(f"{name} must be finite and positive, got {value}")
    return value


def method_of(method="freeman", exponent=None):
    """``(exponent, w_card, w_diag)`` of a preset of ``PRESETS``, or of an
    ``(exponent, w_card, w_diag)`` triple.  ``holmgren`` needs the caller's ``exponent``; the
    other presets take none."""
    if isinstance(method, str):
        if method not in PRESETS:
            raise ValueError(f"method is one of {list(PRESETS)} or an (exponent, w_card, w_diag) "
                             f"triple, got {method!r}")
        preset, w_card, w_diag = PRESETS[method]
        if preset is None:
            if exponent is None:
                raise ValueError(f"method {method!r} needs an exponent")
        elif exponent is not None:
            raise ValueError(f"method {method!r} has the exponent {preset}: leave exponent out, "
                             "or choose 'holmgren'")
        else:
            exponent = preset
    else:
        if not isinstance(method, (tuple, list)) or len(method) != 3:
            raise ValueError(f"method is one of {list(PRESETS)} or an (exponent, w_card, w_diag) "
                             f"triple, got {method!r}")
        if exponent is not None:
            raise ValueError("the triple holds the exponent: leave exponent out")
        exponent, w_card, w_diag = method
    try:
        exponent = float(exponent)
    except (TypeError, ValueError):
        raise ValueError(f"the exponent is a number, got {exponent!r}") from None
    if not EXPONENTS[0] <= exponent <= EXPONENTS[1]:        # a NaN fails both
        raise ValueError(f"the exponent is {EXPONENTS[0]} ... {EXPONENTS[1]:g}, got {exponent}")
    return exponent, _positive("w_card", w_card), _positive("w_diag", w_diag)


def _wanted(want, names, what):
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown {what} outputs {unknown}: choose among {list(names)}")
    return tuple(n for n in names if n in want)


def mfd_args(dem, method="freeman", exponent=None, cellsize=1.0, fallback=None, want=()):
    """The checks of the direction that need no device: ``dem`` and ``fallback`` are anything
    with ``dtype`` and ``shape``.  Returns ``(exponent, w_card, w_diag)``, ``(dx, dy)`` and
    ``want`` in the ABI's order."""
    shape = backend._check(dem, np.float32, "MFD flow direction takes", "a float32 DEM",
                           flat="MFD flow direction takes")
    weights = method_of(method, exponent)
    dx, dy = cellsizes(cellsize)
    if fallback is not None:
        backend._check(fallback, np.uint8, "the fallback is", "uint8 D8 codes",
                       like=("the dem", shape))
    return weights, (dx, dy), _wanted(want, EXTRAS, "MFD")


def mfdacc_args(words, weights=None, frac_bits=16, want=("value",)):
    """The checks of the accumulation that need no device: ``words`` and ``weights`` are anything
    with ``dtype`` and ``shape``.  Returns the weight type (0 without weights) and ``frac_bits``
    for the C call and ``want`` as a tuple in the ABI's order."""
    if words is None:
        raise ValueError("MFD flow accumulation needs the words it routes along")
    shape = backend._check(words, np.uint64, "MFD flow accumulation takes", "uint64 MFD words",
                           flat="MFD flow accumulation takes")
    weight_type, most, whose = 0, 16, ""
    if weights is not None:
        if np.dtype(weights.dtype) not in WEIGHT_TYPES:
            raise ValueError("the weights are float32, uint32 or uint8, got "
                             f"{np.dtype(weights.dtype)}")
        backend._check(weights, None, "the weights are", like=("the words", shape))
        weight_type = WEIGHT_TYPES[np.dtype(weights.dtype)]
        most = 30 if np.dtype(weights.dtype) == np.float32 else 16
        whose = f" for {np.dtype(weights.dtype)} weights"
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= most:
        raise ValueError(f"frac_bits is an integer in 0 ... {most}{whose}, got {frac_bits!r}")
    want = _wanted(want, [n for n, _ in OUTPUTS], "MFD accumulation")
    if not want:
        raise ValueError(f"no output wanted: choose among {[n for n, _ in OUTPUTS]}")
    return weight_type, int(frac_bits), want


# ---------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------
def _call(side, c, name, *args):
    """``name(ctx, *args)``; the flags, second to last, say whose pointers the call is given."""
    args = list(args)
    args[-2] |= ON_DEVICE if side.device else 0
    c.check(getattr(c.lib, name)(c.handle, *args))


def _mfd(side, dem, method, exponent, cellsize, fallback, want, out):
    if dem is None:
        raise ValueError("MFD flow direction needs the dem it is derived from")
    dem = side.take("dem", dem, required=True)
    fallback = side.take("fallback", fallback)
    weights, (dx, dy), want = mfd_args(dem, method, exponent, cellsize, fallback, want)
    if out is not None:
        backend._check(out, np.uint64, "out is", like=("the dem", tuple(dem.shape)))
    c = side.context(dem)
    st = backend._MFDStats()
    with contextlib.ExitStack() as stack:
        words = side.result(stack, out, dem.shape, np.uint64, c)
        extras = {name: side.result(stack, None, dem.shape, np.float32, c) for name in want}
        _call(side, c, "hdem_mfd_f32", side.address(dem), *dem.shape, side.address(fallback),
              dx, dy, *weights, side.address(words),
              *[side.address(extras.get(name)) for name in EXTRAS], 0, ctypes.byref(st))
    return words, extras, st.as_dict()


def mfd_dev(dem, method="freeman", exponent=None, cellsize=1.0, fallback=None, want=(), out=None):
    """MFD flow direction of a float32 device raster (``hdem_mfd_f32`` with ``HDEM_ON_DEVICE``):
    the uint64 words, ``{name: DeviceRaster}`` for the float32 extras in ``want`` (``slope``) and
    the stats dict (``no_flow``, ``fallback_cells``, ``split_cells``, ``ms_total``).  ``method``:
    a preset of ``PRESETS`` (``holmgren`` with the caller's ``exponent``) or an
    ``(exponent, w_card, w_diag)`` triple.  ``cellsize``: a number or ``(dx, dy)``.
    ``fallback``: uint8 D8 codes for the cells without a lower neighbour.  ``out``: a uint64
    raster to write the words into.  Synchronises (the call reads its counters)."""
    return _mfd(backend._DEVICE, dem, method, exponent, cellsize, fallback, want, out)


def mfd(dem, method="freeman", exponent=None, cellsize=1.0, fallback=None, want=()):
    """MFD flow direction of host arrays (``hdem_mfd_f32``; see :func:`mfd_dev`)."""
    return _mfd(backend._HOST, dem, method, exponent, cellsize, fallback, want, None)


def _mfdacc(side, words, weights, frac_bits, want, out):
    words = side.take("words", words, required=True)
    weights = side.take("weights", weights)
    weight_type, frac_bits, want = mfdacc_args(words, weights, frac_bits, want)
    out = dict(out or {})
    for name, dtype in OUTPUTS:
        if name in out:
            if name not in want:
                raise ValueError(f"out has {name}, which is not wanted")
            backend._check(out[name], dtype, f"out[{name!r}] is",
                           like=("the words", tuple(words.shape)))
    c = side.context(words)
    st = backend._MFDAccStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), words.shape, dtype, c)
                for name, dtype in OUTPUTS if name in want}
        _call(side, c, "hdem_mfdacc_u64", side.address(words), *words.shape,
              side.address(weights), weight_type, frac_bits,
              *[side.address(outs.get(name)) for name, _ in OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def mfdacc_dev(words, weights=None, frac_bits=16, want=("value",), out=None):
    """MFD flow accumulation of a uint64 word raster (``hdem_mfdacc_u64`` with
    ``HDEM_ON_DEVICE``): ``A[c] = own(c)`` plus what its donors send it, in integers; ``own`` is
    ``2^frac_bits`` (``frac_bits`` 0 ... 16), or with ``weights`` (a uint8, uint32 or float32
    raster) the weight quantised as :func:`hydrodem_amd.dinf.quantise` does.  ``want``: ``sum``
    (int64 ``A``) and / or ``value`` (float32 ``A * 2^-frac_bits``).  ``out``:
    ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the stats
    dict.  Synchronises once per round."""
    return _mfdacc(backend._DEVICE, words, weights, frac_bits, want, out)


def mfdacc(words, weights=None, frac_bits=16, want=("value",)):
    """MFD flow accumulation of host arrays (``hdem_mfdacc_u64``; see :func:`mfdacc_dev`):
    ``{name: ndarray}`` and the stats dict."""
    return _mfdacc(backend._HOST, words, weights, frac_bits, want, None)
