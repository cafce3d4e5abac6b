"""
Weighted D8 flow accumulation (``hdem_flowsum_u8`` / ``hdem_flowsum_u8_dev``): the binding,
written once for host arrays and device rasters with the two sides of
:mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments

import contextlib
import ctypes
import math

import numpy as np

from . import backend

# outputs, in the order of the C ABI's pointers
FS_OUTPUTS = (("sum", np.int64), ("value", np.float32), ("mask", np.uint8))
# HDEM_FLOWSUM_*
WEIGHT_TYPES = {np.dtype(np.float32): 1, np.dtype(np.uint32): 2, np.dtype(np.uint8): 3}
Q_MAX = 2 ** 31 - 1         # the greatest quantised weight


def quantise(weights, frac_bits=16):
    """q(w) as the kernels compute it, int64: ``w`` itself for uint8 and uint32 weights,
    ``rint(float64(w) * 2^frac_bits)`` for float32 ones (the product is exact: one rounding, to
    nearest even), 0 for a NaN.  Range checks are the caller's."""
    weights = np.asarray(weights)
    if weights.dtype != np.float32:
        return weights.astype(np.int64)
    scaled = np.rint(weights.astype(np.float64) * 2.0 ** frac_bits)
    return np.where(np.isnan(scaled), 0.0, scaled).astype(np.int64)


def threshold_units(threshold, frac_bits):
    """``T = ceil(threshold * 2^frac_bits)``, the threshold of the mask in units of q: an int
    >= 1, or a ValueError."""
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold is a number, got {threshold!r}") from None
    if not math.isfinite(threshold):
        raise ValueError(f"threshold must be finite, got {threshold}")
    units = math.ceil(threshold * 2.0 ** frac_bits)
    if not 1 <= units < 2 ** 63:
        raise ValueError(f"threshold {threshold} is {units} in units of 2^-{frac_bits}: it must "
                         "come out in 1 ... 2^63 - 1")
    return units


def flowsum_args(codes, weights, frac_bits, want, threshold):
    """The checks that need no device: ``codes`` and ``weights`` are anything with ``dtype`` and
    ``shape`` (NumPy arrays or device rasters).  ``threshold`` is in weight units and goes with
    ``mask``.  Returns the weight type, ``frac_bits`` and the threshold for the C call and
    ``want`` as a tuple in the ABI's order."""
    shape = backend._check(codes, np.uint8, "weighted flow accumulation takes", "uint8 D8 codes",
                           flat="weighted flow accumulation takes")
    if weights is None:
        raise ValueError("weighted flow accumulation needs the weights it sums")
    if np.dtype(weights.dtype) not in WEIGHT_TYPES:
        raise ValueError("the weights are float32, uint32 or uint8, got "
                         f"{np.dtype(weights.dtype)}")
    backend._check(weights, None, "the weights are", like=("the codes", shape))
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= 30:
        raise ValueError(f"frac_bits is an integer in 0 ... 30, got {frac_bits!r}")
    frac_bits = int(frac_bits)
    if np.dtype(weights.dtype) != np.float32 and frac_bits != 0:
        raise ValueError(f"integer weights take frac_bits 0, got {frac_bits}")
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in FS_OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown weighted flow accumulation outputs {unknown}: choose among "
                         f"{names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    if "mask" in want:
        if threshold is None:
            raise ValueError("mask needs a threshold")
        units = threshold_units(threshold, frac_bits)
    elif threshold is not None:
        raise ValueError("a threshold goes with the mask output")
    else:
        units = 0
    return WEIGHT_TYPES[np.dtype(weights.dtype)], frac_bits, units, want


def _flowsum(side, codes, weights, frac_bits, want, threshold, out):
    codes = side.take("codes", codes, required=True)
    weights = side.take("weights", weights, required=True)
    weight_type, frac_bits, units, want = flowsum_args(codes, weights, frac_bits, want, threshold)
    out = dict(out or {})
    for name, dtype in FS_OUTPUTS:
        if name in out:
            if name not in want:
                raise ValueError(f"out has {name}, which is not wanted")
            backend._check(out[name], dtype, f"out[{name!r}] is", like=("the codes", codes.shape))
    c = side.context(codes)
    st = backend._FlowSumStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), codes.shape, dtype, c)
                for name, dtype in FS_OUTPUTS if name in want}
        side.call(c, "hdem_flowsum_u8", side.address(codes), *codes.shape,
                  side.address(weights), weight_type, frac_bits, units,
                  *[side.address(outs.get(name)) for name, _ in FS_OUTPUTS], ctypes.byref(st))
    return outs, st.as_dict()


def flowsum_dev(codes, weights, frac_bits=16, want=("value",), threshold=None, out=None):
    """Weighted D8 flow accumulation of a uint8 code raster (``hdem_flowsum_u8_dev``): for every
    cell the sum ``S`` of the quantised weights of the cells whose D8 path passes through it.
    ``weights``: a uint8, uint32 or float32 raster (float32: ``q = rint(w * 2^frac_bits)``).
    ``want``: any of ``sum`` (int64 ``S``), ``value`` (float32 ``S * 2^-frac_bits``) and
    ``mask`` (uint8, ``S >= ceil(threshold * 2^frac_bits)``).  ``out``: ``{name: DeviceRaster}``
    to write into.  Returns ``{name: DeviceRaster}`` and the stats dict.  Synchronises (the call
    reads its counters)."""
    return _flowsum(backend._DEVICE, codes, weights, frac_bits, want, threshold, out)


def flowsum(codes, weights, frac_bits=16, want=("value",), threshold=None):
    """Weighted D8 flow accumulation of host arrays (``hdem_flowsum_u8``; see
    :func:`flowsum_dev`): ``{name: ndarray}`` and the stats dict."""
    return _flowsum(backend._HOST, codes, weights, frac_bits, want, threshold, None)
