"""
Cost distance, back link and allocation over a friction raster (``hdem_costdistance_f32``: one
symbol that takes device pointers by a flag): the binding, written once for host arrays and
device rasters with the two sides of :mod:`hydrodem_amd.backend`.  ``include/hydrodem_hip.h``
(A28) has the contract: costs quantised once to integers, step weights in units of
``2^-(frac_bits+1)`` cost x cell, the back link by the D8 window order.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals

import contextlib
import ctypes
import math

import numpy as np

from . import backend

# outputs and their types, in the order of the C ABI's pointers
OUTPUTS = (("units", np.int64), ("distance", np.float32), ("backlink", np.uint8),
           ("nearest", np.uint32), ("label", np.uint32))
SOURCES_MASK_U8, SOURCES_ACC_U32 = backend.FT_STREAMS_MASK_U8, backend.FT_STREAMS_ACC_U32
SOURCES_LABELS_U32 = 3      # HDEM_PX_SOURCES_LABELS_U32
ON_DEVICE = 0x40000000      # HDEM_ON_DEVICE
UNREACHED = 0xFFFFFFFF      # nearest of a cell out of reach
FRAC_BITS_MAX = 16
Q_MAX = 2 ** 28 - 1         # the largest quantised cost
SQRT2_Q31 = 3037000500      # round(sqrt(2) * 2^31): the diagonal step's factor


def units_per_cost(cellsize=1.0, frac_bits=16):
    """What one unit of ``units`` is worth in cost x length: ``cellsize * 2^-(frac_bits+1)``."""
    return math.ldexp(backend._cellsize(cellsize), -(int(frac_bits) + 1))


def max_units_of(max_distance, cellsize=1.0, frac_bits=16):
    """``max_units`` of the C call for a limit in the units of ``distance``:
    ``floor(max_distance / units_per_cost)`` in float64; 0 (no limit) for ``None``."""
    if max_distance is None:
        return 0
    try:
        limit = float(max_distance)
    except (TypeError, ValueError):
        raise ValueError(f"max_distance is a number, got {max_distance!r}") from None
    if isinstance(max_distance, bool) or not np.isfinite(limit) or limit <= 0:
        raise ValueError(f"max_distance must be finite and positive, got {max_distance!r}")
    units = math.floor(limit / units_per_cost(cellsize, frac_bits))
    if not 1 <= units < 2 ** 63:
        raise ValueError(f"max_distance {limit} is {units} units of "
                         f"{units_per_cost(cellsize, frac_bits)}: out of 1 ... 2^63 - 1")
    return units


def costdistance_args(cost, sources, threshold=None, want=("distance",), cellsize=1.0,
                      frac_bits=16, max_distance=None, max_units=None):
    """The checks that need no device: ``cost`` and ``sources`` are anything with ``dtype`` and
    ``shape`` (NumPy arrays or device rasters).  A uint8 ``sources`` raster is a mask, a uint32
    raster with a ``threshold`` an accumulation, a uint32 raster without one a label raster.
    Returns the source kind, the threshold and ``max_units`` for the C call, ``want`` as a tuple
    in the ABI's order, and ``cellsize`` as a float."""
    if cost is None:
        raise ValueError("cost distance needs the cost raster it crosses")
    if sources is None:
        raise ValueError("cost distance needs the source raster it measures from")
    shape = backend._check(cost, np.float32, "cost distance takes", "a float32 cost raster",
                           flat="cost distance takes")
    h, w = shape
    if h < 1 or w < 1:
        raise ValueError(f"cost distance takes a raster with cells, got {shape}")
    if h * w > 0xFFFFFFFF:
        raise ValueError(f"cost distance works in uint32: {h} x {w} is more than 2^32 - 1 cells")
    backend._check(sources, None, "the sources are", like=("the cost", shape))
    names = [n for n, _ in OUTPUTS]
    if isinstance(want, str):
        want = (want,)
    unknown = [n for n in want if n not in names]
    if unknown:
        raise ValueError(f"unknown cost distance outputs {unknown}: choose among {names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    if np.dtype(sources.dtype) == np.uint8:
        kind = SOURCES_MASK_U8
        if threshold is not None:
            raise ValueError("a uint8 source mask takes no threshold")
        threshold = 0
    elif np.dtype(sources.dtype) == np.uint32 and threshold is None:
        kind = SOURCES_LABELS_U32
        threshold = 0
    elif np.dtype(sources.dtype) == np.uint32:
        kind = SOURCES_ACC_U32
        if isinstance(threshold, bool) or int(threshold) != threshold or \
                not 1 <= int(threshold) <= 0xFFFFFFFF:
            raise ValueError(f"threshold is an integer in 1 ... 2^32 - 1, got {threshold!r}")
        threshold = int(threshold)
    else:
        raise ValueError("sources are a uint8 mask, a uint32 raster with a threshold or a "
                         f"uint32 label raster, got {sources.dtype}")
    if "label" in want and kind != SOURCES_LABELS_U32:
        raise ValueError("label needs a uint32 label raster as sources (and no threshold)")
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= FRAC_BITS_MAX:
        raise ValueError(f"frac_bits is an integer in 0 ... {FRAC_BITS_MAX}, got {frac_bits!r}")
    frac_bits = int(frac_bits)
    cellsize = backend._cellsize(cellsize)
    if max_units is not None:
        if max_distance is not None:
            raise ValueError("give max_distance or max_units, not both")
        if isinstance(max_units, bool) or not isinstance(max_units, (int, np.integer)) or \
                not 0 <= int(max_units) < 2 ** 63:
            raise ValueError("max_units is an integer in 0 ... 2^63 - 1 (0: no limit), "
                             f"got {max_units!r}")
        max_units = int(max_units)
    else:
        max_units = max_units_of(max_distance, cellsize, frac_bits)
    return kind, threshold, max_units, want, cellsize


def _costdistance(side, cost, sources, threshold, want, cellsize, frac_bits, max_distance,
                  max_units, out):
    cost = side.take("cost", cost, required=True)
    sources = side.take("sources", sources, required=True, mask=True)
    kind, threshold, max_units, want, cellsize = costdistance_args(
        cost, sources, threshold, want, cellsize, frac_bits, max_distance, max_units)
    shape = tuple(cost.shape)
    types = dict(OUTPUTS)
    out = dict(out or {})
    for name, raster in out.items():
        if name not in want:
            raise ValueError(f"out holds {name}, which is not wanted: {list(want)}")
        backend._check(raster, types[name], f"out[{name!r}] is", like=("the cost", shape))
    c = side.context(cost)
    st = backend._CostDistanceStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), shape, dtype, c)
                for name, dtype in OUTPUTS if name in want}
        c.check(c.lib.hdem_costdistance_f32(
            c.handle, side.address(cost), *shape, side.address(sources), kind, threshold,
            int(frac_bits), cellsize, max_units,
            *[side.address(outs.get(name)) for name, _ in OUTPUTS],
            ON_DEVICE if side.device else 0, ctypes.byref(st)))
    return outs, st.as_dict()


def costdistance_dev(cost, sources, threshold=None, want=("distance",), cellsize=1.0,
                     frac_bits=16, max_distance=None, out=None, *, max_units=None):
    """Cost distance of every cell to the source set, over a float32 cost raster on the device
    (``hdem_costdistance_f32`` with ``HDEM_ON_DEVICE``).  ``cost``: the price per cell length of
    crossing a cell; NaN is a barrier; quantised once as ``q = rint(cost * 2^frac_bits)``
    (``frac_bits`` 0 ... 16), which must come to 1 ... 2^28 - 1.  ``sources``: a uint8 mask
    (non-zero = source), a uint32 raster with ``threshold`` (source where ``>= threshold``) or a
    uint32 label raster without one.  A step between 8-neighbours ``a``, ``b`` weighs
    ``q(a) + q(b)``, times ``sqrt(2)`` (rounded once, in integers) when diagonal.  ``want``: any
    of ``units`` (int64, the least path weight ``D``), ``distance`` (float32,
    ``D * units_per_cost(cellsize, frac_bits)``), ``backlink`` (uint8 ESRI D8 code of the first
    neighbour in window order on a least path: the input of every D8 operator), ``nearest``
    (uint32, the flat index of the source the back links end in) and ``label`` (uint32,
    ``sources[nearest]``, label sources only).  Out of reach -- a barrier, no path, or beyond
    ``max_distance`` (in the units of ``distance``; ``max_units=`` gives the integer itself) --
    they hold -1, NaN, 0, 0xFFFFFFFF and 0.  ``out``: ``{name: device raster}`` to write wanted
    outputs into (they stay the caller's).  Returns ``{name: DeviceRaster}`` and the stats dict.
    Synchronises once per round."""
    return _costdistance(backend._DEVICE, cost, sources, threshold, want, cellsize, frac_bits,
                         max_distance, max_units, out)


def costdistance(cost, sources, threshold=None, want=("distance",), cellsize=1.0, frac_bits=16,
                 max_distance=None, *, max_units=None):
    """Cost distance of host arrays (``hdem_costdistance_f32``; see :func:`costdistance_dev`):
    ``{name: ndarray}`` and the stats dict.  A bool ``sources`` array is a mask."""
    return _costdistance(backend._HOST, cost, sources, threshold, want, cellsize, frac_bits,
                         max_distance, max_units, None)
