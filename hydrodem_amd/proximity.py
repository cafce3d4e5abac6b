"""
Euclidean proximity to a source set -- squared distance, nearest source, allocation, distance,
rise above the nearest source and stream burning (``hdem_proximity`` /
``hdem_proximity_dev``): the binding, written once for host arrays and device rasters with the
two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals

import contextlib
import ctypes

import numpy as np

from . import backend

# outputs and their types, in the order of the C ABI's pointers
PROXIMITY_OUTPUTS = (("d2", np.uint32), ("nearest", np.uint32), ("label", np.uint32),
                     ("distance", np.float32), ("rise", np.float32), ("burned", np.float32))
SOURCES_MASK_U8, SOURCES_ACC_U32 = backend.FT_STREAMS_MASK_U8, backend.FT_STREAMS_ACC_U32
SOURCES_LABELS_U32 = 3      # HDEM_PX_SOURCES_LABELS_U32
UNREACHED = 0xFFFFFFFF      # d2 and nearest of a cell out of reach
MAX_SIDE = 65535            # the row pass keeps a column in 16 bits beside its sentinel


def _number(name, value, positive):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a number, got {value!r}") from None
    if not np.isfinite(value) or value < 0 or (positive and value == 0):
        raise ValueError(f"{name} must be finite and {'positive' if positive else 'not negative'}"
                         f", got {value}")
    return value


def proximity_args(sources, threshold=None, want=("distance",), dem=None, cellsize=1.0,
                   max_distance=None, buffer=None, smooth=0.0, sharp=0.0):
    """The checks that need no device: ``sources`` and ``dem`` are anything with ``dtype`` and
    ``shape`` (NumPy arrays or device rasters).  A uint8 raster is a mask, a uint32 raster with
    a ``threshold`` an accumulation, a uint32 raster without one a label raster.  Returns the
    source kind, the threshold and ``max_distance`` for the C call, ``want`` as a tuple in the
    ABI's order, and ``(cellsize, buffer, smooth, sharp)`` as floats."""
    if sources is None:
        raise ValueError("proximity needs the source raster it measures from")
    shape = backend._check(sources, None, "proximity takes", flat="proximity takes")
    h, w = shape
    if h < 1 or w < 1:
        raise ValueError(f"proximity takes a raster with cells, got {shape}")
    if h * w > 0xFFFFFFFF:
        raise ValueError(f"proximity works in uint32: {h} x {w} is more than 2^32 - 1 cells")
    if (h - 1) ** 2 + (w - 1) ** 2 > 0xFFFFFFFE:
        raise ValueError(f"the squared diagonal of {h} x {w} is more than 2^32 - 2")
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"{h} x {w} has a side of more than {MAX_SIDE} cells")
    names = [n for n, _ in PROXIMITY_OUTPUTS]
    if isinstance(want, str):
        want = (want,)
    unknown = [n for n in want if n not in names]
    if unknown:
        raise ValueError(f"unknown proximity outputs {unknown}: choose among {names}")
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
    if dem is not None:
        backend._check(dem, np.float32, "the dem is", like=("the sources", shape))
    for name in ("rise", "burned"):
        if name in want and dem is None:
            raise ValueError(f"{name} needs the float32 dem")
    cellsize = backend._cellsize(cellsize)
    if max_distance is None:
        max_distance = 0
    if isinstance(max_distance, bool) or int(max_distance) != max_distance or \
            not 0 <= int(max_distance) <= 0xFFFFFFFF:
        raise ValueError("max_distance is a whole number of cells in 0 ... 2^32 - 1 (0: none), "
                         f"got {max_distance!r}")
    if "burned" in want:
        if buffer is None:
            raise ValueError("burned needs a buffer, in cells")
        buffer = _number("buffer", buffer, True)
        smooth, sharp = _number("smooth", smooth, False), _number("sharp", sharp, False)
    else:
        buffer, smooth, sharp = 1.0, 0.0, 0.0
    return kind, threshold, int(max_distance), want, (cellsize, buffer, smooth, sharp)


def _proximity(side, sources, threshold, want, dem, cellsize, max_distance, buffer, smooth, sharp,
               out):
    sources = side.take("sources", sources, required=True, mask=True)
    dem = side.take("dem", dem)
    kind, threshold, max_distance, want, (cellsize, buffer, smooth, sharp) = proximity_args(
        sources, threshold, want, dem, cellsize, max_distance, buffer, smooth, sharp)
    types = dict(PROXIMITY_OUTPUTS)
    out = dict(out or {})
    for name, raster in out.items():
        if name not in want:
            raise ValueError(f"out holds {name}, which is not wanted: {list(want)}")
        backend._check(raster, types[name], f"out[{name!r}] is",
                       like=("the sources", tuple(sources.shape)))
    c = side.context(sources)
    st = backend._ProximityStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), tuple(sources.shape), dtype, c)
                for name, dtype in PROXIMITY_OUTPUTS if name in want}
        side.call(c, "hdem_proximity", side.address(sources), kind, threshold, *sources.shape,
                  side.address(dem), cellsize, max_distance, buffer, smooth, sharp,
                  *[side.address(outs.get(name)) for name, _ in PROXIMITY_OUTPUTS],
                  ctypes.byref(st))
    return outs, st.as_dict()


def proximity_dev(sources, threshold=None, want=("distance",), dem=None, cellsize=1.0,
                  max_distance=None, buffer=None, smooth=0.0, sharp=0.0, out=None):
    """Euclidean proximity of every cell to the source set of a device raster
    (``hdem_proximity_dev``).  ``sources``: a uint8 mask (non-zero = source), a uint32 raster
    with ``threshold`` (source where ``>= threshold``: a flow accumulation goes in as it is) or
    a uint32 label raster without one (non-zero = source).  The nearest source ``n(c)`` of a
    cell minimises ``d2 = (r - r')^2 + (x - x')^2``; among sources at equal ``d2`` it is the one
    with the smallest flat index.  ``want``: any of ``d2`` (uint32, exact), ``nearest`` (uint32,
    the flat index of ``n(c)``), ``label`` (uint32, ``sources[n(c)]``, label sources only),
    ``distance`` (float32, ``sqrt(d2) * cellsize`` in float64, rounded once), ``rise`` (float32,
    ``dem[c] - dem[n(c)]``) and ``burned`` (float32: ``dem - smooth * (1 - d / buffer) - (sharp
    on a source)`` where ``d < buffer`` cells, the ``dem`` elsewhere; ``buffer`` in cells,
    ``smooth`` and ``sharp`` in the dem's units).  ``max_distance`` (cells): beyond it, and
    everywhere without a source, a cell is out of reach: ``d2 = nearest = 0xFFFFFFFF``,
    ``label = 0``, ``distance = rise = NaN``, ``burned = dem``.  ``out``: ``{name: device
    raster}`` to write wanted outputs into (they stay the caller's).  Returns ``{name:
    DeviceRaster}`` and the stats dict (``sources``, ``unreached``, ``ms_row``, ``ms_column``,
    ``ms_final``).  Synchronises once (the call reads its counters)."""
    return _proximity(backend._DEVICE, sources, threshold, want, dem, cellsize, max_distance,
                      buffer, smooth, sharp, out)


def proximity(sources, threshold=None, want=("distance",), dem=None, cellsize=1.0,
              max_distance=None, buffer=None, smooth=0.0, sharp=0.0):
    """Euclidean proximity of host arrays (``hdem_proximity``; see :func:`proximity_dev`):
    ``{name: ndarray}`` and the stats dict.  A bool ``sources`` array is a mask."""
    return _proximity(backend._HOST, sources, threshold, want, dem, cellsize, max_distance,
                      buffer, smooth, sharp, None)
