"""
Terrain attributes of a DEM -- Horn gradient, slope, aspect, D8 slope, wetness and stream power
index (``hdem_terrain_f32`` / ``hdem_terrain_f32_dev``), and the same from a float32 catchment
area (``hdem_terrain_area_f32`` / ``hdem_terrain_area_f32_dev``): the binding, written once for
host arrays and device rasters with the two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals

import contextlib
import ctypes

import numpy as np

from . import backend

# outputs, all float32, in the order of the C ABI's pointers
TERRAIN_OUTPUTS = ("dzdx", "dzdy", "tangent", "degrees", "aspect", "d8_slope", "twi", "spi")
TWI_D8 = 1                  # HDEM_TERRAIN_TWI_D8
SLOPES = ("horn", "d8")     # what twi and spi take as their slope
TWI_GIVEN = 2               # HDEM_TERRAIN_TWI_GIVEN
AREA_SLOPES = ("horn", "given")     # the same for the area form; "d8" goes as well


def _positive(name, value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a number, got {value!r}") from None
    if not np.isfinite(value) or value <= 0:
        raise ValueError(f"{name} must be finite and positive, got {value}")
    return value


def cellsizes(cellsize):
    """``cellsize`` as ``(dy, dx)``: one number for square cells, or a ``(dy, dx)`` pair."""
    if isinstance(cellsize, (tuple, list)):
        if len(cellsize) != 2:
            raise ValueError(f"cellsize is a number or a (dy, dx) pair, got {cellsize!r}")
        return backend._cellsize(cellsize[0]), backend._cellsize(cellsize[1])
    size = backend._cellsize(cellsize)
    return size, size


def terrain_args(dem, want=("degrees",), cellsize=1.0, z_factor=1.0, codes=None,
                 accumulation=None, min_slope=1e-3, slope="horn"):
    """The checks that need no device: ``dem``, ``codes`` and ``accumulation`` are anything
    with ``dtype`` and ``shape`` (NumPy arrays or device rasters).  Returns ``want`` as a tuple
    in the ABI's order, ``(dy, dx)``, ``z_factor``, ``min_slope`` and the flags of the C call."""
    if dem is None:
        raise ValueError("terrain attributes need the dem they are derived from")
    shape = backend._check(dem, np.float32, "terrain attributes take", "a float32 DEM",
                           flat="terrain attributes take")
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in TERRAIN_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown terrain outputs {unknown}: choose among "
                         f"{list(TERRAIN_OUTPUTS)}")
    want = tuple(n for n in TERRAIN_OUTPUTS if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {list(TERRAIN_OUTPUTS)}")
    dy, dx = cellsizes(cellsize)
    z_factor = _positive("z_factor", z_factor)
    min_slope = _positive("min_slope", min_slope)
    if slope not in SLOPES:
        raise ValueError(f"slope is 'horn' or 'd8', got {slope!r}")
    if codes is not None:
        backend._check(codes, np.uint8, "the codes are", "uint8 D8 codes",
                       like=("the dem", shape))
    if accumulation is not None:
        backend._check(accumulation, np.uint32, "the accumulation is", like=("the dem", shape))
    for name in want:
        if name in ("twi", "spi") and accumulation is None:
            raise ValueError(f"{name} needs the uint32 accumulation raster")
    if "d8_slope" in want and codes is None:
        raise ValueError("d8_slope needs the uint8 D8 codes")
    if slope == "d8" and codes is None:
        raise ValueError("slope='d8' needs the uint8 D8 codes")
    return want, (dy, dx), z_factor, min_slope, TWI_D8 if slope == "d8" else 0


def _terrain(side, dem, want, cellsize, z_factor, codes, accumulation, min_slope, slope, out):
    dem = side.take("dem", dem, required=True)
    codes, accumulation = side.take("codes", codes), side.take("accumulation", accumulation)
    want, (dy, dx), z_factor, min_slope, flags = terrain_args(
        dem, want, cellsize, z_factor, codes, accumulation, min_slope, slope)
    out = dict(out or {})
    for name, raster in out.items():
        if name not in want:
            raise ValueError(f"out holds {name}, which is not wanted: {list(want)}")
        backend._check(raster, np.float32, f"out[{name!r}] is", like=("the dem", dem.shape))
    c = side.context(dem)
    st = backend._TerrainStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), dem.shape, np.float32, c)
                for name in TERRAIN_OUTPUTS if name in want}
        side.call(c, "hdem_terrain_f32", side.address(dem), *dem.shape,
                  side.address(accumulation), side.address(codes), dx, dy, z_factor, min_slope,
                  *[side.address(outs.get(name)) for name in TERRAIN_OUTPUTS], flags,
                  ctypes.byref(st))
    return outs, st.as_dict()


def terrain_dev(dem, want=("degrees",), cellsize=1.0, z_factor=1.0, codes=None,
                accumulation=None, min_slope=1e-3, slope="horn", out=None):
    """Terrain attributes of a float32 device raster (``hdem_terrain_f32_dev``), one launch for
    any subset ``want`` of :data:`TERRAIN_OUTPUTS`: ``dzdx`` / ``dzdy`` (Horn's gradient with
    ``z_factor / (8 dx)`` and ``z_factor / (8 dy)``; a neighbour outside the raster or NaN takes
    the centre's value), ``tangent`` (its length: percent slope / 100), ``degrees``, ``aspect``
    (compass direction of the steepest descent, -1 where the gradient is 0), ``d8_slope`` (drop
    to the D8 receiver over the step's length; needs ``codes``), ``twi`` =
    ``ln(a / max(t, min_slope))`` and ``spi`` = ``a * t`` with ``a = accumulation * sqrt(dx dy)``
    (both need ``accumulation``) and ``t`` the tangent, or the D8 slope with ``slope="d8"``.
    ``cellsize``: a number or ``(dy, dx)``.  ``out``: ``{name: float32 device raster}`` to write
    wanted outputs into (they stay the caller's).  Returns ``{name: DeviceRaster}`` and the
    stats dict (``nan_cells``, ``flat_cells``, ``floored_cells``, ``invalid_codes``,
    ``ms_total``).  Synchronises (the call reads its counters)."""
    return _terrain(backend._DEVICE, dem, want, cellsize, z_factor, codes, accumulation,
                    min_slope, slope, out)


def terrain(dem, want=("degrees",), cellsize=1.0, z_factor=1.0, codes=None, accumulation=None,
            min_slope=1e-3, slope="horn"):
    """Terrain attributes of host arrays (``hdem_terrain_f32``; see :func:`terrain_dev`):
    ``{name: ndarray}`` and the stats dict."""
    return _terrain(backend._HOST, dem, want, cellsize, z_factor, codes, accumulation,
                    min_slope, slope, None)


def terrain_area_args(dem, want=("twi",), cellsize=1.0, z_factor=1.0, area=None,
                      given_slope=None, codes=None, min_slope=1e-3, slope="horn"):
    """The checks of the area form that need no device: ``dem``, ``area``, ``given_slope`` and
    ``codes`` are anything with ``dtype`` and ``shape``.  Returns ``want`` as a tuple in the
    ABI's order, ``(dy, dx)``, ``z_factor``, ``min_slope`` and the flags of the C call."""
    if dem is None:
        raise ValueError("terrain attributes need the dem they are derived from")
    shape = backend._check(dem, np.float32, "terrain attributes take", "a float32 DEM",
                           flat="terrain attributes take")
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in TERRAIN_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown terrain outputs {unknown}: choose among "
                         f"{list(TERRAIN_OUTPUTS)}")
    want = tuple(n for n in TERRAIN_OUTPUTS if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {list(TERRAIN_OUTPUTS)}")
    dy, dx = cellsizes(cellsize)
    z_factor = _positive("z_factor", z_factor)
    min_slope = _positive("min_slope", min_slope)
    if slope not in AREA_SLOPES + ("d8",):
        raise ValueError(f"slope is 'horn', 'given' or 'd8', got {slope!r}")
    if codes is not None:
        backend._check(codes, np.uint8, "the codes are", "uint8 D8 codes",
                       like=("the dem", shape))
    if area is not None:
        backend._check(area, np.float32, "the area is", like=("the dem", shape))
    if given_slope is not None:
        backend._check(given_slope, np.float32, "the given slope is", like=("the dem", shape))
    for name in want:
        if name in ("twi", "spi") and area is None:
            raise ValueError(f"{name} needs the float32 area raster")
    if "d8_slope" in want and codes is None:
        raise ValueError("d8_slope needs the uint8 D8 codes")
    if slope == "d8" and codes is None:
        raise ValueError("slope='d8' needs the uint8 D8 codes")
    if slope == "given" and given_slope is None:
        raise ValueError("slope='given' needs the float32 given slope raster")
    if slope != "given" and given_slope is not None:
        raise ValueError(f"a given slope raster goes with slope='given', got {slope!r}")
    flags = {"horn": 0, "d8": TWI_D8, "given": TWI_GIVEN}[slope]
    return want, (dy, dx), z_factor, min_slope, flags


def _terrain_area(side, dem, want, cellsize, z_factor, area, given_slope, codes, min_slope,
                  slope, out):
    dem = side.take("dem", dem, required=True)
    area, given_slope = side.take("area", area), side.take("given_slope", given_slope)
    codes = side.take("codes", codes)
    want, (dy, dx), z_factor, min_slope, flags = terrain_area_args(
        dem, want, cellsize, z_factor, area, given_slope, codes, min_slope, slope)
    out = dict(out or {})
    for name, raster in out.items():
        if name not in want:
            raise ValueError(f"out holds {name}, which is not wanted: {list(want)}")
        backend._check(raster, np.float32, f"out[{name!r}] is", like=("the dem", dem.shape))
    c = side.context(dem)
    st = backend._TerrainAreaStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), dem.shape, np.float32, c)
                for name in TERRAIN_OUTPUTS if name in want}
        side.call(c, "hdem_terrain_area_f32", side.address(dem), *dem.shape,
                  side.address(area), side.address(given_slope), side.address(codes), dx, dy,
                  z_factor, min_slope,
                  *[side.address(outs.get(name)) for name in TERRAIN_OUTPUTS], flags,
                  ctypes.byref(st))
    return outs, st.as_dict()


def terrain_area_dev(dem, want=("twi",), cellsize=1.0, z_factor=1.0, area=None,
                     given_slope=None, codes=None, min_slope=1e-3, slope="horn", out=None):
    """:func:`terrain_dev` with a float32 catchment ``area`` in cells (the ``value`` of a
    D-infinity accumulation) in place of the uint32 accumulation
    (``hdem_terrain_area_f32_dev``): ``a = area * sqrt(dx dy)``.  ``slope``: ``"horn"``,
    ``"d8"`` (needs ``codes``) or ``"given"``: ``twi`` and ``spi`` take ``given_slope`` (float32,
    e.g. the D-infinity slope) as their ``t``, floored at ``min_slope``.  A NaN area gives NaN;
    zero and negative areas go through the arithmetic and are counted in
    ``stats["nonpositive_area"]``."""
    return _terrain_area(backend._DEVICE, dem, want, cellsize, z_factor, area, given_slope,
                         codes, min_slope, slope, out)


def terrain_area(dem, want=("twi",), cellsize=1.0, z_factor=1.0, area=None, given_slope=None,
                 codes=None, min_slope=1e-3, slope="horn"):
    """Terrain attributes from a float32 area, of host arrays (``hdem_terrain_area_f32``; see
    :func:`terrain_area_dev`): ``{name: ndarray}`` and the stats dict."""
    return _terrain_area(backend._HOST, dem, want, cellsize, z_factor, area, given_slope, codes,
                         min_slope, slope, None)
