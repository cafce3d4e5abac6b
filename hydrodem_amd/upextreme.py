"""
Upstream D8 extremes and depression breaching (``hdem_upextreme_u8`` / ``hdem_breach_f32`` and
their ``_dev`` twins): the binding, written once for host arrays and device rasters with the
two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments

import contextlib
import ctypes

import numpy as np

from . import backend

# HDEM_UPEXT_*
VALUE_TYPES = {np.dtype(np.float32): 1, np.dtype(np.uint32): 2}
MODES = {"min": 0, "max": 1}
# outputs of the extreme, in the order of the C ABI's pointers (extreme: of the values' dtype)
UE_OUTPUTS = ("extreme", "where")
# outputs of the breach, in the order of the C ABI's pointers
BR_OUTPUTS = (("carved", np.float32), ("source", np.uint32))
NOWHERE = 0xFFFFFFFF        # where / source: no holder, cell unchanged


def upextreme_args(codes, values, mode, want):
    """The checks that need no device: ``codes`` and ``values`` are anything with ``dtype`` and
    ``shape`` (NumPy arrays or device rasters).  Returns the value type and the mode for the C
    call and ``want`` as a tuple in the ABI's order."""
    shape = backend._check(codes, np.uint8, "the upstream extreme takes", "uint8 D8 codes",
                           flat="the upstream extreme takes")
    if values is None:
        raise ValueError("the upstream extreme needs the values it reduces")
    if np.dtype(values.dtype) not in VALUE_TYPES:
        raise ValueError(f"the values are float32 or uint32, got {np.dtype(values.dtype)}")
    backend._check(values, None, "the values are", like=("the codes", shape))
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode is one of {list(MODES)}, got {mode!r}")
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in UE_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown upstream extreme outputs {unknown}: choose among "
                         f"{list(UE_OUTPUTS)}")
    want = tuple(n for n in UE_OUTPUTS if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {list(UE_OUTPUTS)}")
    return VALUE_TYPES[np.dtype(values.dtype)], MODES[mode], want


def _checked_outs(out, dtypes, want, shape):
    out = dict(out or {})
    for name, given in out.items():
        if name not in want:
            raise ValueError(f"out has {name}, which is not wanted")
        backend._check(given, dtypes[name], f"out[{name!r}] is", like=("the codes", shape))
    return out


def _upextreme(side, codes, values, mode, want, out):
    codes = side.take("codes", codes, required=True)
    values = side.take("values", values, required=True)
    value_type, mode, want = upextreme_args(codes, values, mode, want)
    dtypes = {"extreme": np.dtype(values.dtype), "where": np.dtype(np.uint32)}
    out = _checked_outs(out, dtypes, want, codes.shape)
    c = side.context(codes)
    st = backend._UpExtremeStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), codes.shape, dtypes[name], c)
                for name in want}
        side.call(c, "hdem_upextreme_u8", side.address(codes), *codes.shape,
                  side.address(values), value_type, mode,
                  *[side.address(outs.get(name)) for name in UE_OUTPUTS], ctypes.byref(st))
    return outs, st.as_dict()


def upextreme_dev(codes, values, mode="max", want=("extreme",), out=None):
    """Upstream extreme of a uint8 D8 code raster (``hdem_upextreme_u8_dev``): for every cell
    the least (``mode="min"``) or greatest (``"max"``) present value of ``values`` (a float32 or
    uint32 raster; a float32 NaN is absent) over the cells whose D8 path passes through it, the
    cell included.  ``want``: any of ``extreme`` (of the values' dtype; the quiet NaN where
    nothing upstream is present) and ``where`` (uint32, the flat index of the cell that holds
    it -- the smallest one among equals -- and ``0xFFFFFFFF`` where nothing is present).
    ``out``: ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the
    stats dict.  Synchronises (the call reads its counters)."""
    return _upextreme(backend._DEVICE, codes, values, mode, want, out)


def upextreme(codes, values, mode="max", want=("extreme",)):
    """Upstream extreme of host arrays (``hdem_upextreme_u8``; see :func:`upextreme_dev`):
    ``{name: ndarray}`` and the stats dict."""
    return _upextreme(backend._HOST, codes, values, mode, want, None)


def breach_args(dem, codes, want):
    """The checks of the breach that need no device; ``want`` as a tuple in the ABI's order
    (``carved`` is always written)."""
    shape = backend._check(dem, np.float32, "depression breaching takes", "a float32 DEM",
                           flat="depression breaching takes")
    if codes is None:
        raise ValueError("depression breaching needs the D8 codes it carves along")
    backend._check(codes, np.uint8, "the codes are", "uint8 D8 codes")
    backend._check(codes, None, "the codes are", like=("the DEM", shape))
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in BR_OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown depression breaching outputs {unknown}: choose among {names}")
    return tuple(n for n in names if n in want or n == "carved")


def _breach(side, dem, codes, want, out):
    dem = side.take("dem", dem, required=True)
    codes = side.take("codes", codes, required=True)
    want = breach_args(dem, codes, want)
    dtypes = {name: np.dtype(dtype) for name, dtype in BR_OUTPUTS}
    out = _checked_outs(out, dtypes, want, dem.shape)
    c = side.context(dem)
    st = backend._BreachStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), dem.shape, dtypes[name], c)
                for name in want}
        side.call(c, "hdem_breach_f32", side.address(dem), side.address(codes), *dem.shape,
                  *[side.address(outs.get(name)) for name, _ in BR_OUTPUTS], ctypes.byref(st))
    return outs, st.as_dict()


def breach_dev(dem, codes, want=("carved",), out=None):
    """Depression breaching of a float32 DEM along a D8 forest (``hdem_breach_f32_dev``): every
    cell is lowered to the lowest pit upstream of it where that is below it, and stays bit for
    bit otherwise.  ``want``: ``carved`` (always) and ``source`` (uint32, the flat index of the
    pit a cell was lowered to, ``0xFFFFFFFF`` where it is unchanged).  ``out``:
    ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the stats
    dict.  Synchronises."""
    return _breach(backend._DEVICE, dem, codes, want, out)


def breach(dem, codes, want=("carved",)):
    """Depression breaching of host arrays (``hdem_breach_f32``; see :func:`breach_dev`):
    ``{name: ndarray}`` and the stats dict."""
    return _breach(backend._HOST, dem, codes, want, None)
