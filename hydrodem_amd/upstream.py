"""
Longest upstream D8 flow length (``hdem_upstream_u8`` / ``hdem_upstream_u8_dev``): the
binding, written once for host arrays and device rasters with the two sides of
:mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access

import contextlib
import ctypes

import numpy as np

from . import backend

# outputs, in the order of the C ABI's pointers
UP_OUTPUTS = (("ncard", np.uint32), ("ndiag", np.uint32), ("length", np.float32))


def upstream_args(codes, cellsize, want):
    """The checks that need no device: ``codes`` is anything with ``dtype`` and ``shape`` (a
    NumPy array or a device raster).  Returns ``want`` as a tuple in the ABI's order."""
    backend._check(codes, np.uint8, "upstream flow length takes", "uint8 D8 codes",
                   flat="upstream flow length takes")
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in UP_OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown upstream flow length outputs {unknown}: choose among {names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    backend._cellsize(cellsize)
    return want


def _upstream(side, codes, cellsize, want):
    codes = side.take("codes", codes, required=True)
    want = upstream_args(codes, cellsize, want)
    c = side.context(codes)
    st = backend._UpstreamStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, None, codes.shape, dtype, c)
                for name, dtype in UP_OUTPUTS if name in want}
        side.call(c, "hdem_upstream_u8", side.address(codes), *codes.shape, float(cellsize),
                  *[side.address(outs.get(name)) for name, _ in UP_OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def upstream_dev(codes, cellsize=1.0, want=("length",)):
    """Longest upstream D8 flow length of a uint8 code raster (``hdem_upstream_u8_dev``): for
    every cell the cardinal and diagonal steps of the longest D8 path that ends there.
    ``want``: any of ``ncard``, ``ndiag`` (uint32) and ``length`` (float32).  Returns
    ``{name: DeviceRaster}`` and the stats dict.  Synchronises (the call reads its counters)."""
    return _upstream(backend._DEVICE, codes, cellsize, want)


def upstream(codes, cellsize=1.0, want=("length",)):
    """Longest upstream D8 flow length of a host array (``hdem_upstream_u8``; see
    :func:`upstream_dev`): ``{name: ndarray}`` and the stats dict."""
    return _upstream(backend._HOST, codes, cellsize, want)
