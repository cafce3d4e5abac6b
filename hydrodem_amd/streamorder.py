"""
Strahler stream order, Shreve magnitude and stream links (``hdem_streamorder_u8`` /
``hdem_streamorder_u8_dev``): the binding, written once for host arrays and device rasters
with the two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access

import contextlib
import ctypes

import numpy as np

from . import backend

# outputs, in the order of the C ABI's pointers
SO_OUTPUTS = (("order", np.uint8), ("magnitude", np.uint32), ("link", np.uint32))


def streamorder_args(codes, streams, threshold, want):
    """The checks that need no device: ``codes`` and ``streams`` are anything with ``dtype``
    and ``shape`` (NumPy arrays or device rasters).  The stream set is the flow trace's
    operand, checked by its rules.  Returns the stream kind, the threshold for the C call and
    ``want`` as a tuple in the ABI's order."""
    backend._check(codes, np.uint8, "stream order takes", "uint8 D8 codes",
                   flat="stream order takes")
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in SO_OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown stream order outputs {unknown}: choose among {names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    kind, threshold, _ = backend.flowtrace_args(codes, streams, threshold, None, 1.0, ("stop",))
    return kind, threshold, want


def _streamorder(side, codes, streams, threshold, want):
    codes = side.take("codes", codes, required=True)
    streams = side.take("streams", streams, mask=True)
    kind, threshold, want = streamorder_args(codes, streams, threshold, want)
    c = side.context(codes)
    st = backend._StreamOrderStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, None, codes.shape, dtype, c)
                for name, dtype in SO_OUTPUTS if name in want}
        side.call(c, "hdem_streamorder_u8", side.address(codes), *codes.shape,
                  side.address(streams), kind, threshold,
                  *[side.address(outs.get(name)) for name, _ in SO_OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def streamorder_dev(codes, streams=None, threshold=None, want=("order",)):
    """Stream order of a uint8 code raster (``hdem_streamorder_u8_dev``).  ``streams``:
    ``None`` (every cell is a stream cell), a uint8 mask raster, or a uint32 raster with
    ``threshold`` (stream where ``>= threshold``).  ``want``: any of ``order`` (uint8,
    Strahler), ``magnitude`` (uint32, Shreve) and ``link`` (uint32: 1 + flat index of the last
    cell of the cell's link).  Returns ``{name: DeviceRaster}`` and the stats dict.
    Synchronises (the call reads its counters)."""
    return _streamorder(backend._DEVICE, codes, streams, threshold, want)


def streamorder(codes, streams=None, threshold=None, want=("order",)):
    """Stream order of host arrays (``hdem_streamorder_u8``; see :func:`streamorder_dev`):
    ``{name: ndarray}`` and the stats dict.  A bool ``streams`` array is a mask."""
    return _streamorder(backend._HOST, codes, streams, threshold, want)
