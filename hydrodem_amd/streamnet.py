"""
The stream network as a table, one row per link (``hdem_streamlinks_u8`` /
``hdem_streamlinks_u8_dev``): the binding, written once for host arrays and device rasters
with the two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals

import contextlib
import ctypes

import numpy as np

from . import backend

# columns of the table, in the order of the C ABI's pointers
STREAMNET_COLUMNS = (("end", np.uint32), ("top", np.uint32), ("down", np.uint32),
                     ("order", np.uint8), ("magnitude", np.uint32), ("cells", np.uint32),
                     ("ncard", np.uint32), ("ndiag", np.uint32), ("length", np.float32),
                     ("catchment", np.uint32), ("z_top", np.float32), ("z_end", np.float32))
# the operand a column cannot do without
_NEEDS = {"order": "order", "magnitude": "magnitude", "z_top": "dem", "z_end": "dem"}
NO_LINK = 0xFFFFFFFF        # ``down`` of a link that drains into no link


def _count(count):
    if isinstance(count, bool) or int(count) != count or int(count) < 0:
        raise ValueError(f"count is the number of links, got {count!r}")
    return int(count)


def streamnet_args(codes, streams, threshold, link, order, magnitude, dem, cellsize, count,
                   columns, want_row):
    """The checks that need no device: the rasters are anything with ``dtype`` and ``shape``
    (NumPy arrays or device rasters).  The stream set is the flow trace's operand, checked by
    its rules.  ``columns``: names of :data:`STREAMNET_COLUMNS`, or ``None`` for all that the
    operands allow.  Returns the stream kind, the threshold for the C call, the count and the
    columns as a tuple in the ABI's order."""
    shape = backend._check(codes, np.uint8, "the stream network takes", "uint8 D8 codes",
                           flat="the stream network takes")
    kind, threshold, _ = backend.flowtrace_args(codes, streams, threshold, dem, cellsize,
                                                ("stop",))
    if link is None:
        raise ValueError("the stream network needs the link raster of the stream order")
    backend._check(link, np.uint32, "the links are", like=("the codes", shape))
    if order is not None:
        backend._check(order, np.uint8, "the orders are", like=("the codes", shape))
    if magnitude is not None:
        backend._check(magnitude, np.uint32, "the magnitudes are", like=("the codes", shape))
    given = {"order": order, "magnitude": magnitude, "dem": dem}
    names = [n for n, _ in STREAMNET_COLUMNS]
    if columns is None:
        columns = [n for n in names if n not in _NEEDS or given[_NEEDS[n]] is not None]
    elif isinstance(columns, str):
        columns = (columns,)
    unknown = [c for c in columns if c not in names]
    if unknown:
        raise ValueError(f"unknown stream network columns {unknown}: choose among {names}")
    columns = tuple(n for n in names if n in columns)
    for name in columns:
        if name in _NEEDS and given[_NEEDS[name]] is None:
            raise ValueError(f"the column {name} needs the {_NEEDS[name]} raster it is read from")
    if not columns and not want_row:
        raise ValueError(f"no output wanted: choose among {names}, or the row raster")
    return kind, threshold, _count(count), columns


def _streamlinks(side, codes, streams, threshold, link, order, magnitude, dem, cellsize, count,
                 columns, want_row):
    codes, link = side.take("codes", codes, required=True), side.take("link", link)
    streams = side.take("streams", streams, mask=True)
    order, magnitude, dem = (side.take("order", order), side.take("magnitude", magnitude),
                             side.take("dem", dem))
    kind, threshold, count, columns = streamnet_args(
        codes, streams, threshold, link, order, magnitude, dem, cellsize, count, columns,
        want_row)
    dtypes = dict(STREAMNET_COLUMNS)
    if not side.device:     # written where they are (``offsets``: addresses)
        table = {name: np.empty(count, dtypes[name]) for name in columns}
        offsets = {name: column.ctypes.data for name, column in table.items()}
    else:
        # one device block, downloaded and freed here: the 4-byte columns first
        by_size = sorted(columns, key=lambda name: -np.dtype(dtypes[name]).itemsize)
        host = np.empty(sum(np.dtype(dtypes[name]).itemsize for name in by_size) * count,
                        np.uint8)
        table, offsets, at = {}, {}, 0
        for name in by_size:
            n = np.dtype(dtypes[name]).itemsize * count
            table[name], offsets[name] = host[at:at + n].view(dtypes[name]), at
            at += n
        table = {name: table[name] for name in columns}
    st = backend._StreamLinksStats()
    row = None
    if count or want_row:
        c = side.context(codes)
        with contextlib.ExitStack() as stack:
            if side.device and host.size:
                block = stack.enter_context(backend.DeviceRaster.empty(host.shape, np.uint8, c))
                offsets = {name: block.ptr + at for name, at in offsets.items()}
            if want_row:
                row = side.result(stack, None, codes.shape, np.uint32, c)
            side.call(c, "hdem_streamlinks_u8", side.address(codes), *codes.shape,
                      side.address(streams), kind, threshold, side.address(link),
                      side.address(order), side.address(magnitude), side.address(dem),
                      float(cellsize), count,
                      *[offsets.get(name) if count else None for name, _ in STREAMNET_COLUMNS],
                      side.address(row), 0, ctypes.byref(st))
            if side.device and host.size:
                block.to_host(host)
    return table, row, st.as_dict()


def streamlinks_dev(codes, link, count, streams=None, threshold=None, order=None, magnitude=None,
                    dem=None, cellsize=1.0, columns=None, want_row=False):
    """One row per link of the ``link`` raster that ``streamorder_dev`` wrote for these codes
    and streams (``hdem_streamlinks_u8_dev``; ``count`` is its ``stats["links"]``).  ``order``,
    ``magnitude`` (the rasters of that call) and ``dem`` feed the columns of their name and
    ``z_top`` / ``z_end``.  Returns the table, a dict of host arrays of length ``count`` (the
    columns are gathered in one device block that is downloaded and freed here), the ``row``
    raster (a ``DeviceRaster``, the caller's to free: 1 + row on the cells of a link, 0 off the
    streams) or ``None``, and the stats dict.  ``count == 0`` without ``want_row`` allocates
    and launches nothing.  Synchronises (the call reads its validity counters)."""
    return _streamlinks(backend._DEVICE, codes, streams, threshold, link, order, magnitude, dem,
                        cellsize, count, columns, want_row)


def streamlinks(codes, link, count, streams=None, threshold=None, order=None, magnitude=None,
                dem=None, cellsize=1.0, columns=None, want_row=False):
    """The stream network table of host arrays (``hdem_streamlinks_u8``; see
    :func:`streamlinks_dev`).  A bool ``streams`` array is a mask."""
    return _streamlinks(backend._HOST, codes, streams, threshold, link, order, magnitude, dem,
                        cellsize, count, columns, want_row)
