"""
Zonal statistics, one row per zone of a label raster (``hdem_zonal_count_u32[_dev]``,
``hdem_zonal_table_u32[_dev]``, ``hdem_zonal_broadcast_dev``): the binding, written once for
host arrays and device rasters with the two sides of :mod:`hydrodem_amd.backend`.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals

import contextlib
import ctypes

import numpy as np

from . import backend

# columns of the table, in the order of the C ABI's pointers
ZONAL_COLUMNS = ("id", "count", "first", "row_min", "row_max", "col_min", "col_max", "valid",
                 "min", "max", "at_min", "at_max", "sum")
# ... those that are read off the values
VALUE_COLUMNS = ("valid", "min", "max", "at_min", "at_max", "sum")
# HDEM_ZONAL_*
VALUE_TYPES = {np.dtype(np.float32): 1, np.dtype(np.uint32): 2, np.dtype(np.uint8): 3}
NO_CELL = 0xFFFFFFFF        # ``at_min`` / ``at_max`` of a zone without a valid cell


def column_dtype(name, values_dtype=None):
    """The dtype of column ``name``: ``min`` and ``max`` have the values' own, ``sum`` is int64
    for float32 values (a sum of quantised values) and uint64 for the integer types."""
    if name in ("min", "max"):
        return np.dtype(values_dtype)
    if name == "sum":
        return np.dtype(np.int64 if np.dtype(values_dtype) == np.float32 else np.uint64)
    return np.dtype(np.uint32)


def zonal_args(zones, values=None, columns=None, frac_bits=16):
    """The checks that need no device: the rasters are anything with ``dtype`` and ``shape``
    (NumPy arrays or device rasters).  ``columns``: names of :data:`ZONAL_COLUMNS`, or ``None``
    for all that the operands allow.  Returns the value type for the C call, ``frac_bits`` and
    the columns as a tuple in the ABI's order."""
    shape = backend._check(zones, np.uint32, "zonal statistics take", "uint32 zone ids",
                           flat="zonal statistics take")
    value_type = 0
    if values is not None:
        if np.dtype(values.dtype) not in VALUE_TYPES:
            raise ValueError("the values are float32, uint32 or uint8, got "
                             f"{np.dtype(values.dtype)}")
        backend._check(values, None, "the values are", like=("the zones", shape))
        value_type = VALUE_TYPES[np.dtype(values.dtype)]
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= 30:
        raise ValueError(f"frac_bits is an integer in 0 ... 30, got {frac_bits!r}")
    if columns is None:
        columns = [n for n in ZONAL_COLUMNS if values is not None or n not in VALUE_COLUMNS]
    elif isinstance(columns, str):
        columns = (columns,)
    unknown = [c for c in columns if c not in ZONAL_COLUMNS]
    if unknown:
        raise ValueError(f"unknown zonal columns {unknown}: choose among {list(ZONAL_COLUMNS)}")
    columns = tuple(n for n in ZONAL_COLUMNS if n in columns)
    for name in columns:
        if name in VALUE_COLUMNS and values is None:
            raise ValueError(f"the column {name} needs the values it is read from")
    if not columns:
        raise ValueError(f"no column wanted: choose among {list(ZONAL_COLUMNS)}")
    return value_type, int(frac_bits), columns


def _count(side, zones):
    c = side.context(zones)
    st, count = backend._ZonalStats(), ctypes.c_int64(0)
    side.call(c, "hdem_zonal_count_u32", side.address(zones), *zones.shape, ctypes.byref(count),
              ctypes.byref(st))
    return int(count.value), st.as_dict()


def _table(side, zones, values, count, value_type, frac_bits, columns):
    dtypes = {name: column_dtype(name, None if values is None else values.dtype)
              for name in columns}
    if not side.device:     # written where they are (``offsets``: addresses)
        table = {name: np.empty(count, dtypes[name]) for name in columns}
        offsets = {name: column.ctypes.data for name, column in table.items()}
    else:
        # one device block, downloaded and freed here: the widest columns first.  Its host twin
        # is page-locked when it is large (a table of lakes has millions of rows)
        by_size = sorted(columns, key=lambda name: -dtypes[name].itemsize)
        host = backend.host_empty((sum(dtypes[name].itemsize for name in by_size) * count,),
                                  np.uint8)
        table, offsets, at = {}, {}, 0
        for name in by_size:
            n = dtypes[name].itemsize * count
            table[name], offsets[name] = host[at:at + n].view(dtypes[name]), at
            at += n
        table = {name: table[name] for name in columns}
    st = backend._ZonalStats()
    c = side.context(zones)
    with contextlib.ExitStack() as stack:
        if side.device:
            block = stack.enter_context(backend.DeviceRaster.empty(host.shape, np.uint8, c))
            offsets = {name: block.ptr + at for name, at in offsets.items()}
        side.call(c, "hdem_zonal_table_u32", side.address(zones), *zones.shape,
                  side.address(values), value_type, frac_bits, count,
                  *[offsets.get(name) for name in ZONAL_COLUMNS], 0, ctypes.byref(st))
        if side.device:
            block.to_host(host)
    return table, st.as_dict()


def with_mean(table, values_dtype, frac_bits):
    """``table`` plus ``mean``, derived on the host in float64 as ``sum / 2^frac_bits / valid``
    (integer values: ``sum / valid``), NaN where ``valid`` is 0; only when both are there."""
    if "sum" in table and "valid" in table:
        scale = 2.0 ** frac_bits if np.dtype(values_dtype) == np.float32 else 1.0
        valid = table["valid"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = table["sum"].astype(np.float64) / scale / valid
        table["mean"] = np.where(table["valid"] == 0, np.nan, mean)
    return table


def _zonal(side, zones, values, columns, frac_bits):
    zones = side.take("zones", zones, required=True)
    values = side.take("values", values)
    value_type, frac_bits, columns = zonal_args(zones, values, columns, frac_bits)
    count, stats = _count(side, zones)
    if count:
        table, table_stats = _table(side, zones, values, count, value_type, frac_bits, columns)
        stats = dict(table_stats, ms_count=stats["ms_rank"])
    else:       # no zone: empty columns, nothing more to launch
        dtype = None if values is None else values.dtype
        table = {name: np.empty(0, column_dtype(name, dtype)) for name in columns}
        stats = dict(stats, ms_count=stats["ms_rank"], ms_rank=0.0)
    return with_mean(table, None if values is None else values.dtype, frac_bits), stats


def zonal_count_dev(zones):
    """K, the number of zone ids present in a uint32 device raster, and the stats dict
    (``hdem_zonal_count_u32_dev``).  ``ValueError`` for an id above H * W."""
    zonal_args(zones)
    return _count(backend._DEVICE, zones)


def zonal_count(zones):
    """K and the stats dict of a host array (``hdem_zonal_count_u32``)."""
    zones = backend._HOST.take("zones", zones, required=True)
    zonal_args(zones)
    return _count(backend._HOST, zones)


def zonal_dev(zones, values=None, columns=None, frac_bits=16):
    """One row per zone of the uint32 device raster ``zones`` (0: no zone), in ascending id: the
    table, a dict of host arrays in the order of :data:`ZONAL_COLUMNS` (the columns are gathered
    in one device block that is downloaded and freed here) plus the derived ``mean``, and the
    stats dict.  Two C calls: the count, then the table.  Ids lie in 1 ... H * W, as every label
    raster of this library has them; arbitrary pour-point labels are relabelled first.
    Synchronises (each call reads its counters)."""
    return _zonal(backend._DEVICE, zones, values, columns, frac_bits)


def zonal(zones, values=None, columns=None, frac_bits=16):
    """The zonal table of host arrays (``hdem_zonal_count_u32``, ``hdem_zonal_table_u32``; see
    :func:`zonal_dev`)."""
    return _zonal(backend._HOST, zones, values, columns, frac_bits)


def zonal_broadcast_dev(zones, column, fill=0, out=None):
    """``out[c] = column[row of zones[c]]`` and ``fill`` where ``zones[c] == 0``
    (``hdem_zonal_broadcast_dev``): ``column`` is a host array of K 4-byte entries, one per zone
    in ascending id; a device raster of its dtype comes back (the caller's to free)."""
    zonal_args(zones)
    column = np.ascontiguousarray(column)
    if column.ndim != 1 or column.dtype.itemsize != 4 or column.dtype not in backend._DTYPES:
        raise ValueError("a column to broadcast is one-dimensional with 4-byte entries, got "
                         f"{column.dtype} {column.shape}")
    word = int(np.array([fill]).astype(column.dtype).view(np.uint32)[0])
    c = zones.ctx
    with contextlib.ExitStack() as stack:
        dcol = None
        if column.size:
            dcol = stack.enter_context(backend.DeviceRaster.empty(column.shape, column.dtype, c))
            c.check(c.lib.hdem_memcpy_h2d(c.handle, dcol.ptr, column.ctypes.data, column.nbytes))
        out = stack.enter_context(backend.result_raster(out, zones.shape, column.dtype, c))
        c.check(c.lib.hdem_zonal_broadcast_dev(c.handle, zones.ptr, *zones.shape, column.size,
                                               None if dcol is None else dcol.ptr, word, out.ptr))
    return out
