"""
Downstream D8 path sums and extremes (``hdem_flowpath_u8`` / ``hdem_flowpath_u8_dev``): the
binding, written once for host arrays and device rasters with the two sides of
:mod:`hydrodem_amd.backend`, the step-length tables and the quantisation as the kernels do it.
"""
# pylint: disable=protected-access,too-many-arguments,too-many-locals,too-many-branches

import contextlib
import ctypes
import math

import numpy as np

from . import backend

# HDEM_FLOWPATH_*
MODES = {"sum": 0, "min": 1, "max": 2}
PERS = {"step": 0, "length": 1}
VALUE_TYPES = {np.dtype(np.float32): 1, np.dtype(np.uint32): 2, np.dtype(np.uint8): 3}
VALUE_NONE = 0
# outputs, in the order of the C ABI's pointers (extreme: of the values' dtype)
FP_OUTPUTS = ("stop", "sum", "value", "extreme", "where")
SUM_OUTPUTS = ("stop", "sum", "value")
EXTREME_OUTPUTS = ("stop", "extreme", "where")
Q_MAX = 2 ** 31 - 1         # the greatest quantised cost
NOWHERE = 0xFFFFFFFF        # where: nothing on the path is present
EARTH_RADIUS = 6371008.8    # metres, the mean radius

# column of the table that a code's step takes: east-west, north-south, diagonal
_COLUMN = np.zeros(256, np.int64)
_COLUMN[[4, 64]] = 1
_COLUMN[[2, 8, 32, 128]] = 2
_HAS_DIRECTION = np.zeros(256, bool)
_HAS_DIRECTION[[1, 2, 4, 8, 16, 32, 64, 128]] = True


def step_lengths(height, cellsize=1.0):
    """The table of a grid of square cells: ``height`` rows of ``(cs, cs, cs * sqrt(2))``,
    float64."""
    cellsize = backend._cellsize(cellsize)
    height = _height(height)
    return np.tile(np.array([cellsize, cellsize, cellsize * np.sqrt(2.0)], np.float64),
                   (height, 1))


def geographic_step_lengths(height, lat_top, dlat, dlon, radius=EARTH_RADIUS):
    """The table of a geographic grid on a sphere of ``radius``: row ``y`` has its cell centres at
    latitude ``lat_top - (y + 0.5) * dlat`` degrees (``lat_top``: the raster's northern edge;
    ``dlat``, ``dlon``: the cell's extent in degrees, both positive), and holds
    ``ew = R cos(phi) dlon``, ``ns = R dlat`` (both angles in radians) and
    ``diag = hypot(ew, ns)``.  Float64 NumPy on the host."""
    height = _height(height)
    lat_top, dlat, dlon, radius = (float(v) for v in (lat_top, dlat, dlon, radius))
    if not all(math.isfinite(v) for v in (lat_top, dlat, dlon, radius)) or \
            dlat <= 0 or dlon <= 0 or radius <= 0:
        raise ValueError("dlat, dlon and radius are finite and positive and lat_top is finite, "
                         f"got {lat_top}, {dlat}, {dlon}, {radius}")
    phi = np.radians(lat_top - (np.arange(height, dtype=np.float64) + 0.5) * dlat)
    if phi.max() >= np.pi / 2 or phi.min() <= -np.pi / 2:
        raise ValueError("the cell centres must lie strictly between the poles: rows run from "
                         f"{np.degrees(phi.max())} to {np.degrees(phi.min())} degrees")
    ew = radius * np.cos(phi) * np.radians(dlon)
    ns = np.full(height, radius * np.radians(dlat))
    return np.stack([ew, ns, np.hypot(ew, ns)], axis=1)


def _height(height):
    if isinstance(height, bool) or not isinstance(height, (int, np.integer)) or height < 1:
        raise ValueError(f"the number of rows is a positive integer, got {height!r}")
    return int(height)


def table_of(step_len, height=None):
    """``step_len`` as a contiguous float64 ``(height, 3)`` array (``height=None``: of any
    number of rows), every entry finite and positive, or a ValueError."""
    try:
        table = np.ascontiguousarray(step_len, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("step_lengths is an array of (rows, 3) numbers, got "
                         f"{type(step_len)}") from None
    if table.ndim != 2 or table.shape[1] != 3 or not table.shape[0]:
        raise ValueError(f"step_lengths is an array of (rows, 3) numbers, got {table.shape}")
    if height is not None and table.shape[0] != height:
        raise ValueError(f"step_lengths is {table.shape}, the codes have {height} rows: "
                         f"({height}, 3) is wanted")
    wrong = ~(np.isfinite(table) & (table > 0))
    if wrong.any():
        raise ValueError(f"step_lengths has {int(wrong.sum())} entries that are not finite and "
                         f"positive, the first in row {int(np.argwhere(wrong)[0][0])}")
    return table


def _frac_bits(frac_bits):
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or \
            not 0 <= int(frac_bits) <= 30:
        raise ValueError(f"frac_bits is an integer in 0 ... 30, got {frac_bits!r}")
    return int(frac_bits)


def quantise_steps(codes, weights, per="step", step_len=None, frac_bits=16):
    """q of every cell as the kernel computes it, int64: per step the weight itself for uint8
    and uint32 weights and ``rint(float64(w) * 2^frac_bits)`` for float32 ones; per unit length
    ``rint((float64(w) * len) * 2^frac_bits)`` -- one rounding in the product, an exact scaling,
    one rint -- with ``len`` the entry of ``step_len`` for the cell's row and the step its code
    takes, ``w = 1`` without weights and 0 for a cell without a direction.  0 for a NaN.  Range
    checks are the caller's."""
    codes = np.asarray(codes)
    if per not in PERS:
        raise ValueError(f"per is one of {list(PERS)}, got {per!r}")
    frac_bits = _frac_bits(frac_bits)
    if weights is None:
        if per == "step":
            raise ValueError("a sum per step needs the weights it sums")
        w = np.ones(codes.shape, np.float64)
    else:
        weights = np.asarray(weights)
        if weights.dtype != np.float32 and per == "step":
            return weights.astype(np.int64)
        w = weights.astype(np.float64)
    scale = 2.0 ** frac_bits
    if per == "step":
        scaled = np.rint(w * scale)
    else:
        table = table_of(step_len, codes.shape[0])
        rows = np.arange(codes.shape[0])[:, None]
        length = table[rows, _COLUMN[codes]]
        scaled = np.where(_HAS_DIRECTION[codes], np.rint((w * length) * scale), 0.0)
    return np.where(np.isnan(scaled), 0.0, scaled).astype(np.int64)


def flowpath_args(codes, streams, threshold, mode, values, per, step_len, frac_bits, want):
    """The checks that need no device: ``codes``, ``streams`` and ``values`` are anything with
    ``dtype`` and ``shape`` (NumPy arrays or device rasters).  Returns what the C call takes --
    the stream kind, the threshold, the mode, the value type, per, frac_bits, the table as a
    contiguous float64 array or ``None`` -- and ``want`` as a tuple in the ABI's order."""
    shape = backend._check(codes, np.uint8, "the flow path takes", "uint8 D8 codes",
                           flat="the flow path takes")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode is one of {list(MODES)}, got {mode!r}")
    names = SUM_OUTPUTS if mode == "sum" else EXTREME_OUTPUTS
    if isinstance(want, str):
        want = (want,)
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown flow path outputs {unknown} in mode {mode}: choose among "
                         f"{list(names)}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {list(names)}")
    # the streams: the flow trace's rule, in its words
    kind, threshold, _ = backend.flowtrace_args(codes, streams, threshold, None, 1.0, ("stop",))
    table = None
    if mode == "sum":
        if not isinstance(per, str) or per not in PERS:
            raise ValueError(f"per is one of {list(PERS)}, got {per!r}")
        frac_bits = _frac_bits(frac_bits)
        if values is None:
            if per == "step":
                raise ValueError("a sum per step needs the weights it sums (per unit length "
                                 "they may be left out)")
            value_type = VALUE_NONE
        else:
            if np.dtype(values.dtype) not in VALUE_TYPES:
                raise ValueError("the weights are float32, uint32 or uint8, got "
                                 f"{np.dtype(values.dtype)}")
            backend._check(values, None, "the weights are", like=("the codes", shape))
            value_type = VALUE_TYPES[np.dtype(values.dtype)]
            if per == "step" and np.dtype(values.dtype) != np.float32 and frac_bits != 0:
                raise ValueError(f"integer weights per step take frac_bits 0, got {frac_bits}")
        if per == "length":
            if step_len is None:
                raise ValueError("a sum per unit length needs step_lengths, (rows, 3)")
            table = table_of(step_len, shape[0])
        elif step_len is not None:
            raise ValueError("step_lengths go with per='length'")
    else:
        if values is None:
            raise ValueError("the flow path extreme needs the values it reduces")
        if np.dtype(values.dtype) not in (np.dtype(np.float32), np.dtype(np.uint32)):
            raise ValueError(f"the values are float32 or uint32, got {np.dtype(values.dtype)}")
        backend._check(values, None, "the values are", like=("the codes", shape))
        value_type = VALUE_TYPES[np.dtype(values.dtype)]
        if per != "step" or step_len is not None or frac_bits not in (0, None):
            raise ValueError("per, step_lengths and frac_bits belong to mode 'sum'")
        frac_bits = 0
    return kind, threshold, MODES[mode], value_type, PERS[per], frac_bits, table, want


def _dtypes(mode, values):
    if mode == "sum":
        return {"stop": np.dtype(np.uint32), "sum": np.dtype(np.int64),
                "value": np.dtype(np.float32)}
    return {"stop": np.dtype(np.uint32), "extreme": np.dtype(values.dtype),
            "where": np.dtype(np.uint32)}


def _flowpath(side, codes, streams, threshold, mode, values, per, step_len, frac_bits, want, out):
    codes = side.take("codes", codes, required=True)
    streams = side.take("streams", streams, mask=True)
    values = side.take("values", values)
    kind, threshold, mode_id, value_type, per_id, frac_bits, table, want = flowpath_args(
        codes, streams, threshold, mode, values, per, step_len, frac_bits, want)
    dtypes = _dtypes(mode, values)
    out = dict(out or {})
    for name, given in out.items():
        if name not in want:
            raise ValueError(f"out has {name}, which is not wanted")
        backend._check(given, dtypes[name], f"out[{name!r}] is", like=("the codes", codes.shape))
    c = side.context(codes)
    st = backend._FlowPathStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, out.get(name), codes.shape, dtypes[name], c)
                for name in want}
        side.call(c, "hdem_flowpath_u8", side.address(codes), *codes.shape,
                  side.address(streams), kind, threshold, mode_id, side.address(values),
                  value_type, per_id, frac_bits,
                  None if table is None else table.ctypes.data,     # a host pointer on both sides
                  *[side.address(outs.get(name)) for name in FP_OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def flowpath_dev(codes, values=None, mode="sum", streams=None, threshold=None, per="step",
                 step_len=None, frac_bits=16, want=None, out=None):
    """Downstream D8 path sum or extreme of a uint8 code raster (``hdem_flowpath_u8_dev``).
    The path of a cell runs to its first stop as the flow trace defines one (``streams``,
    ``threshold``: as :func:`hydrodem_amd.backend.flowtrace_dev` takes them).

    ``mode="sum"``: the sum of the quantised costs of the steps of the path; ``values`` are the
    weights (uint8, uint32 or float32; ``None`` per unit length: pure length), ``per`` is
    ``"step"`` or ``"length"`` (``step_len``: a ``(rows, 3)`` table of east-west, north-south
    and diagonal step lengths, see :func:`step_lengths` and :func:`geographic_step_lengths`);
    ``want``: any of ``stop`` (uint32), ``sum`` (int64), ``value`` (float32
    ``sum * 2^-frac_bits``, NaN where unreached; the default).
    ``mode="min"`` / ``"max"``: the least / greatest present value of ``values`` (float32 or
    uint32; a NaN is absent) over the path, both ends included; ``want``: any of ``stop``,
    ``extreme`` (the default) and ``where`` (uint32, the holder's flat index).  ``frac_bits`` is
    ignored.

    ``out``: ``{name: DeviceRaster}`` to write into.  Returns ``{name: DeviceRaster}`` and the
    stats dict.  Synchronises (the call reads its counters)."""
    return _flowpath(backend._DEVICE, codes, streams, threshold, mode, values, per, step_len,
                     frac_bits if mode == "sum" else 0,
                     want or ("value" if mode == "sum" else "extreme"), out)


def flowpath(codes, values=None, mode="sum", streams=None, threshold=None, per="step",
             step_len=None, frac_bits=16, want=None):
    """Downstream D8 path sum or extreme of host arrays (``hdem_flowpath_u8``; see
    :func:`flowpath_dev`): ``{name: ndarray}`` and the stats dict.  A bool ``streams`` array is
    a mask."""
    return _flowpath(backend._HOST, codes, streams, threshold, mode, values, per, step_len,
                     frac_bits if mode == "sum" else 0,
                     want or ("value" if mode == "sum" else "extreme"), None)
