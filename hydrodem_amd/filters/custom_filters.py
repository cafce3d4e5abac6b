"""
Stencil operators of the hot path, backed by the HIP library.

Reference twins (`cguerrero/hydrodem/filters/custom_filters.py`):
``QuadraticFilter`` :202-257, ``MaskTallGroves`` :513-534,
``GrovesCorrection`` :664-732, ``GrovesCorrectionsIter`` :735-767,
``PostProcessingFinal`` :1104-1125 -- same class names, constructor
signatures, mutable operand attributes and error classes.

Fourier destripe branch: ``ExpandFilter`` :76-125,
``IsolatedPoints`` :320-366, ``BlanksFourier`` :369-429,
``DetectBlanksFourier`` :432-462, ``MaskFourier`` :537-561, ``FourierInitial``
:834-877, ``FourierProcessQuarters`` :880-1050, ``DetectApplyFourier``
:1053-1101.

Lagoon branch: ``MajorityFilter`` :22-73, ``CorrectNANValues``
:260-317, ``MaskNegatives`` / ``MaskPositives`` :465-510, ``TidyingLagoons``
:564-610, ``LagoonsDetection`` :613-661.

River branch (host side only -- ``RouteRivers`` is a serial scan by
construction, SURVEY section 2 #9 / 8e "not shardable"; no kernel is wanted):
``RouteRivers`` :128-199, ``ProcessRivers`` :770-798, ``ClipLagoonsRivers``
:801-831.  They exist so that `image_hsheds.py:6-7,203-205` imports and runs
unchanged when ``filters`` resolves here.

New operators (the reference has neither): ``SinkFill``,
``D8FlowDirection``, ``ResolveFlats``, ``FlowAccumulation``, ``WeightedFlowAccumulation``,
``UpstreamExtreme``, ``BreachDepressions``, ``Watersheds``, ``FlowDistance``,
``FlowPathSum``, ``FlowPathExtreme``, ``HeightAboveDrainage``, ``UpstreamFlowLength``,
``StreamOrder``, ``StreamNetwork``, ``DInfFlowDirection``, ``DInfFlowAccumulation``,
``WeightedDInfFlowAccumulation``, ``AreaWetnessIndex``, ``DInfDistanceDown``,
``DInfHeightAboveDrainage``, ``DInfDistanceUp``, ``MFDFlowDirection``, ``MFDFlowAccumulation``,
``CostDistance``, ``CostAllocation``, ``CostPath``
and the chains ``DemToHAND``, ``DemToStreamOrder``, ``DemToStreamNetwork``, ``DemToDInfArea``,
``DemToDInfWetness``, ``DemToDInfHAND``, ``DemToDInfDistanceUp`` and ``DemToMFDArea``, shaped
like every other ``Filter``.

Module namespace.  The reference's ``custom_filters`` is also where its callers
pick up the element-wise and SciPy wrappers (`image_srtm.py:7-8` takes
``BinaryClosing`` from here, `hydro_dem_process.py:20-21` ``AdditionFilter``),
because `custom_filters.py:9-19` imports them at module level.  The imports
below bind the same complete set of names.

Storage type.  The device path stores rasters as float32 (what GDAL hands the
reference, `image_srtm.py:125`).  The reference drifts to float64 after the
first groves pass (float32 * int64); the values agree to <= 1 float32 ulp and
every reference stencil re-reads its input through ``astype('float32')``
anyway (`sliding_window.py:132`).
"""

import contextlib
import copy
from collections import Counter  # noqa: F401  (name of the reference module's namespace)

import numpy as np

from . import Filter, ComposedFilter, ComposedFilterResults
from .simple_filters import (LowerThan, BooleanToInteger, GreaterThan,  # noqa: F401
                             ProductFilter, SubtractionFilter, AdditionFilter)
from .extension_filters import (BitwiseXOR, BinaryErosion, Around,  # noqa: F401
                                BinaryClosing, GreyDilation, Convolve,
                                FourierITransform, FourierTransform,
                                FourierShift, FourierIShift, AbsoluteValues)
from ..sliding_window import (SlidingWindow, CircularWindow,  # noqa: F401
                              NoCenterWindow, IgnoreBorderInnerSliding)
from .. import backend
from .. import upstream as _upstream
from .. import streamorder as _streamorder
from .. import streamnet as _streamnet
from .. import zonal as _zonal
from .. import terrain as _terrain
from .. import proximity as _proximity
from .. import flowsum as _flowsum
from .. import upextreme as _upextreme
from .. import flowpath as _flowpath
from .. import dinf as _dinf
from .. import mfd as _mfd
from .. import costdistance as _costdistance


def _check_raster(name, raster, dtype, takes):
    """``raster`` (a host array or a device raster) is 2-D and of ``dtype``, or a ValueError
    in the words of the operator ``name``, which ``takes`` that kind of raster."""
    backend._check(raster, dtype, f"{name} takes", takes,  # pylint: disable=protected-access
                   flat=f"{name} takes")


class _Given:  # pylint: disable=too-few-public-methods
    """An operand given at construction (a dem, streams, a seeds raster): ``value`` is a NumPy
    array or a device raster (a bool mask as bytes) or ``None``, checked when it comes with a
    ``name`` to be that, 2-D and of one of ``dtypes``; ``host()`` and ``device(ctx)`` give it
    in the form an operator needs, whichever it was given in."""

    def __init__(self, operand, name=None, dtypes=()):
        if name is not None and operand is not None:
            if not (isinstance(operand, np.ndarray) or backend.is_device_raster(operand)):
                raise ValueError(f"{name} is a NumPy array or a DeviceRaster, got "
                                 f"{type(operand)}")
            if len(operand.shape) != 2:
                raise ValueError(f"{name} is a 2-D raster, got {len(operand.shape)} dimensions")
            if np.dtype(operand.dtype) not in [np.dtype(k) for k in dtypes]:
                raise ValueError(f"{name} has dtype {' or '.join(np.dtype(k).name for k in dtypes)}"
                                 f", got {operand.dtype}")
        if isinstance(operand, np.ndarray) and operand.dtype == np.bool_:
            operand = operand.view(np.uint8)
        self.value = operand

    def host(self):
        return self.value.to_host() if backend.is_device_raster(self.value) else self.value

    def device(self, ctx):
        """For the length of a ``with``: see ``backend.on_device``."""
        return backend.on_device(self.value, ctx=ctx)

    def stand_in(self):
        """A 1 x 1 array of the operand's dtype, for the checks that come before a shape."""
        return None if self.value is None else np.empty((1, 1), self.value.dtype)


def _fill_d8(stack, raster, fill, flats):
    """Fill + D8 of a device raster in one call (the certifying pass of the fill writes the
    flow directions) with the operands of ``fill``, the ``SinkFill`` member, then
    ``ResolveFlats`` on the codes in place when ``flats`` says so: the filled raster and the
    codes, both entered in ``stack``, and the resolution's stats (``None`` without one)."""
    filled, codes, fill.stats = backend.sinkfill_d8_dev(raster, eps=fill.epsilon,
                                                        max_rounds=fill.max_rounds)
    stack.enter_context(filled)
    stack.enter_context(codes)
    resolve_stats = None
    if flats == "resolve":
        _, _, resolve_stats = backend.resolve_flats_dev(codes, filled, out=codes)
    return filled, codes, resolve_stats


def _through_device(operator, image, kept=()):
    """``operator.apply_device`` for a host array: upload, apply, download the result and the
    rasters the operator left in its attributes ``kept``, host arrays afterwards."""
    with backend.DeviceRaster.from_host(image, dtype=np.float32) as z, \
            contextlib.ExitStack() as stack:
        result = stack.enter_context(operator.apply_device(z))
        rasters = [stack.enter_context(getattr(operator, name)) for name in kept]
        for name in kept:
            setattr(operator, name, None)
        out = result.to_host()
        for name, raster in zip(kept, rasters):
            setattr(operator, name, raster.to_host())
    return out


class QuadraticFilter(Filter):  # pylint: disable=too-few-public-methods
    """Least-squares quadratic smoothing over a ``window_size`` square window;
    the ring of ``window_size // 2`` cells is returned unchanged
    (custom_filters.py:202-257).  Window validation raises the same
    ``WindowSizeHighError`` / ``WindowSizeEvenError`` as the reference's
    ``SlidingWindow`` constructor (sliding_window.py:150-156)."""

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, *, window_size):
        self.window_size = window_size

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        return backend.quadratic(image_to_filter, self.window_size)

    def apply_device(self, raster):
        return backend.quadratic_dev(raster, self.window_size)


class MaskTallGroves(ComposedFilter):  # pylint: disable=too-few-public-methods
    """``(image > 1.5) * 1`` (custom_filters.py:513-534).  Host NumPy; inside
    ``GrovesCorrection`` this algebra runs in the fused kernel's epilogue."""

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [GreaterThan(value=1.5), BooleanToInteger()]


class GrovesCorrection(ComposedFilter):  # pylint: disable=too-few-public-methods
    """One groves correction pass (custom_filters.py:664-732):

        smooth = QuadraticFilter(15)(img); hl = img - smooth
        m = groves_class * (hl > 1.5);     out = hl * (1 - m) + smooth

    evaluated by ONE fused HIP kernel when ``groves_class`` is a 0 / 1 mask (what
    `image_srtm.py:177-178` passes: a ``binary_closing`` result); a class raster with
    other values takes the reference's algebra literally -- ``m = class * tall`` --
    member by member, with only the quadratic filter on the GPU.  ``filters`` keeps
    the reference's five
    members so that callers can still re-bind their operands
    (``filters[3].factor`` is the groves class, ``filters[0].window_size`` the
    window, ``filters[2].filters[0].value`` the tall-grove threshold); they
    are read at ``apply`` time.  ``partial_results`` is filled only with
    ``keep_partial_results=True`` (it costs an extra quadratic pass)."""

    @property
    def auto_device(self):
        """Device form == host form for a float32 raster -- with a 0 / 1 class raster."""
        return self._is_mask(self._params()[0])

    def __init__(self, groves_class, keep_partial_results=False):  # pylint: disable=super-init-not-called
        self.partial_results = []
        self.keep_partial_results = keep_partial_results
        self.filters = [QuadraticFilter(window_size=15), SubtractionFilter(),
                        MaskTallGroves(), ProductFilter(factor=groves_class),
                        SubtractionFilter(minuend=1)]

    def _params(self):
        return (self.filters[3].factor, self.filters[0].window_size,
                self.filters[2].filters[0].value)

    @staticmethod
    def _is_mask(groves_class):
        """Only 0 and 1 in the class raster (then the fused kernel's `class != 0` is the
        reference's product with the class)."""
        g = np.asarray(groves_class)
        if g.dtype == bool or g.size == 0:
            return True
        if g.dtype.kind in "ui":                       # one or two SIMD passes, no temporaries
            return bool(g.max() <= 1 and (g.dtype.kind == "u" or g.min() >= 0))
        return not np.any((g != 0) & (g != 1))

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        groves_class, window, thr = self._params()
        if not self._is_mask(groves_class):
            # custom_filters.py:724-732 as written: highlight * (1 - class * tall) + smooth
            smooth = backend.quadratic(image_to_filter, window)
            highlight = image_to_filter - smooth
            product = groves_class * ((highlight > thr) * 1)
            if self.keep_partial_results:
                self.partial_results = [smooth, highlight, (highlight > thr) * 1, product,
                                        1 - product]
            return highlight * (1 - product) + smooth
        if self.keep_partial_results:
            img = np.ascontiguousarray(image_to_filter, dtype=np.float32)
            smooth = backend.quadratic(img, window)
            highlight = img - smooth
            tall = (highlight > thr) * 1
            product = groves_class * tall
            self.partial_results = [smooth, highlight, tall, product, 1 - product]
        return backend.groves(image_to_filter, groves_class, window, thr, 1)

    def apply_device(self, raster):
        groves_class, window, thr = self._params()
        if not self._is_mask(groves_class):
            raise NotImplementedError("the fused groves kernel takes a 0 / 1 class raster")
        with backend.on_device(backend.mask_bytes(groves_class), np.uint8, raster.ctx) as g:
            out = backend.groves_dev(raster, g, window, thr, 1)
            raster.ctx.synchronize()
        return out


class GrovesCorrectionsIter(ComposedFilter):  # pylint: disable=too-few-public-methods
    """``iterations`` chained ``GrovesCorrection`` passes
    (custom_filters.py:735-767).  When the members are untouched the whole
    chain is one C call that ping-pongs two device buffers."""

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, groves_class, iterations=3):  # pylint: disable=super-init-not-called
        self.filters = []
        for _ in range(iterations):
            self.filters.append(GrovesCorrection(groves_class))

    def _uniform(self):
        if not self.filters or not all(type(f) is GrovesCorrection and
                                       not f.keep_partial_results
                                       for f in self.filters):
            return None
        p0 = self.filters[0]._params()
        for f in self.filters[1:]:
            p = f._params()
            if p[0] is not p0[0] or p[1:] != p0[1:]:
                return None
        if not GrovesCorrection._is_mask(p0[0]):
            return None                     # member by member: the reference's algebra
        return p0

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        params = self._uniform()
        if params is None:
            return ComposedFilter.apply(self, image_to_filter)
        groves_class, window, thr = params
        return backend.groves(image_to_filter, groves_class, window, thr,
                              len(self.filters))

    def apply_device(self, raster):
        params = self._uniform()
        if params is None:
            return ComposedFilter.apply_device(self, raster)
        groves_class, window, thr = params
        with backend.on_device(backend.mask_bytes(groves_class), np.uint8, raster.ctx) as g:
            out = backend.groves_dev(raster, g, window, thr, len(self.filters))
            raster.ctx.synchronize()
        return out


class PostProcessingFinal(ComposedFilter):  # pylint: disable=too-few-public-methods
    """3x3 box mean then round to 1 m (custom_filters.py:1104-1125).  With the
    default members the two run as one fused kernel (float32 or float64)."""

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [Convolve(), Around()]

    def _fused(self):
        return (len(self.filters) == 2 and type(self.filters[0]) is Convolve
                and self.filters[0]._is_box3() and type(self.filters[1]) is Around)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        if self._fused():
            return backend.boxmean3(image_to_filter, do_round=True)
        content = image_to_filter
        for filter_ in self.filters:
            content = filter_.apply(content)
        return content

    def apply_device(self, raster):
        if not self._fused():
            raise NotImplementedError("device chain needs the default members")
        return backend.boxmean3_dev(raster, do_round=True)


class SinkFill(Filter):  # pylint: disable=too-few-public-methods
    """Depression filling (new operator; normative definition SURVEY 8a A1).

    ``W = max(Z, spill elevation)``: the greatest fixed point of
    ``W[c] = max(Z[c], min(W[c], min8(W[n] + epsilon)))`` with the one-cell
    border pinned to Z ("interior only, border untouched", the convention of
    `sliding_window.py:187-192`); nodata (NaN) cells stay NaN and act as
    outlets.  ``epsilon = 0`` gives flats and is bit-reproducible.

    Attributes
    ----------
    epsilon : float
        Planchon-Darboux gradient added per step (metres), default 0.
    max_rounds : int
        Worklist-round limit; 0 = library default.  ``NotConvergedError`` when
        it is hit.
    stats : dict
        rounds / tile_visits / tiles of the last ``apply``.
    """

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, *, epsilon=0.0, max_rounds=0):
        self.epsilon = epsilon
        self.max_rounds = max_rounds
        self.stats = {}

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        out, self.stats = backend.sinkfill(image_to_filter, self.epsilon,
                                           self.max_rounds, return_stats=True)
        return out

    def apply_device(self, raster):
        out, self.stats = backend.sinkfill_dev(raster, self.epsilon, self.max_rounds)
        return out


class D8FlowDirection(Filter):  # pylint: disable=too-few-public-methods
    """D8 steepest-descent direction (new operator): ESRI codes
    E=1, SE=2, S=4, SW=8, W=16, NW=32, N=64, NE=128, 0 = no lower neighbour or
    border cell; drop = (z_c - z_k) / distance evaluated in float32 as
    ``(z_c - z_k) * w_k``, w = 1 or float32(0.70710678); ties go to the first
    neighbour in window order NW, N, NE, W, E, SW, S, SE (the order
    ``np.nonzero`` gives `custom_filters.py:193-195`).  Returns uint8."""

    auto_device = True      # device form == host form for a float32 raster

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        return backend.d8(image_to_filter)

    def apply_device(self, raster):
        return backend.d8_dev(raster)


class FlowAccumulation(Filter):  # pylint: disable=too-few-public-methods
    """D8 flow accumulation (new operator).  Input: a uint8 H x W raster of ESRI D8
    codes as ``D8FlowDirection`` returns them (E=1, SE=2, S=4, SW=8, W=16, NW=32, N=64,
    NE=128); code 0, or a code that points outside the raster, makes a cell terminal.
    Returns uint32: ``acc[c]`` is the number of cells whose D8 path passes through ``c``,
    ``c`` included, so every cell is >= 1 -- the unique solution of
    ``acc[c] = 1 + sum(acc[d])`` over the neighbours ``d`` whose code points at ``c``.
    Exact integers, identical from run to run.

    Nodata: NaN cells of a DEM get code 0 from D8 and are never chosen as a receiver,
    so they read 1; masking them is the caller's job.

    ``ValueError`` for a dtype other than uint8 or a raster that is not 2-D (checked
    before the device is touched), for a byte that is not a D8 code, for codes that form
    a cycle (only user-supplied codes can: D8 always points to a strictly lower cell) and
    for more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        exits (nodes of the exit forest), max_hops (tile crossings of the longest forest
        walk), tile_h / tile_w of the last call; phase times when profiling is on.
    """

    auto_device = True      # device form == host form for a uint8 code raster

    def __init__(self):
        self.stats = {}

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        _check_raster("FlowAccumulation", image_to_filter, np.uint8, "uint8 D8 codes")
        out, self.stats = backend.flowacc(image_to_filter, return_stats=True)
        return out

    def apply_device(self, raster):
        _check_raster("FlowAccumulation", raster, np.uint8, "uint8 D8 codes")
        out, self.stats = backend.flowacc_dev(raster)
        return out


class WeightedFlowAccumulation(Filter):  # pylint: disable=too-few-public-methods
    """Weighted D8 flow accumulation (new operator; ArcGIS *Flow Accumulation* with a weight
    raster, TauDEM ``aread8 -wg``).  Input: a uint8 H x W raster of ESRI D8 codes exactly as
    ``FlowAccumulation`` takes them.  ``weights``: an H x W NumPy array or ``DeviceRaster`` of
    uint8, uint32 or float32 (float64 is refused, not narrowed).  Every cell's weight is
    quantised to an integer ``q``: the weight itself for the integer types, which take
    ``frac_bits=0``, and ``rint(float64(w) * 2^frac_bits)`` for float32, ``frac_bits`` 0 ... 30.
    ``S[c] = q[c] + sum(S[d])`` over the neighbours ``d`` whose code points at ``c`` is summed in
    int64: exact, identical from run to run.

    ``output`` fixes what ``apply`` returns: ``"sum"`` int64 ``S``; ``"value"`` float32
    ``float32(float64(S) * 2^-frac_bits)``; ``"mask"`` uint8, 1 where
    ``S >= ceil(threshold * 2^frac_bits)``, with ``threshold`` in weight units -- a stream mask
    for ``FlowDistance``, ``HeightAboveDrainage``, ``StreamOrder``, ``StreamNetwork``,
    ``EuclideanDistance`` and ``BurnStreams``.

    A NaN weight contributes 0 (``stats["nan_weights"]`` counts them).  ``ValueError`` for
    operands of another type, dtype or shape, ``frac_bits`` out of range, a ``threshold`` that
    does not go with the output or comes out below 1 (all before the device is touched), for a
    negative or infinite weight, a quantised weight above 2^31 - 1 (so that no sum can
    overflow), a byte that is not a D8 code, codes that form a cycle and more than 2^32 - 1
    cells.

    Attributes
    ----------
    stats : dict
        nan_weights, exits (nodes of the exit forest), max_hops (tile crossings of the longest
        forest walk), tile_h / tile_w of the last call; phase times when profiling is on.
    """

    auto_device = True      # device form == host form for a uint8 code raster
    WEIGHT_TYPES = (np.uint8, np.uint32, np.float32)
    OUTPUTS = {name: np.dtype(dtype) for name, dtype in _flowsum.FS_OUTPUTS}

    def __init__(self, weights, frac_bits=16, output="value", threshold=None):
        if weights is None:
            raise ValueError("WeightedFlowAccumulation needs the weights it sums")
        self.weights = _Given(weights, "weights", self.WEIGHT_TYPES).value
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self.frac_bits, self.output, self.threshold = frac_bits, output, threshold
        self.dtype = self.OUTPUTS[output]
        self.stats = {}
        # everything but the shapes, on 1 x 1 stand-ins
        _flowsum.flowsum_args(np.empty((1, 1), np.uint8), _Given(self.weights).stand_in(),
                              frac_bits, output, threshold)

    def _args(self, codes):
        _flowsum.flowsum_args(codes, self.weights, self.frac_bits, self.output, self.threshold)

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        self._args(image_to_filter)
        outs, self.stats = _flowsum.flowsum(image_to_filter, _Given(self.weights).host(),
                                            self.frac_bits, self.output, self.threshold)
        return outs[self.output]

    def apply_device(self, raster):
        self._args(raster)
        with _Given(self.weights).device(raster.ctx) as weights:
            outs, self.stats = _flowsum.flowsum_dev(raster, weights, self.frac_bits,
                                                    self.output, self.threshold)
        return outs[self.output]


class UpstreamExtreme(Filter):  # pylint: disable=too-few-public-methods
    """Upstream D8 minimum or maximum (new operator; TauDEM ``d8flowpathextremeup``).  Input: a
    uint8 H x W raster of ESRI D8 codes exactly as ``FlowAccumulation`` takes them.  ``values``:
    an H x W NumPy array or ``DeviceRaster`` of float32 or uint32 (float64 is refused, not
    narrowed).  For every cell, over the cell and every cell whose D8 path passes through it,
    the least (``mode="min"``) or greatest (``mode="max"``) present value.  A float32 NaN is
    absent (``stats["absent"]`` counts them); floats are ordered
    ``-inf < ... < -0.0 < +0.0 < ... < +inf``.

    ``output`` fixes what ``apply`` returns: ``"extreme"``, of the values' dtype, the bits of
    the cell that holds the extreme (the quiet NaN where nothing upstream is present), or
    ``"where"``, uint32, that cell's flat index (``0xFFFFFFFF`` where nothing is present).
    Among cells that hold the same value the smallest flat index is the holder, in both modes.
    Min and max are reductions on a total order: identical from run to run.

    ``ValueError`` for operands of another type, dtype or shape, an unknown ``mode`` or
    ``output`` (all before the device is touched), a byte that is not a D8 code, codes that form
    a cycle and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        absent, exits (nodes of the exit forest), max_hops (tile crossings of the longest
        forest walk), tile_h / tile_w of the last call; phase times when profiling is on.
    """

    auto_device = True      # device form == host form for a uint8 code raster
    VALUE_TYPES = (np.float32, np.uint32)

    def __init__(self, values, mode="max", output="extreme"):
        if values is None:
            raise ValueError("UpstreamExtreme needs the values it reduces")
        self.values = _Given(values, "values", self.VALUE_TYPES).value
        if not isinstance(output, str) or output not in _upextreme.UE_OUTPUTS:
            raise ValueError(f"output is one of {list(_upextreme.UE_OUTPUTS)}, got {output!r}")
        self.mode, self.output = mode, output
        self.dtype = np.dtype(np.uint32) if output == "where" else np.dtype(self.values.dtype)
        self.stats = {}
        # everything but the shapes, on 1 x 1 stand-ins
        _upextreme.upextreme_args(np.empty((1, 1), np.uint8), _Given(self.values).stand_in(),
                                  mode, output)

    def _args(self, codes):
        _upextreme.upextreme_args(codes, self.values, self.mode, self.output)

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        self._args(image_to_filter)
        outs, self.stats = _upextreme.upextreme(image_to_filter, _Given(self.values).host(),
                                                self.mode, self.output)
        return outs[self.output]

    def apply_device(self, raster):
        self._args(raster)
        with _Given(self.values).device(raster.ctx) as values:
            outs, self.stats = _upextreme.upextreme_dev(raster, values, self.mode, self.output)
        return outs[self.output]


class Watersheds(Filter):  # pylint: disable=too-few-public-methods
    """D8 watershed labelling (new operator).  Input: a uint8 H x W raster of ESRI D8 codes
    exactly as ``FlowAccumulation`` takes them; code 0, or a code that points outside the
    raster, makes a cell terminal.  Returns uint32 labels.

    ``Watersheds()``: ``label[c]`` is 1 + the flat index ``y * W + x`` of the terminal
    cell that ``c``'s D8 path ends in (a terminal cell labels itself), so every cell is
    >= 1.  NaN cells of a DEM get code 0 from D8: each is its own one-cell basin; masking
    them is the caller's job.

    ``Watersheds(labels="compact")``: the same basins numbered 1 ... K, K the number of
    terminal cells; ``outlets`` (uint32, K flat indices) maps label ``k`` to
    ``outlets[k - 1]``.  The numbering is fixed for a raster (by 64 x 64 tile, row-major
    inside a tile) and the same from ``apply`` and ``apply_device``.

    ``Watersheds(pour_points=...)``: ``label[c]`` is the label of the first pour point on
    ``c``'s path, ``c`` included, and 0 when the path ends without meeting one, so nested
    pour points give sub-catchments.  ``pour_points`` is a seeds raster of the codes'
    shape (any integer dtype whose values fit uint32, or a uint32 ``DeviceRaster``; 0 = no
    pour point, anything else that cell's label) or a sequence (not an array: an array is
    a raster) of ``(row, col)`` / ``(row, col, label)``; bare pairs are labelled 1 ... n
    in order.

    ``ValueError`` for codes that are not a 2-D uint8 raster, seeds of another shape or
    dtype, coordinates outside the raster, label 0, ``compact`` together with pour points
    (all before the device is touched), a byte that is not a D8 code, codes that form a
    cycle (in pour-point mode a loop that holds a pour point is legal) and more than
    2^32 - 1 cells.  Exact integers, identical from run to run.

    Attributes
    ----------
    stats : dict
        basins (terminal cells), exits, forest_rounds, tile_h / tile_w of the last call;
        phase times when profiling is on.
    outlets : numpy.ndarray or None
        the outlets of the compact numbering of the last call.
    """

    auto_device = True      # device form == host form for a uint8 code raster

    def __init__(self, pour_points=None, labels="outlet"):
        if labels not in ("outlet", "compact"):
            raise ValueError(f"labels is 'outlet' or 'compact', got {labels!r}")
        if labels == "compact" and pour_points is not None:
            raise ValueError("compact labels number the outlets: they cannot be combined "
                             "with pour points")
        self.labels = labels
        self.stats = {}
        self.outlets = None
        self._seeds = self._points = None
        if pour_points is None:
            return
        if backend.is_device_raster(pour_points):
            if pour_points.dtype != np.uint32 or len(pour_points.shape) != 2:
                raise ValueError("a device seeds raster is 2-D uint32, got "
                                 f"{pour_points.dtype} {tuple(pour_points.shape)}")
            self._seeds = pour_points
        elif isinstance(pour_points, np.ndarray):      # an array is a raster, never a list
            if pour_points.ndim != 2:
                raise ValueError(f"a seeds raster is 2-D, got {pour_points.ndim} dimensions")
            self._seeds = self._seeds_raster(pour_points)
        else:
            self._points = self._point_list(pour_points)

    @staticmethod
    def _seeds_raster(seeds):
        if not np.issubdtype(seeds.dtype, np.integer):
            raise ValueError(f"a seeds raster has an integer dtype, got {seeds.dtype}")
        if seeds.size and (int(seeds.min()) < 0 or int(seeds.max()) > 0xFFFFFFFF):
            raise ValueError("seed labels must fit uint32")
        return np.ascontiguousarray(seeds, dtype=np.uint32)

    @staticmethod
    def _point_list(points):
        out = []
        for k, p in enumerate(points):
            p = tuple(int(v) for v in p)
            if len(p) == 2:
                p += (k + 1,)
            if len(p) != 3:
                raise ValueError(f"pour point {k} is (row, col) or (row, col, label), got {p}")
            if not 0 < p[2] <= 0xFFFFFFFF:
                raise ValueError(f"pour point {k}: label {p[2]} is not in 1 ... 2^32 - 1 "
                                 "(0 means no pour point)")
            out.append(p)
        return out

    def _host_seeds(self, shape):
        """The uint32 seeds raster for codes of ``shape`` (None in the outlet modes)."""
        if self._points is not None:
            seeds = np.zeros(shape, np.uint32)
            for k, (row, col, label) in enumerate(self._points):
                if not (0 <= row < shape[0] and 0 <= col < shape[1]):
                    raise ValueError(f"pour point {k} at ({row}, {col}) is outside the "
                                     f"{shape[0]} x {shape[1]} raster")
                seeds[row, col] = label
            return seeds
        if self._seeds is not None and tuple(self._seeds.shape) != tuple(shape):
            raise ValueError(f"seeds are {tuple(self._seeds.shape)}, the codes {tuple(shape)}")
        return self._seeds

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        _check_raster("Watersheds", image_to_filter, np.uint8, "uint8 D8 codes")
        seeds = _Given(self._host_seeds(image_to_filter.shape)).host()
        out, self.outlets, self.stats = backend.watershed(image_to_filter, seeds,
                                                          self.labels == "compact")
        return out

    def apply_device(self, raster):
        _check_raster("Watersheds", raster, np.uint8, "uint8 D8 codes")
        with _Given(self._host_seeds(raster.shape)).device(raster.ctx) as seeds:
            out, self.outlets, self.stats = backend.watershed_dev(raster, seeds,
                                                                  self.labels == "compact")
        return out


class _FlowTrace(Filter):  # pylint: disable=too-few-public-methods
    """What ``FlowDistance`` and ``HeightAboveDrainage`` share: the operands of one
    ``hdem_flowtrace_u8`` call (streams, threshold, dem, cellsize), checked as far as they can
    be before the codes are known, and the call on host arrays or device rasters."""

    auto_device = True      # device form == host form for a uint8 code raster

    def _set_operands(self, streams, threshold, dem, cellsize):
        self.streams = _Given(streams, "streams", (np.bool_, np.uint8, np.uint32)).value
        self.dem = _Given(dem, "dem", (np.float32,)).value
        self.threshold, self.cellsize = threshold, cellsize
        self.stats = {}
        # everything but the shapes: 1 x 1 stand-ins for the codes and the operands
        backend.flowtrace_args(np.zeros((1, 1), np.uint8), _Given(self.streams).stand_in(),
                               threshold, _Given(self.dem).stand_in(), cellsize, ("distance",))

    def _check(self, codes, want):
        return backend.flowtrace_args(codes, self.streams, self.threshold, self.dem,
                                      self.cellsize, want)

    def _trace(self, image_to_filter, want):
        Filter.apply(self, image_to_filter)
        self._check(image_to_filter, want)
        outs, self.stats = backend.flowtrace(
            image_to_filter, _Given(self.streams).host(), self.threshold,
            _Given(self.dem).host(), self.cellsize, want)
        return outs

    def _trace_device(self, raster, want):
        self._check(raster, want)
        with _Given(self.streams).device(raster.ctx) as streams, \
                _Given(self.dem).device(raster.ctx) as dem:
            outs, self.stats = backend.flowtrace_dev(raster, streams, self.threshold, dem,
                                                     self.cellsize, want)
        return outs


class FlowDistance(_FlowTrace):  # pylint: disable=too-few-public-methods
    """Downstream D8 flow length (new operator).  Input: a uint8 H x W raster of ESRI D8 codes
    exactly as ``FlowAccumulation`` takes them.  Returns float32: the length of the cell's D8
    path down to the first *stop*, ``ncard * cellsize + ndiag * cellsize * sqrt(2)`` evaluated
    in float64 and rounded once, with ``ncard`` / ``ndiag`` the cardinal and diagonal steps.

    ``FlowDistance()``: a stop is a terminal cell (code 0 or pointing outside the raster):
    the distance to the outlet.  ``FlowDistance(streams)``: a stream cell is a stop too
    (distance to streams); ``streams`` is a bool / uint8 mask of the codes' shape (non-zero =
    stream), a uint32 raster with ``threshold`` (stream where ``>= threshold``: a
    ``FlowAccumulation`` result goes in as it is), or a ``DeviceRaster`` of uint8 or uint32.
    A cell whose path ends in a terminal cell that is no stream cell is unreached and reads
    NaN, and so does that terminal cell.

    ``ValueError`` for operands of another type, dtype or shape, ``threshold`` without a
    uint32 raster, with a mask, or < 1, a ``cellsize`` that is not finite and positive (all
    before the device is touched), a byte that is not a D8 code, codes that form a cycle (a
    loop that holds a stream cell is legal) and more than 2^32 - 1 cells.  Exact, identical
    from run to run.

    Attributes
    ----------
    stats : dict
        stops (stream and terminal cells), unreached (cells), exits, forest_rounds,
        tile_h / tile_w of the last call; phase times when profiling is on.
    """

    def __init__(self, streams=None, *, threshold=None, cellsize=1.0):
        self._set_operands(streams, threshold, None, cellsize)

    def apply(self, image_to_filter):
        return self._trace(image_to_filter, ("distance",))["distance"]

    def apply_device(self, raster):
        return self._trace_device(raster, ("distance",))["distance"]


class HeightAboveDrainage(_FlowTrace):  # pylint: disable=too-few-public-methods
    """Height above the nearest drainage, HAND (new operator).  Input: uint8 D8 codes as
    ``FlowDistance`` takes them.  Returns float32 ``dem[c] - dem[s(c)]``, one float32
    subtraction, ``s(c)`` the first stream cell on ``c``'s D8 path (``c`` included), and NaN
    where the path ends without meeting one.  NaN in ``dem`` propagates by arithmetic.

    ``dem``: float32 array or ``DeviceRaster`` of the codes' shape; ``streams``,
    ``threshold``, ``cellsize`` and the errors as for ``FlowDistance``.  With
    ``keep_partial_results=True`` the same call also leaves ``distance`` (the
    ``FlowDistance(streams)`` raster) and ``drainage`` (uint32: 1 + flat index of ``s(c)``, 0
    where unreached) -- host arrays after ``apply``, device rasters after ``apply_device``;
    otherwise both are ``None``.
    """

    def __init__(self, *, dem, streams, threshold=None, cellsize=1.0,
                 keep_partial_results=False):
        if dem is None:
            raise ValueError("HeightAboveDrainage needs the dem it is measured on")
        if streams is None:
            raise ValueError("HeightAboveDrainage needs streams (a mask, or a uint32 raster "
                             "with a threshold)")
        self._set_operands(streams, threshold, dem, cellsize)
        self.keep_partial_results = keep_partial_results
        self.distance = self.drainage = None

    def _keep(self, outs):
        self.distance, self.drainage = outs.get("distance"), outs.get("stop")
        return outs["hand"]

    def _want(self):
        return ("stop", "distance", "hand") if self.keep_partial_results else ("hand",)

    def apply(self, image_to_filter):
        return self._keep(self._trace(image_to_filter, self._want()))

    def apply_device(self, raster):
        return self._keep(self._trace_device(raster, self._want()))


class _FlowPath(Filter):  # pylint: disable=too-few-public-methods
    """What ``FlowPathSum`` and ``FlowPathExtreme`` share: the operands of one
    ``hdem_flowpath_u8`` call, with the streams and the threshold handled as ``_FlowTrace``
    handles them, checked as far as they can be before the codes are known, and the call on
    host arrays or device rasters.  ``stop`` is what ``keep_partial_results`` leaves."""

    auto_device = True      # device form == host form for a uint8 code raster
    VALUE_TYPES = ()

    def _set_operands(self, mode, values, streams, threshold, output, keep_partial_results):
        self.mode = mode
        self._values = _Given(values, "weights" if mode == "sum" else "values",
                              self.VALUE_TYPES).value
        self.streams = _Given(streams, "streams", (np.bool_, np.uint8, np.uint32)).value
        self.threshold, self.output = threshold, output
        self.keep_partial_results = keep_partial_results
        self.stop = None
        self.stats = {}

    def _table(self, height):
        """The step-length table for codes of ``height`` rows (``None``: not per length)."""
        raise NotImplementedError

    def _call_args(self, height, values, streams):
        per, frac_bits = getattr(self, "per", "step"), getattr(self, "frac_bits", 0)
        return dict(values=values, mode=self.mode, streams=streams, threshold=self.threshold,
                    per=per, step_len=self._table(height), frac_bits=frac_bits, want=self._want())

    def _want(self):
        return ("stop", self.output) if self.keep_partial_results else (self.output,)

    def _check(self, codes):
        height = codes.shape[0] if len(codes.shape) == 2 else 1
        a = self._call_args(height, self._values, self.streams)
        _flowpath.flowpath_args(codes, a["streams"], a["threshold"], a["mode"], a["values"],
                                a["per"], a["step_len"], a["frac_bits"], a["want"])

    def _keep(self, outs):
        self.stop = outs.get("stop")
        return outs[self.output]

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        self._check(image_to_filter)
        outs, self.stats = _flowpath.flowpath(
            image_to_filter, **self._call_args(image_to_filter.shape[0],
                                               _Given(self._values).host(),
                                               _Given(self.streams).host()))
        return self._keep(outs)

    def apply_device(self, raster):
        self._check(raster)
        with _Given(self._values).device(raster.ctx) as values, \
                _Given(self.streams).device(raster.ctx) as streams:
            outs, self.stats = _flowpath.flowpath_dev(
                raster, **self._call_args(raster.shape[0], values, streams))
        return self._keep(outs)


class FlowPathSum(_FlowPath):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """Downstream D8 path sum (new operator; ArcGIS *Flow Length (downstream)* with a weight
    raster, Whitebox ``DownslopeFlowpathLength --weights``, travel time, the downslope component
    of the sediment connectivity index).  Input: a uint8 H x W raster of ESRI D8 codes exactly
    as ``FlowDistance`` takes them, and ``streams`` / ``threshold`` mean what they mean there: a
    path runs from the cell to its first *stop*, a terminal cell or a stream cell.  Returns the
    sum, over the cells of the path but the stop, of the cost of the step that leaves the cell;
    a stop reads 0.

    Every cell's cost is quantised to an integer ``q`` in 0 ... 2^31 - 1 and summed in int64:
    exact, identical from run to run.  ``per="step"``: ``q`` is the weight itself for uint8 and
    uint32 ``weights``, which take ``frac_bits=0``, and ``rint(float64(w) * 2^frac_bits)`` for
    float32.  ``per="length"``: ``q = rint((float64(w) * len) * 2^frac_bits)``, ``len`` the
    length of the leaving step from ``step_lengths``, an array of ``(rows, 3)`` float64
    ``(east-west, north-south, diagonal)`` (``hydrodem_amd.flowpath.step_lengths`` for square
    cells, ``geographic_step_lengths`` for a latitude / longitude grid); without one the table
    of square cells of ``cellsize`` is used.  ``weights=None`` per length counts ``w = 1``: the
    flow length on an anisotropic grid.  ``weights``: an H x W NumPy array or ``DeviceRaster``
    of uint8, uint32 or float32 (float64 is refused, not narrowed).

    ``output`` fixes what ``apply`` returns: ``"value"`` float32
    ``float32(float64(S) * 2^-frac_bits)``, NaN where the path ends in a terminal cell that is
    no stream cell, or ``"sum"`` int64 ``S`` (for an unreached cell the sum to that terminal
    cell).  With ``keep_partial_results=True`` the call also leaves ``stop`` (uint32: 1 + flat
    index of the stop, 0 where unreached), a host array after ``apply`` and a device raster
    after ``apply_device``.

    A NaN weight costs 0 (``stats["nan_weights"]`` counts them).  ``ValueError`` for operands of
    another type, dtype or shape, a bad ``per``, ``frac_bits``, ``cellsize`` or table (all
    before the device is touched), for a negative or infinite weight, a quantised cost above
    2^31 - 1, a byte that is not a D8 code, codes that form a cycle and more than 2^32 - 1
    cells.

    Attributes
    ----------
    stats : dict
        nan_weights, stops, unreached, exits, forest_rounds, tile_h / tile_w of the last call;
        phase times when profiling is on.
    stop : numpy.ndarray, DeviceRaster or None
    """

    VALUE_TYPES = (np.uint8, np.uint32, np.float32)
    OUTPUTS = {"value": np.dtype(np.float32), "sum": np.dtype(np.int64)}

    def __init__(self, weights=None, *, per="step", step_lengths=None, cellsize=1.0,
                 frac_bits=16, streams=None, threshold=None, output="value",
                 keep_partial_results=False):
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self._set_operands("sum", weights, streams, threshold, output, keep_partial_results)
        self.weights = self._values
        self.per, self.frac_bits = per, frac_bits
        self.step_lengths = step_lengths
        self.cellsize = backend._cellsize(cellsize)  # pylint: disable=protected-access
        self.dtype = self.OUTPUTS[output]
        if step_lengths is not None and per == "length":
            self.step_lengths = _flowpath.table_of(step_lengths)
        # everything but the shapes, on 1 x 1 stand-ins
        _flowpath.flowpath_args(
            np.zeros((1, 1), np.uint8), _Given(self.streams).stand_in(), threshold, "sum",
            _Given(self._values).stand_in(), per,
            _flowpath.step_lengths(1, self.cellsize) if per == "length" else step_lengths,
            frac_bits, self._want())

    def _table(self, height):
        if self.per != "length" or self.step_lengths is not None:
            return self.step_lengths
        return _flowpath.step_lengths(height, self.cellsize)


class FlowPathExtreme(_FlowPath):  # pylint: disable=too-few-public-methods
    """Downstream D8 path minimum or maximum (new operator; the twin of ``UpstreamExtreme``
    along a cell's own path).  Input: a uint8 H x W raster of ESRI D8 codes exactly as
    ``FlowDistance`` takes them, with its ``streams`` / ``threshold``.  ``values``: an H x W
    NumPy array or ``DeviceRaster`` of float32 or uint32.  For every cell, over the cells of
    its D8 path down to its first stop, the cell and the stop included, the least
    (``mode="min"``) or greatest (``mode="max"``) present value.  A float32 NaN is absent
    (``stats["absent"]`` counts them); floats are ordered
    ``-inf < ... < -0.0 < +0.0 < ... < +inf``.

    ``output`` fixes what ``apply`` returns: ``"extreme"``, of the values' dtype, the bits of
    the cell that holds the extreme (the quiet NaN where nothing on the path is present), or
    ``"where"``, uint32, that cell's flat index (``0xFFFFFFFF`` where nothing is present).
    Among cells that hold the same value the smallest flat index is the holder, in both modes.
    Where the path ends in a terminal cell that is no stream cell the path to that cell is
    reduced; ``keep_partial_results=True`` leaves ``stop`` (uint32, 0 there) to tell.

    ``ValueError`` for operands of another type, dtype or shape, an unknown ``mode`` or
    ``output`` (all before the device is touched), a byte that is not a D8 code, codes that form
    a cycle and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        absent, stops, unreached, exits, forest_rounds, tile_h / tile_w of the last call; phase
        times when profiling is on.
    stop : numpy.ndarray, DeviceRaster or None
    """

    VALUE_TYPES = (np.float32, np.uint32)
    OUTPUTS = ("extreme", "where")

    def __init__(self, values, mode="min", *, streams=None, threshold=None, output="extreme",
                 keep_partial_results=False):
        if values is None:
            raise ValueError("FlowPathExtreme needs the values it reduces")
        if not isinstance(mode, str) or mode not in ("min", "max"):
            raise ValueError(f"mode is one of ['min', 'max'], got {mode!r}")
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self._set_operands(mode, values, streams, threshold, output, keep_partial_results)
        self.values = self._values
        self.dtype = np.dtype(np.uint32) if output == "where" else np.dtype(self.values.dtype)
        # everything but the shapes, on 1 x 1 stand-ins
        _flowpath.flowpath_args(np.zeros((1, 1), np.uint8), _Given(self.streams).stand_in(),
                                threshold, mode, _Given(self._values).stand_in(), "step", None, 0,
                                self._want())

    def _table(self, height):
        return None


class UpstreamFlowLength(Filter):  # pylint: disable=too-few-public-methods
    """Longest upstream D8 flow length (new operator).  Input: a uint8 H x W raster of ESRI D8
    codes exactly as ``FlowAccumulation`` takes them.  Returns float32: the length of the
    longest D8 path that ends in the cell, ``ncard * cellsize + ndiag * cellsize * sqrt(2)``
    evaluated in float64 and rounded once (``FlowDistance``'s formula), 0 for a cell nothing
    drains into.  ``(ncard, ndiag)``, the cardinal and diagonal steps of that path, solve
    ``up(c) = max(up(d) + step(d))`` over the neighbours ``d`` whose code points at ``c``,
    where pairs are ordered by ``ncard + ndiag * sqrt(2)`` decided exactly, in integers: two
    different pairs never tie, and no rounded length is ever compared.

    With ``keep_partial_results=True`` the same call also leaves ``ncard`` and ``ndiag``
    (uint32) -- host arrays after ``apply``, device rasters (the caller's to free) after
    ``apply_device``; otherwise both are ``None``.

    ``ValueError`` for a dtype other than uint8, a raster that is not 2-D, a ``cellsize`` that
    is not finite and positive (all before the device is touched), a byte that is not a D8
    code, codes that form a cycle and more than 2^32 - 1 cells.  Exact, identical from run to
    run.

    Attributes
    ----------
    stats : dict
        heads (cells without a donor), exits (nodes of the exit forest), max_hops (tile
        crossings of the longest forest walk), tile_h / tile_w of the last call; phase times
        when profiling is on.
    """

    auto_device = True      # device form == host form for a uint8 code raster

    def __init__(self, *, cellsize=1.0, keep_partial_results=False):
        self.cellsize = backend._cellsize(cellsize)  # pylint: disable=protected-access
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.ncard = self.ndiag = None

    def _want(self):
        return ("ncard", "ndiag", "length") if self.keep_partial_results else ("length",)

    def _keep(self, outs):
        self.ncard, self.ndiag = outs.get("ncard"), outs.get("ndiag")
        return outs["length"]

    def apply(self, image_to_filter):
        super().apply(image_to_filter)
        outs, self.stats = _upstream.upstream(image_to_filter, self.cellsize, self._want())
        return self._keep(outs)

    def apply_device(self, raster):
        outs, self.stats = _upstream.upstream_dev(raster, self.cellsize, self._want())
        return self._keep(outs)


class StreamOrder(_FlowTrace):  # pylint: disable=too-few-public-methods
    """Strahler stream order, Shreve magnitude and stream links (new operator).  Input: a uint8
    H x W raster of ESRI D8 codes exactly as ``FlowAccumulation`` takes them.  ``streams`` is
    the stream set as ``FlowDistance`` takes it: ``None`` (every cell is a stream cell), a
    bool / uint8 mask of the codes' shape (non-zero = stream), a uint32 raster with
    ``threshold`` (stream where ``>= threshold``: a ``FlowAccumulation`` result goes in as it
    is), or a ``DeviceRaster`` of uint8 or uint32.

    A stream donor of a cell is a neighbouring stream cell whose code points at it.  Off the
    streams every result is 0.  On them, ``method="strahler"`` returns the uint8 order: 1
    without a stream donor; else, with ``m`` the greatest order among the stream donors,
    ``m + 1`` when two or more of them have it and ``m`` otherwise (the TauDEM / Whitebox rule
    where more than two branches meet).  ``method="shreve"`` returns the uint32 magnitude: 1
    without a stream donor, else the sum over the stream donors: the number of heads upstream.

    With ``keep_partial_results=True`` the same call leaves ``order``, ``magnitude`` and
    ``links`` (uint32: 1 + flat index of the last cell of the cell's link, the segment between
    two junctions; ``Watersheds(pour_points=...)`` takes these ids and gives one catchment per
    link) -- host arrays after ``apply``, device rasters (the caller's to free; the one
    returned is among them) after ``apply_device``; otherwise they are ``None``.

    ``ValueError`` for operands of another type, dtype or shape, ``threshold`` without a
    uint32 raster, with a mask, or < 1, an unknown ``method`` (all before the device is
    touched), a byte that is not a D8 code, codes that form a cycle, on or off the streams,
    and more than 2^32 - 1 cells.  Exact, identical from run to run.

    Attributes
    ----------
    stats : dict
        stream_cells, heads (stream cells without a stream donor), junctions (two or more),
        links, max_order, max_hops (links of the longest walk over the link graph),
        tile_h / tile_w of the last call; phase times when profiling is on.
    """

    METHODS = {"strahler": "order", "shreve": "magnitude"}

    def __init__(self, streams=None, *, threshold=None, method="strahler",
                 keep_partial_results=False):
        if method not in self.METHODS:
            raise ValueError(f"method is 'strahler' or 'shreve', got {method!r}")
        self._set_operands(streams, threshold, None, 1.0)
        self.method = method
        self.keep_partial_results = keep_partial_results
        self.order = self.magnitude = self.links = None

    def _want(self):
        if self.method not in self.METHODS:
            raise ValueError(f"method is 'strahler' or 'shreve', got {self.method!r}")
        return ("order", "magnitude", "link") if self.keep_partial_results \
            else (self.METHODS[self.method],)

    def _keep(self, outs):
        self.order = self.magnitude = self.links = None
        if self.keep_partial_results:
            self.order, self.magnitude, self.links = outs["order"], outs["magnitude"], outs["link"]
        return outs[self.METHODS[self.method]]

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        want = self._want()
        outs, self.stats = _streamorder.streamorder(
            image_to_filter, _Given(self.streams).host(), self.threshold, want)
        return self._keep(outs)

    def apply_device(self, raster):
        want = self._want()
        _streamorder.streamorder_args(raster, self.streams, self.threshold, want)
        with _Given(self.streams).device(raster.ctx) as streams:
            outs, self.stats = _streamorder.streamorder_dev(raster, streams, self.threshold, want)
        return self._keep(outs)


class StreamNetwork(_FlowTrace):  # pylint: disable=too-few-public-methods
    """The stream network as a table, one row per link (new operator).  Input: a uint8 H x W
    raster of ESRI D8 codes; ``streams`` and ``threshold`` are the stream set as ``StreamOrder``
    takes it.  Runs ``StreamOrder`` and then gathers the links (the segments between two
    junctions) into ``table``, a dict of host arrays with one entry per link, numbered in
    ascending flat index of the link's last cell: ``end`` and ``top`` (flat indices of the last
    and first cell), ``down`` (the row of the link it drains into, ``0xFFFFFFFF`` for none),
    ``order``, ``magnitude``, ``cells``, ``ncard`` / ``ndiag`` (cardinal and diagonal steps from
    ``top`` to ``end``, plus the step out of ``end`` when ``down`` is a link, so that lengths
    add up along ``down``), ``length`` (``ncard * cellsize + ndiag * cellsize * sqrt(2)`` in
    float64, rounded once), ``catchment`` (cells, on or off the streams, whose first stream
    cell lies in the link) and, with a float32 ``dem``, ``z_top`` / ``z_end``.  ``columns``
    picks among them (default: all that the operands allow); without ``catchment`` no flow
    trace runs.

    Returns the ``row`` raster (uint32: 1 + row on the cells of a link, 0 off the streams; pour
    points for ``Watersheds`` whose labels index the table): a host array from ``apply``, a
    device raster (the caller's to free) from ``apply_device``.  ``count`` is the number of
    links.  With ``keep_partial_results=True`` the call also leaves ``order``, ``magnitude``
    and ``links`` as ``StreamOrder`` does.

    ``ValueError`` for everything ``StreamOrder`` refuses, an unknown column and ``z_top`` /
    ``z_end`` without ``dem`` (all before the device is touched).  Exact, identical from run
    to run.

    Attributes
    ----------
    stats : dict
        links, stream_cells, catchment_cells (cells that reach a stream), tops, tile_h / tile_w
        of the last call, phase times when profiling is on, and ``order_stats``, the stats of
        the stream order.
    """

    KEPT = ("order", "magnitude", "links")

    def __init__(self, streams=None, *, threshold=None, dem=None, cellsize=1.0, columns=None,
                 keep_partial_results=False):
        self._set_operands(streams, threshold, dem, cellsize)
        self.columns = columns
        self.keep_partial_results = keep_partial_results
        self.table, self.count = None, 0
        self.order = self.magnitude = self.links = None
        # everything but the shapes: 1 x 1 stand-ins for the rasters of the two calls
        one = np.zeros((1, 1), np.uint8)
        self._check_table(one, np.zeros((1, 1), np.uint32), one, np.zeros((1, 1), np.uint32),
                          _Given(self.streams).stand_in(), _Given(self.dem).stand_in())

    def _check_table(self, codes, link, order, magnitude, streams, dem):
        return _streamnet.streamnet_args(codes, streams, self.threshold, link, order, magnitude,
                                         dem, self.cellsize, 0, self.columns, True)

    def _check_codes(self, codes):
        """The checks of both calls before either runs: the order's, then the table's on
        stand-ins of the shape the order's rasters will have."""
        _streamorder.streamorder_args(codes, self.streams, self.threshold, "link")
        like = lambda dtype: np.broadcast_to(np.zeros((), dtype), codes.shape)  # noqa: E731
        self._check_table(codes, like(np.uint32), like(np.uint8), like(np.uint32), self.streams,
                          self.dem)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._check_codes(image_to_filter)
        with contextlib.ExitStack() as stack:
            codes = stack.enter_context(backend.DeviceRaster.from_host(image_to_filter))
            row = stack.enter_context(self.apply_device(codes))
            for name in self.KEPT if self.keep_partial_results else ():
                raster = stack.enter_context(getattr(self, name))
                setattr(self, name, raster.to_host())
            return row.to_host()

    def apply_device(self, raster):
        self._check_codes(raster)
        self.order = self.magnitude = self.links = None
        with _Given(self.streams).device(raster.ctx) as streams, \
                _Given(self.dem).device(raster.ctx) as dem, contextlib.ExitStack() as stack:
            outs, order_stats = _streamorder.streamorder_dev(
                raster, streams, self.threshold, ("order", "magnitude", "link"))
            for out in outs.values():
                stack.enter_context(out)
            self.count = order_stats["links"]
            self.table, row, stats = _streamnet.streamlinks_dev(
                raster, outs["link"], self.count, streams, self.threshold, outs["order"],
                outs["magnitude"], dem, self.cellsize, self.columns, want_row=True)
            self.stats = dict(stats, order_stats=order_stats)
            if self.keep_partial_results:
                self.order, self.magnitude, self.links = (outs["order"], outs["magnitude"],
                                                          outs["link"])
                stack.pop_all()                     # the caller's to free from here on
        return row


class ZonalStatistics(Filter):  # pylint: disable=too-few-public-methods
    """Zonal statistics as a table (new operator).  Input: a uint32 H x W raster of zone ids, 0
    where a cell belongs to no zone -- the labels of ``Watersheds``, the ``row`` raster of
    ``StreamNetwork``, the labels of ``Depressions`` -- and, at construction, optionally a
    raster of ``values`` of the same shape (float32, uint32 or uint8; array or
    ``DeviceRaster``).  Ids lie in 1 ... H * W, which every label raster of this library
    satisfies; arbitrary pour-point labels are relabelled first (``np.unique`` with
    ``return_inverse``).

    Returns the table, a dict of host arrays with one entry per zone present, in ascending id
    (the order of ``np.unique``): ``id``, ``count``, ``first`` (smallest flat index),
    ``row_min`` / ``row_max`` / ``col_min`` / ``col_max`` (the bounding box, inclusive) and,
    with values, ``valid`` (cells that are not NaN), ``min`` / ``max`` (in the values' type;
    -0.0 sorts below +0.0 and infinities take part; NaN, or 0 for the integer types, where
    ``valid`` is 0), ``at_min`` / ``at_max`` (flat index of a cell holding them, the smallest on
    ties, ``0xFFFFFFFF`` where ``valid`` is 0) and ``sum``: the exact uint64 sum of integer
    values; for float32 the int64 sum of ``q(v) = clamp(rint(v * 2**frac_bits), +-(2**31 - 1))``
    (``frac_bits`` in 0 ... 30; the default 16 holds ``|v| < 32768`` at a resolution of
    1.5e-5; cells that clamp are counted in ``stats["clamped"]``).  ``mean`` is not computed on
    the device: it is derived here in float64 as ``sum / 2**frac_bits / valid`` (integer
    values: ``sum / valid``), NaN where ``valid`` is 0, when both columns are there.
    ``columns`` picks among the device columns (default: all that the operands allow).  Exact,
    identical from run to run and from ``apply`` and ``apply_device``.

    ``broadcast(column, fill=0)`` is the raster form: every cell gets its zone's entry of a
    column of the last table (by name, or an array of K 4-byte entries), ``fill`` where the id
    is 0 -- a host array after ``apply``, a device raster (the caller's to free) after
    ``apply_device``.

    ``ValueError`` for zones that are not a 2-D uint32 raster, values of another shape or dtype,
    unknown columns, a value column without values, ``frac_bits`` out of range (all before the
    device is touched) and an id above H * W (the message names how many cells and the largest
    id).

    Attributes
    ----------
    stats : dict
        zones (K), unzoned (cells with id 0), clamped, overflow (cells that went past their
        tile's table), over_range, capped, max_id, tile_h / tile_w of the last call; phase times
        when profiling is on.
    table : dict of numpy.ndarray, or None
        the table of the last call.
    """

    auto_device = True      # device form == host form for a uint32 raster

    def __init__(self, values=None, columns=None, frac_bits=16):
        self.values = _Given(values, "values", tuple(_zonal.VALUE_TYPES)).value
        self.columns, self.frac_bits = columns, frac_bits
        self.stats, self.table = {}, None
        self._zones = None
        # everything but the shapes, on 1 x 1 stand-ins
        _zonal.zonal_args(np.zeros((1, 1), np.uint32), _Given(self.values).stand_in(),
                          columns, frac_bits)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _zonal.zonal_args(image_to_filter, self.values, self.columns, self.frac_bits)
        self.table, self.stats = _zonal.zonal(image_to_filter, _Given(self.values).host(),
                                              self.columns, self.frac_bits)
        self._zones = image_to_filter
        return self.table

    def apply_device(self, raster):
        _zonal.zonal_args(raster, self.values, self.columns, self.frac_bits)
        with _Given(self.values).device(raster.ctx) as values:
            self.table, self.stats = _zonal.zonal_dev(raster, values, self.columns,
                                                      self.frac_bits)
        self._zones = raster
        return self.table

    def broadcast(self, column, fill=0):
        """The raster whose cells hold their zone's entry of ``column`` (see the class)."""
        if self._zones is None:
            raise ValueError("broadcast follows apply or apply_device: there is no table yet")
        if isinstance(column, str):
            if column not in self.table:
                raise ValueError(f"the last table has no column {column!r}: it has "
                                 f"{list(self.table)}")
            column = self.table[column]
        column = np.asarray(column)
        if column.shape != (self.stats["zones"],):
            raise ValueError(f"a column has one entry per zone ({self.stats['zones']}), got "
                             f"shape {column.shape}")
        if backend.is_device_raster(self._zones):
            return _zonal.zonal_broadcast_dev(self._zones, column, fill)
        with backend.DeviceRaster.from_host(self._zones) as zones, \
                _zonal.zonal_broadcast_dev(zones, column, fill) as out:
            return out.to_host()


class TerrainAttributes(Filter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """Slope, aspect and what is built on them, from one read of the DEM (new operator).
    Input: a float32 H x W DEM, NaN where there is no data.  ``want`` names outputs of
    ``hydrodem_amd.terrain.TERRAIN_OUTPUTS``, all float32:

    ``dzdx`` / ``dzdy``  Horn's gradient over the 3 x 3 window (x eastwards, y southwards),
                         differences first, times ``z_factor / (8 dx)`` and ``z_factor / (8 dy)``;
                         a neighbour outside the raster or NaN takes the centre's value (ArcGIS)
    ``tangent``          ``sqrt(dzdx^2 + dzdy^2)``: the percent slope / 100
    ``degrees``          ``atan(tangent)`` in degrees
    ``aspect``           compass direction of the steepest descent in degrees clockwise from
                         north, in [0, 360); -1 where the gradient is 0
    ``d8_slope``         drop to the cell the D8 code points at over the length of that step,
                         0 for code 0 and for a code pointing outside; needs ``codes``
    ``twi``              ``ln(a / max(t, min_slope))`` with ``a = accumulation * sqrt(dx dy)``,
                         the specific catchment area; needs ``accumulation``
    ``spi``              ``a * t``; needs ``accumulation``

    ``t`` is the tangent (``slope="horn"``) or the D8 slope (``slope="d8"``, TauDEM's choice).
    A NaN cell is NaN in every output.  ``cellsize``: a number or ``(dy, dx)``.  ``codes`` (uint8
    ESRI D8 codes) and ``accumulation`` (uint32, ``FlowAccumulation``'s raster) are given at
    construction, as arrays or device rasters of the DEM's shape.

    Returns the first output of ``want``.  With ``keep_partial_results=True`` the same launch
    also writes the other outputs of ``want`` and leaves them in the attributes of their names
    -- host arrays after ``apply``, device rasters (the caller's to free) after
    ``apply_device``; otherwise only the first is computed and the attributes are ``None``.

    ``ValueError`` for a dtype other than float32, a raster that is not 2-D, operands of
    another shape or dtype, unknown outputs, an output without the operand it needs, a
    ``cellsize``, ``z_factor`` or ``min_slope`` that is not finite and positive (all before the
    device is touched) and a ``codes`` byte that is no D8 code.

    Attributes
    ----------
    stats : dict
        nan_cells, flat_cells (aspect -1), floored_cells (cells whose slope was below
        ``min_slope``, counted when ``twi`` is computed), invalid_codes of the last call;
        ms_total when profiling is on.
    """

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, want=("degrees",), cellsize=1.0, z_factor=1.0, codes=None,
                 accumulation=None, min_slope=1e-3, slope="horn", keep_partial_results=False):
        self.want = (want,) if isinstance(want, str) else tuple(want)
        self.cellsize, self.z_factor = cellsize, z_factor
        self.codes = _Given(codes, "codes", (np.uint8,)).value
        self.accumulation = _Given(accumulation, "accumulation", (np.uint32,)).value
        self.min_slope, self.slope = min_slope, slope
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        for name in _terrain.TERRAIN_OUTPUTS:
            setattr(self, name, None)
        # everything but the shapes, on 1 x 1 stand-ins
        self._args(np.zeros((1, 1), np.float32), _Given(self.codes).stand_in(),
                   _Given(self.accumulation).stand_in())

    def _args(self, dem, codes, accumulation):
        return _terrain.terrain_args(dem, self.want, self.cellsize, self.z_factor, codes,
                                     accumulation, self.min_slope, self.slope)

    def _want(self):
        return self.want if self.keep_partial_results else self.want[:1]

    def _keep(self, outs):
        for name in _terrain.TERRAIN_OUTPUTS:
            setattr(self, name, outs.get(name) if name != self.want[0] else None)
        return outs[self.want[0]]

    def _run(self, run, dem, codes, accumulation):
        outs, self.stats = run(dem, self._want(), self.cellsize, self.z_factor, codes,
                               accumulation, self.min_slope, self.slope)
        return self._keep(outs)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._args(image_to_filter, self.codes, self.accumulation)
        return self._run(_terrain.terrain, image_to_filter, _Given(self.codes).host(),
                         _Given(self.accumulation).host())

    def apply_device(self, raster):
        self._args(raster, self.codes, self.accumulation)
        with _Given(self.codes).device(raster.ctx) as codes, \
                _Given(self.accumulation).device(raster.ctx) as accumulation:
            return self._run(_terrain.terrain_dev, raster, codes, accumulation)


class Slope(TerrainAttributes):  # pylint: disable=too-few-public-methods
    """Horn's slope of a float32 DEM (``TerrainAttributes``): ``units`` is ``"degrees"``,
    ``"percent"`` (the tangent times 100, by the element-wise device operator) or
    ``"tangent"``."""

    UNITS = ("degrees", "percent", "tangent")

    def __init__(self, units="degrees", cellsize=1.0, z_factor=1.0):
        if units not in self.UNITS:
            raise ValueError(f"units is 'degrees', 'percent' or 'tangent', got {units!r}")
        super().__init__(want=("degrees" if units == "degrees" else "tangent",),
                         cellsize=cellsize, z_factor=z_factor)
        self.units = units

    def apply(self, image_to_filter):
        if self.units != "percent":
            return super().apply(image_to_filter)
        Filter.apply(self, image_to_filter)
        self._args(image_to_filter, None, None)
        return _through_device(self, image_to_filter)

    def apply_device(self, raster):
        first = super().apply_device(raster)
        if self.units != "percent":
            return first
        with first:
            return backend.elementwise_dev(backend.EW_MUL, first, 100.0)


class Aspect(TerrainAttributes):  # pylint: disable=too-few-public-methods
    """The aspect of a float32 DEM (``TerrainAttributes``): degrees clockwise from north of the
    steepest descent of Horn's gradient, -1 where the gradient is 0."""

    def __init__(self, cellsize=1.0, z_factor=1.0):
        super().__init__(want=("aspect",), cellsize=cellsize, z_factor=z_factor)


class WetnessIndex(TerrainAttributes):  # pylint: disable=too-few-public-methods
    """The topographic wetness index ``ln(a / max(tan b, min_slope))`` of a float32 DEM and its
    uint32 ``accumulation`` raster (``TerrainAttributes``): ``a`` is the accumulation times
    ``sqrt(dx dy)``, ``tan b`` Horn's tangent, or the D8 slope along ``codes`` with
    ``slope="d8"``."""

    def __init__(self, accumulation=None, codes=None, cellsize=1.0, z_factor=1.0,
                 min_slope=1e-3, slope="horn"):
        super().__init__(want=("twi",), cellsize=cellsize, z_factor=z_factor, codes=codes,
                         accumulation=accumulation, min_slope=min_slope, slope=slope)


class _Proximity(Filter):  # pylint: disable=too-few-public-methods
    """What ``EuclideanDistance``, ``EuclideanAllocation`` and ``BurnStreams`` share: the
    operands of one ``hdem_proximity`` call, checked as far as they can be before the shapes
    are known, and the call on host arrays or device rasters.

    The nearest source of a cell minimises ``(r - r')^2 + (x - x')^2``, in integers; among
    sources at equal distance it is the one with the smallest flat index ``r' * W + x'``.
    Exact, identical from run to run.  ``ValueError`` (before the device is touched) for
    operands of another type, dtype or shape, a ``threshold`` that does not go with the
    sources, more than 2^32 - 1 cells, a squared diagonal of more than 2^32 - 2 and a side of
    more than 65535 cells.

    Attributes
    ----------
    stats : dict
        sources (cells of the source set), unreached (cells out of reach) of the last call;
        ms_row, ms_column and ms_final when profiling is on.
    """

    SOURCE_TYPES = (np.bool_, np.uint8, np.uint32)

    def _set_operands(self, sources, threshold, cellsize=1.0, max_distance=None, buffer=None,
                      smooth=0.0, sharp=0.0):
        self.sources = _Given(sources, "sources", self.SOURCE_TYPES).value
        self.threshold, self.cellsize, self.max_distance = threshold, cellsize, max_distance
        self.buffer, self.smooth, self.sharp = buffer, smooth, sharp
        self.stats = {}

    def _args(self, sources, want, dem=None):
        return _proximity.proximity_args(sources, self.threshold, want, dem, self.cellsize,
                                         self.max_distance, self.buffer, self.smooth, self.sharp)

    def _call(self, run, sources, want, dem=None):
        outs, self.stats = run(sources, self.threshold, want, dem, self.cellsize,
                               self.max_distance, self.buffer, self.smooth, self.sharp)
        return outs


class _FromSources(_Proximity):  # pylint: disable=too-few-public-methods
    """The proximity filters whose input is the source raster itself, unless ``sources`` were
    given at construction: then the raster they are applied to only has to have their shape."""

    auto_device = False     # the input is a mask, an accumulation or labels, not a float32 DEM

    def __init__(self, sources=None, *, threshold=None, cellsize=1.0, max_distance=None):
        self._set_operands(sources, threshold, cellsize, max_distance)
        # everything but the shapes, on a 1 x 1 stand-in
        if self.sources is not None:
            self._args(_Given(self.sources).stand_in(), self._first(self.sources))

    def _first(self, sources):
        raise NotImplementedError

    def _given(self, raster):
        if self.sources is None:
            return raster
        backend._check(raster, None, "the raster is",  # pylint: disable=protected-access
                       like=("the sources", tuple(self.sources.shape)))
        return self.sources

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        sources = _Given(self._given(image_to_filter)).host()     # (a bool mask as bytes)
        want = self._first(sources)
        self._args(sources, want)
        return self._call(_proximity.proximity, sources, want)[want]

    def apply_device(self, raster):
        sources = self._given(raster)
        want = self._first(sources)
        self._args(sources, want)
        with _Given(sources).device(raster.ctx) as on_device:
            return self._call(_proximity.proximity_dev, on_device, want)[want]


class EuclideanDistance(_FromSources):  # pylint: disable=too-few-public-methods
    """Euclidean distance to the nearest source (new operator; ArcGIS *Euclidean Distance*).
    Input: the source raster -- a bool / uint8 mask (non-zero = source), a uint32 raster with
    ``threshold`` (source where ``>= threshold``: a ``FlowAccumulation`` result goes in as it
    is) or a uint32 label raster without one (non-zero = source) -- or, with ``sources`` given
    at construction, any raster of their shape.  Returns float32
    ``sqrt(d2) * cellsize``, evaluated in float64 and rounded once, ``d2`` the exact squared
    distance in cells; NaN beyond ``max_distance`` cells and where there is no source at all.
    Tie rule, errors and ``stats``: ``_Proximity``."""

    def _first(self, sources):
        return "distance"


class EuclideanAllocation(_FromSources):  # pylint: disable=too-few-public-methods
    """The nearest source of every cell (new operator; ArcGIS *Euclidean Allocation*).  Input
    as ``EuclideanDistance`` takes it.  Returns uint32: for a uint32 label raster (no
    ``threshold``) the label of the nearest source, 0 out of reach; for a mask or an
    accumulation with ``threshold`` the flat index of the nearest source, 0xFFFFFFFF out of
    reach.  Among sources at equal distance the one with the smallest flat index wins."""

    def _first(self, sources):
        labels = np.dtype(sources.dtype) == np.uint32 and self.threshold is None
        return "label" if labels else "nearest"


class BurnStreams(_Proximity):  # pylint: disable=too-few-public-methods
    """Stream burning of the AGREE kind (new operator): a float32 DEM in, the DEM lowered
    towards a known stream raster out, to be filled afterwards.  ``streams`` (a mask, a uint32
    raster with ``threshold``, or uint32 labels; array or ``DeviceRaster`` of the DEM's shape)
    is given at construction.  With ``d`` the float32 Euclidean distance in cells to the
    nearest stream cell, in float32, one rounding per operation:
    ``burned = dem - smooth * (1 - d / buffer) - (sharp on a stream cell)`` where
    ``d < buffer``, the DEM elsewhere (``1 / buffer`` is rounded to float32 once and
    multiplied); NaN stays NaN.  ``buffer > 0`` in cells, ``smooth >= 0`` and ``sharp >= 0`` in
    the DEM's units.  ``ComposedFilter`` chains ``BurnStreams``, ``SinkFill`` and
    ``D8FlowDirection`` on the device.  Tie rule, errors and ``stats``: ``_Proximity``."""

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, streams, *, threshold=None, buffer, smooth=0.0, sharp=0.0):
        if streams is None:
            raise ValueError("BurnStreams needs the streams it burns in (a mask, a uint32 raster "
                             "with a threshold, or labels)")
        self._set_operands(streams, threshold, buffer=buffer, smooth=smooth, sharp=sharp)
        self._args(_Given(self.sources).stand_in(), "burned", np.zeros((1, 1), np.float32))

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("BurnStreams", image_to_filter, np.float32, "a float32 DEM")
        self._args(self.sources, "burned", image_to_filter)
        return self._call(_proximity.proximity, _Given(self.sources).host(), "burned",
                          image_to_filter)["burned"]

    def apply_device(self, raster):
        _check_raster("BurnStreams", raster, np.float32, "a float32 DEM")
        self._args(self.sources, "burned", raster)
        with _Given(self.sources).device(raster.ctx) as streams:
            return self._call(_proximity.proximity_dev, streams, "burned", raster)["burned"]


class _CostFromSources(Filter):  # pylint: disable=too-few-public-methods
    """What ``CostDistance`` and ``CostAllocation`` share: the operands of one
    ``hdem_costdistance_f32`` call, checked as far as they can be before the shapes are known,
    and the call on host arrays or device rasters.  Input: the float32 cost raster, the price per
    cell length of crossing a cell; NaN is a barrier.  ``sources``: a bool / uint8 mask, a uint32
    raster with ``threshold`` (source where ``>= threshold``) or a uint32 label raster without
    one; array or ``DeviceRaster`` of the cost's shape.

    Every cost is quantised once, ``q = rint(float64(cost) * 2^frac_bits)``, ``frac_bits``
    0 ... 16, and must come to 1 ... 2^28 - 1.  A step between 8-neighbours ``a`` and ``b`` weighs
    ``s = q(a) + q(b)`` units of ``cellsize * 2^-(frac_bits+1)``, a diagonal one
    ``(s * 3037000500 + 2^30) >> 31``; cutting the corner of a barrier is legal.  The distance
    ``D`` of a cell is the least sum over all paths to a source: integers, identical from run to
    run and between ``apply`` and ``apply_device``.  Out of reach are barriers, cells with no
    path, and cells beyond ``max_distance`` (in the units of the distance output).

    ``ValueError`` (before the device is touched) for operands of another type, dtype or shape,
    a ``threshold`` that does not go with the sources, ``frac_bits``, ``cellsize`` or
    ``max_distance`` out of range and more than 2^32 - 1 cells; from the call for a negative or
    infinite cost and one that quantises to 0 or to more than 2^28 - 1, with their count.

    Attributes
    ----------
    stats : dict
        sources (that are no barrier), barriers, unreached, tie_cells, invalid, max_units,
        rounds and tile_visits (these two depend on the schedule), tile_h / tile_w of the last
        call; ms_classify, ms_relax, ms_final and ms_trace when profiling is on.
    """

    auto_device = True      # device form == host form for a float32 raster
    SOURCE_TYPES = (np.bool_, np.uint8, np.uint32)
    OUTPUTS = ()

    def __init__(self, sources, *, threshold=None, output=None, cellsize=1.0, frac_bits=16,
                 max_distance=None):
        name = type(self).__name__
        if sources is None:
            raise ValueError(f"{name} needs the sources it measures from (a mask, a uint32 "
                             "raster with a threshold, or labels)")
        self.sources = _Given(sources, "sources", self.SOURCE_TYPES).value
        if output is None:
            output = self._default_output(threshold)
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self.threshold, self.output, self.cellsize = threshold, output, cellsize
        self.frac_bits, self.max_distance = frac_bits, max_distance
        self.stats = {}
        # everything but the shapes, on 1 x 1 stand-ins
        self._args(np.zeros((1, 1), np.float32), _Given(self.sources).stand_in())

    def _default_output(self, threshold):
        raise NotImplementedError

    def _args(self, cost, sources):
        _costdistance.costdistance_args(cost, sources, self.threshold, self.output,
                                        self.cellsize, self.frac_bits, self.max_distance)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._args(image_to_filter, self.sources)
        outs, self.stats = _costdistance.costdistance(
            image_to_filter, _Given(self.sources).host(), self.threshold, self.output,
            self.cellsize, self.frac_bits, self.max_distance)
        return outs[self.output]

    def apply_device(self, raster):
        self._args(raster, self.sources)
        with _Given(self.sources).device(raster.ctx) as sources:
            outs, self.stats = _costdistance.costdistance_dev(
                raster, sources, self.threshold, self.output, self.cellsize, self.frac_bits,
                self.max_distance)
        return outs[self.output]


class CostDistance(_CostFromSources):  # pylint: disable=too-few-public-methods
    """Least accumulated cost to the nearest source (new operator; ArcGIS *Cost Distance* and
    *Cost Back Link*, Whitebox ``CostDistance``, GRASS ``r.cost``).  Input, ``sources``,
    arithmetic, errors and ``stats``: ``_CostFromSources``.  ``output``: ``"distance"`` float32
    ``float32(float64(D) * cellsize * 2^-(frac_bits+1))``, NaN out of reach; ``"units"`` int64
    ``D``, -1 out of reach; ``"backlink"`` uint8, the ESRI D8 code of the first neighbour in
    window order (NW, N, NE, W, E, SW, S, SE) on a least path, 0 at sources and out of reach.
    The back links are D8 codes whose paths end at sources: ``Watersheds``, ``FlowDistance``,
    ``FlowPathSum``, ``WeightedFlowAccumulation`` and ``CostPath`` take them as they are."""

    OUTPUTS = ("distance", "units", "backlink")

    def _default_output(self, threshold):
        return "distance"


class CostAllocation(_CostFromSources):  # pylint: disable=too-few-public-methods
    """The source every cell's least-cost path ends in (new operator; ArcGIS *Cost Allocation*,
    Whitebox ``CostAllocation``).  Input, ``sources``, arithmetic, errors and ``stats``:
    ``_CostFromSources``.  ``output``: ``"nearest"`` uint32, the flat index of the source the
    back links of ``CostDistance`` lead to, 0xFFFFFFFF out of reach; ``"label"`` uint32, that
    source's label, 0 out of reach (uint32 label sources only, where it is the default)."""

    OUTPUTS = ("nearest", "label")

    def _default_output(self, threshold):
        labels = np.dtype(self.sources.dtype) == np.uint32 and threshold is None
        return "label" if labels else "nearest"


class CostPath(Filter):  # pylint: disable=too-few-public-methods
    """Least-cost paths from destinations back to their sources (new operator; ArcGIS *Cost
    Path*, Whitebox ``CostPathway``).  Input: the uint8 back-link raster of ``CostDistance``.
    ``destinations``: a bool / uint8 mask of its shape (array or ``DeviceRaster``; non-zero = a
    destination), or a list of ``(row, column)`` cells.  Returns a uint8 mask: 1 on every cell
    of a back-link path from a destination to its source, both ends included; a destination out
    of reach marks only itself.  It is ``WeightedFlowAccumulation`` on the back links with the
    destinations as uint8 weights, written as its mask at threshold 1: exact, device-resident,
    with that operator's errors and ``stats``."""

    auto_device = True      # device form == host form for a uint8 code raster

    def __init__(self, destinations):
        if destinations is None:
            raise ValueError("CostPath needs the destinations it starts from (a mask or a list "
                             "of (row, column) cells)")
        if isinstance(destinations, np.ndarray) or backend.is_device_raster(destinations):
            self.cells = None
            self.destinations = _Given(destinations, "destinations", (np.bool_, np.uint8)).value
        else:
            try:
                cells = [(int(r), int(c)) for r, c in destinations]
            except (TypeError, ValueError):
                raise ValueError("destinations are a uint8 mask or a list of (row, column) "
                                 f"cells, got {destinations!r}") from None
            if not cells or any(r < 0 or c < 0 for r, c in cells):
                raise ValueError("destinations are a uint8 mask or a list of (row, column) "
                                 f"cells, got {destinations!r}")
            self.cells, self.destinations = cells, None
        self.stats = {}

    def _mask(self, shape):
        if self.cells is None:
            return self.destinations
        mask = np.zeros(shape, np.uint8)
        for row, col in self.cells:
            if row >= shape[0] or col >= shape[1]:
                raise ValueError(f"destination ({row}, {col}) lies outside the {shape[0]} x "
                                 f"{shape[1]} raster")
            mask[row, col] = 1
        return mask

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("CostPath", image_to_filter, np.uint8, "uint8 back-link codes")
        mask = _Given(self._mask(tuple(image_to_filter.shape))).host()
        outs, self.stats = _flowsum.flowsum(image_to_filter, mask, 0, "mask", 1)
        return outs["mask"]

    def apply_device(self, raster):
        _check_raster("CostPath", raster, np.uint8, "uint8 back-link codes")
        with _Given(self._mask(tuple(raster.shape))).device(raster.ctx) as mask:
            outs, self.stats = _flowsum.flowsum_dev(raster, mask, 0, "mask", 1)
        return outs["mask"]


class ResolveFlats(Filter):  # pylint: disable=too-few-public-methods
    """D8 directions across flats (new operator).  Input: a uint8 H x W raster of ESRI D8 codes
    as ``D8FlowDirection`` returns them, and -- at construction -- the float32 ``dem`` they
    were made on (array or ``DeviceRaster``, NaN = nodata).  ``D8FlowDirection`` only routes
    strictly downhill, so every cell of a flat, and of a depression filled with
    ``epsilon=0``, has code 0.  Returns uint8 codes in which those cells point along a
    shortest path of equal elevation to where their flat drains.  "Equal" is float ``==``:
    -0.0 equals 0.0 and NaN equals nothing.

    *Drains*: non-NaN cells with a code != 0, on the raster ring or with a NaN neighbour.
    *Flat cells*: every other non-NaN cell.  ``dist[c]`` of a flat cell is the length of the
    shortest 8-connected path from ``c`` through flat cells of ``c``'s elevation to a drain of
    that elevation.  A flat cell with a finite distance gets the code of the first neighbour
    in D8 window order (NW, N, NE, W, E, SW, S, SE) that has its elevation and distance
    ``dist[c] - 1`` (drains count as 0); every other cell keeps its code, so a flat that
    cannot drain -- a pit of an unfilled DEM -- stays 0 and is counted in
    ``stats["unresolved"]``.

    The distance strictly decreases along the new codes: the result is acyclic whenever the
    input is.  On a DEM filled with ``epsilon=0`` no cell is unresolved, and the only interior
    cells left at 0 are nodata cells and their neighbours, which the fill treats as outlets.
    The elevations are not touched, and nothing depends on an ``epsilon`` that float32 could
    absorb.  Exact integers, identical from run to run.

    ``ValueError`` for a ``dem`` that is missing, of another type, dtype or dimension (at
    construction), codes that are not a 2-D uint8 raster of the dem's shape (before the
    device is touched), a byte that is not a D8 code and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        flat_cells, unresolved, max_distance, rounds (relaxation rounds that had work),
        active_tiles, tile_visits, tile_h / tile_w of the last call; phase times when
        profiling is on.
    distance : numpy.ndarray, DeviceRaster or None
        with ``keep_partial_results=True`` the uint32 distances of the last call (0 outside
        the flats, 0xFFFFFFFF where unresolved): a host array after ``apply``, a device
        raster (the caller's to free) after ``apply_device``.
    """

    auto_device = True      # device form == host form for a uint8 code raster

    def __init__(self, *, dem, keep_partial_results=False):
        if dem is None:
            raise ValueError("ResolveFlats needs the dem the codes were made on")
        self.dem = _Given(dem, "dem", (np.float32,)).value
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.distance = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        backend.resolve_flats_args(image_to_filter, self.dem)
        out, self.distance, self.stats = backend.resolve_flats(
            image_to_filter, _Given(self.dem).host(), self.keep_partial_results)
        return out

    def apply_device(self, raster):
        backend.resolve_flats_args(raster, self.dem)
        with _Given(self.dem).device(raster.ctx) as dem:
            out, self.distance, self.stats = backend.resolve_flats_dev(
                raster, dem, self.keep_partial_results)
        return out


class Depressions(Filter):  # pylint: disable=too-few-public-methods
    """Depression labelling and inventory (new operator).  Applied to a **filled** float32
    raster, with -- at construction -- the float32 ``dem`` it is compared with (array or
    ``DeviceRaster``).  A cell is *raised* where ``filled > dem`` (false where either is NaN);
    a depression is an 8-connected component of raised cells and ``first`` its smallest flat
    index ``y * W + x``.  Any such pair of rasters is legal, not only a DEM and its sink fill.
    Returns uint32 labels, 0 where the cell is not raised.

    ``labels="compact"`` (default): the depressions numbered 1 ... K in ascending order of
    ``first`` -- exactly ``scipy.ndimage.label(filled > dem, structure=np.ones((3, 3)))``.
    ``labels="first"``: ``1 + first`` of the cell's depression.

    ``table=True`` (compact labels only) also fills ``table``, one row per label ``k`` at
    index ``k - 1``: ``first`` (uint32), ``area`` (uint32, cells), ``level`` (float32, the
    minimum of ``filled``: the water level after an ``epsilon=0`` fill), ``max_depth``
    (float32, the maximum of ``filled - dem``), ``volume_q20`` (uint64, the sum of the depths
    in units of 2^-20, each rounded to nearest even and saturating at 2^31 - 1) and
    ``volume`` (float64, ``volume_q20 / 2**20 * cellsize**2``).  Labels and table are exact,
    identical from run to run and from ``apply`` and ``apply_device``.

    ``ValueError`` for a ``dem`` that is missing or of another type, dtype or dimension,
    unknown ``labels``, a table without compact labels, a bad ``cellsize`` (all at
    construction), a filled raster that is not 2-D float32 of the dem's shape (before the
    device is touched) and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        depressions (K), raised_cells, tile_components, tile_h / tile_w of the last call;
        phase times when profiling is on.
    count : int or None
        K of the last call.
    table : dict of numpy.ndarray, or None
        the table of the last call: host arrays of length K, whichever form was called.
    """

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, *, dem, labels="compact", table=False, cellsize=1.0):
        if dem is None:
            raise ValueError("Depressions needs the dem the filled raster is compared with")
        dem = _Given(dem, "dem", (np.float32,)).value
        if labels not in ("first", "compact"):
            raise ValueError(f"labels is 'first' or 'compact', got {labels!r}")
        if table and labels != "compact":
            raise ValueError("the table has one row per compact label: table=True needs "
                             "labels='compact'")
        self.dem = dem
        self.labels = labels
        self.want_table = bool(table)
        self.cellsize = backend._cellsize(cellsize)  # pylint: disable=protected-access
        self.stats = {}
        self.count = None
        self.table = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        backend.depressions_args(self.dem, image_to_filter)
        dem = _Given(self.dem).host()
        self.table = None
        out, self.stats = backend.depressions(dem, image_to_filter, self.labels == "compact")
        self.count = self.stats["depressions"]
        if self.want_table:
            self.table = backend.depression_table(dem, image_to_filter, out, self.count,
                                                  self.cellsize)
        return out

    def apply_device(self, raster):
        backend.depressions_args(self.dem, raster)
        self.table = None
        with _Given(self.dem).device(raster.ctx) as dem, \
                backend.result_raster(None, raster.shape, np.uint32, raster.ctx) as out:
            _, self.stats = backend.depressions_dev(dem, raster, self.labels == "compact",
                                                    out=out)
            self.count = self.stats["depressions"]
            if self.want_table:
                self.table = backend.depression_table_dev(dem, raster, out, self.count,
                                                          self.cellsize)
        return out


class DepressionInventory(Filter):  # pylint: disable=too-few-public-methods
    """A float32 DEM to its depressions in one device-resident pass: ``SinkFill(epsilon)``,
    then compact ``Depressions`` labels of the DEM and its fill, then their table.  The DEM is
    uploaded once and nothing is downloaded in between.  Returns the uint32 labels.

    ``filled`` is the filled DEM of the last call: a host array after ``apply``, a device
    raster (the caller's to free) after ``apply_device``.  ``table`` (host arrays, see
    ``Depressions``), ``count`` and ``stats`` (of the labelling; ``fill_stats`` of the fill)
    are those of the last call."""

    def __init__(self, *, epsilon=0.0, cellsize=1.0):
        try:
            self.epsilon = float(epsilon)
        except (TypeError, ValueError):
            raise ValueError(f"epsilon is a number, got {epsilon!r}") from None
        if not np.isfinite(self.epsilon) or self.epsilon < 0:
            raise ValueError(f"epsilon must be finite and not negative, got {epsilon}")
        self.cellsize = backend._cellsize(cellsize)  # pylint: disable=protected-access
        self.filled = self.table = self.count = None
        self.stats, self.fill_stats = {}, {}

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DepressionInventory", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter, ("filled",))

    def apply_device(self, raster):
        _check_raster("DepressionInventory", raster, np.float32, "a float32 DEM")
        self.filled = self.table = self.count = None
        with contextlib.ExitStack() as stack:
            filled, self.fill_stats = backend.sinkfill_dev(raster, self.epsilon)
            stack.enter_context(filled)
            labels = Depressions(dem=raster, table=True, cellsize=self.cellsize)
            out = labels.apply_device(filled)
            self.stats, self.count, self.table = labels.stats, labels.count, labels.table
            self.filled = filled
            stack.pop_all()                         # the caller's to free from here on
        return out


def _check_flats(flats):
    if flats not in ("keep", "resolve"):
        raise ValueError(f"flats is 'keep' or 'resolve', got {flats!r}")
    return flats


class HydroConditioning(ComposedFilter):  # pylint: disable=too-few-public-methods
    """``SinkFill`` then ``D8FlowDirection`` as one device-resident chain (the
    pair BASELINE.json's metric is quoted on).  ``filled`` keeps the filled
    DEM of the last ``apply``; the return value is the D8 grid.

    ``flats="resolve"`` appends ``ResolveFlats`` on the filled DEM, still on the device with
    no download in between: with ``epsilon=0`` the flats the fill makes then drain, and the
    elevations stay those of the exact fill.  ``resolve_stats`` holds that stage's stats.
    The default ``flats="keep"`` leaves code 0 on flats.  ``apply_batch``, the canvas form,
    has no resolution stage: with ``flats="resolve"`` it raises ``ValueError``."""

    def __init__(self, *, epsilon=0.0, flats="keep"):
        super().__init__()
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection()]
        self.flats = _check_flats(flats)
        self.filled = None
        self.resolve_stats = {}

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        with backend.DeviceRaster.from_host(image_to_filter, dtype=np.float32) as z, \
                contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, z, self.filters[0], self.flats)
            if resolve_stats is not None:
                self.resolve_stats = resolve_stats
            self.filled = filled.to_host()
            return codes.to_host()

    def apply_batch(self, rasters):
        """Fill + D8 of several rasters in ONE pass of the solver: ``[(filled, codes), ...]``.

        Small rasters (SRTM / HydroSHEDS tiles are 1201^2 ... 6000^2 cells) leave most of the
        GPU idle -- a fill is a chain of dependent tile visits -- so those of one width are
        stacked into one canvas with a nodata row between neighbours.  That changes no result: the cells next to nodata are pinned exactly as
        a raster's ring is (the operator's own rule), so every raster fills as it does alone;
        only the D8 codes of each raster's ring are put back to 0 afterwards (on the canvas
        they have neighbours).  The arrays returned are views of the downloaded canvases (one
        pair of canvases per width).  Bit-equal to ``apply`` raster by raster
        (``tests/test_gpu_parity.py::test_batch_of_rasters_fills_like_each_alone``).
        ``flats="resolve"`` is not available here: ``ValueError``."""
        if self.flats != "keep":
            raise ValueError("apply_batch does not resolve flats: use apply raster by raster "
                             "with flats='resolve'")
        rasters = [np.asarray(r, dtype=np.float32) for r in rasters]
        for r in rasters:
            Filter.apply(self, r)
            if r.ndim != 2:
                raise ValueError("apply_batch takes 2-D rasters")
        if not rasters:
            return []
        rasters = [np.ascontiguousarray(r) for r in rasters]
        ctx = backend.context()
        lib, hnd = ctx.lib, ctx.handle
        fill = self.filters[0]
        out = [None] * len(rasters)
        # one canvas per width (tiles of a survey share theirs): a raster then is one
        # contiguous block of its canvas and goes up and comes down in one plain copy each
        # (pitched copies from pageable memory run row by row: 30 x slower)
        by_width = {}
        for k, r in enumerate(rasters):
            by_width.setdefault(r.shape[1], []).append(k)
        stats = None
        for width, members in by_width.items():
            rows = sum(rasters[k].shape[0] for k in members) + len(members) - 1
            with backend.DeviceRaster.empty((rows, width), np.float32, ctx) as z:
                ctx.check(lib.hdem_memset_dev(hnd, z.ptr, 0xff, z.nbytes))      # all NaN
                tops, y = [], 0
                for k in members:
                    r = rasters[k]
                    ctx.check(lib.hdem_memcpy_h2d(hnd, z.ptr + y * width * 4, r.ctypes.data, r.nbytes))
                    tops.append(y)
                    y += r.shape[0] + 1
                filled, codes, st = backend.sinkfill_d8_dev(z, eps=fill.epsilon,
                                                            max_rounds=fill.max_rounds)
                stats = st if stats is None else {
                    key: (min(stats[key], st[key]) if key == "converged" else stats[key] + st[key])
                    if isinstance(st[key], int) else st[key] for key in st}
                with filled, codes:
                    # the canvas comes down in two copies (page-locked blocks of the library,
                    # backend.host_empty); what is handed out are views of it, one per raster
                    # -- many small copies into fresh pageable arrays were measured at 200 ms
                    # for 16 tiles, the driver pinning and unpinning their pages
                    w_all, d_all = filled.to_host(), codes.to_host()
                for k, y0 in zip(members, tops):
                    h = rasters[k].shape[0]
                    d = d_all[y0:y0 + h]
                    d[0], d[-1], d[:, 0], d[:, -1] = 0, 0, 0, 0
                    out[k] = (w_all[y0:y0 + h], d)
        fill.stats = stats or {}
        return out


class DemToHAND(ComposedFilter):  # pylint: disable=too-few-public-methods
    """A float32 DEM to its height above the nearest drainage in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``FlowAccumulation``, then ``HeightAboveDrainage`` relative to the **filled** DEM with
    streams where the accumulation is ``>= threshold``.  Nothing is downloaded in between.

    ``stats`` maps ``SinkFill``, ``FlowAccumulation`` and ``HeightAboveDrainage`` to the
    stats of their stage.  With ``keep_partial_results=True`` the last call leaves
    ``filled``, ``codes``, ``accumulation`` and ``distance`` (distance to the streams): host
    arrays after ``apply``, device rasters (the caller's to free) after ``apply_device``;
    otherwise they are ``None``.  ``epsilon > 0`` makes the D8 paths of the filled DEM descend
    strictly, so that they cross what were flats and pits.

    ``flats="resolve"`` runs ``ResolveFlats`` on the filled DEM between the D8 and the
    accumulation, and the resolved codes feed every later stage (``codes`` keeps them,
    ``stats["ResolveFlats"]`` that stage's stats).  ``epsilon=0.0, flats="resolve"`` is the
    exact route: the paths cross the filled depressions on elevations no gradient has
    raised.  The default ``flats="keep"`` changes nothing."""

    def __init__(self, *, threshold, epsilon=1e-3, cellsize=1.0, keep_partial_results=False,
                 flats="keep"):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the trace's operands, on stand-ins of the types the chain makes
        HeightAboveDrainage(dem=np.zeros((1, 1), np.float32),
                            streams=np.zeros((1, 1), np.uint32), threshold=threshold,
                            cellsize=cellsize)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(), FlowAccumulation()]
        self.threshold, self.cellsize = threshold, cellsize
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.accumulation = self.distance = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToHAND", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "accumulation", "distance")
                               if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToHAND", raster, np.float32, "a float32 DEM")
        fill, _, accumulate = self.filters
        self.filled = self.codes = self.accumulation = self.distance = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            acc, accumulate.stats = backend.flowacc_dev(codes)
            stack.enter_context(acc)
            trace = HeightAboveDrainage(dem=filled, streams=acc, threshold=self.threshold,
                                        cellsize=self.cellsize,
                                        keep_partial_results=self.keep_partial_results)
            hand = trace.apply_device(codes)
            self.stats = {"SinkFill": fill.stats, "FlowAccumulation": accumulate.stats,
                          "HeightAboveDrainage": trace.stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                trace.drainage.free()
                self.filled, self.codes, self.accumulation = filled, codes, acc
                self.distance = trace.distance
                stack.pop_all()                     # the caller's to free from here on
            return hand


class BreachDepressions(ComposedFilter):  # pylint: disable=too-few-public-methods
    """Depression breaching (new operator; Soille's carving, Whitebox and RichDEM
    *BreachDepressions*): the other way to condition a DEM.  Where ``SinkFill`` raises every
    depression to its spill level, this cuts a trench at the level of each pit down to where the
    terrain is lower again and leaves the rest of the depression alone.  Takes a float32 DEM and
    returns the carved DEM.

    One device-resident chain, nothing downloaded in between: ``SinkFill(epsilon=0)`` and
    ``D8FlowDirection`` with ``ResolveFlats`` (one call, as in
    ``HydroConditioning(epsilon=0.0, flats="resolve")``) give a forest in which every cell
    reaches an outlet, then one reduction up that forest: every cell takes the elevation of the
    lowest pit upstream of it where that is below its own, and stays bit for bit otherwise (NaN
    included).  A pit is a non-NaN cell off the raster's one-cell ring with no NaN neighbour and
    no strictly lower neighbour.  An outlet on the ring that a trench reaches is lowered too.

    The carved DEM has no sinks (its ``epsilon=0`` fill is itself) and carving it again changes
    nothing.  ``HydroConditioning(epsilon=0.0, flats="resolve")`` gives its D8 codes.

    ``stats`` maps ``SinkFill``, ``ResolveFlats`` and ``BreachDepressions`` (pits, lowered,
    exits, max_hops, ...) to the stats of their stage.  With ``keep_partial_results=True`` the
    last call leaves ``filled`` (the exact fill), ``codes`` (the forest) and ``source`` (uint32,
    the flat index of the pit a cell was lowered to, ``0xFFFFFFFF`` where it is unchanged): host
    arrays after ``apply``, device rasters (the caller's to free) after ``apply_device``;
    otherwise they are ``None``."""

    def __init__(self, keep_partial_results=False):
        super().__init__()
        self.filters = [SinkFill(epsilon=0.0), D8FlowDirection()]
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.source = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("BreachDepressions", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "source")
                               if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("BreachDepressions", raster, np.float32, "a float32 DEM")
        fill = self.filters[0]
        self.filled = self.codes = self.source = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, "resolve")
            outs, breach_stats = _upextreme.breach_dev(
                raster, codes, ("carved", "source") if self.keep_partial_results else ("carved",))
            self.stats = {"SinkFill": fill.stats, "ResolveFlats": resolve_stats,
                          "BreachDepressions": breach_stats}
            if self.keep_partial_results:
                self.filled, self.codes, self.source = filled, codes, outs["source"]
                stack.pop_all()                     # the caller's to free from here on
            return outs["carved"]


class DemToWetness(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its topographic wetness index in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``FlowAccumulation``, then ``WetnessIndex`` on the **filled** DEM with that accumulation
    (and, with ``slope="d8"``, the slope along those codes).  Nothing is downloaded in
    between.  ``flats`` as in ``DemToHAND``.

    ``stats`` maps ``SinkFill``, ``FlowAccumulation`` and ``WetnessIndex`` (and
    ``ResolveFlats``) to the stats of their stage.  With ``keep_partial_results=True`` the last
    call leaves ``filled``, ``codes``, ``accumulation`` and ``tangent`` (Horn's, written by the
    wetness launch): host arrays after ``apply``, device rasters (the caller's to free) after
    ``apply_device``; otherwise they are ``None``."""

    def __init__(self, *, epsilon=1e-3, flats="keep", cellsize=1.0, min_slope=1e-3,
                 slope="horn", keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the last stage's operands, on stand-ins of the types the chain makes
        _terrain.terrain_args(np.zeros((1, 1), np.float32), ("tangent", "twi"), cellsize, 1.0,
                              np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint32),
                              min_slope, slope)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(), FlowAccumulation()]
        self.cellsize, self.min_slope, self.slope = cellsize, min_slope, slope
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.accumulation = self.tangent = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToWetness", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "accumulation", "tangent")
                               if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToWetness", raster, np.float32, "a float32 DEM")
        fill, _, accumulate = self.filters
        self.filled = self.codes = self.accumulation = self.tangent = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            acc, accumulate.stats = backend.flowacc_dev(codes)
            stack.enter_context(acc)
            outs, stats = _terrain.terrain_dev(
                filled, ("tangent", "twi") if self.keep_partial_results else ("twi",),
                self.cellsize, 1.0, codes, acc, self.min_slope, self.slope)
            self.stats = {"SinkFill": fill.stats, "FlowAccumulation": accumulate.stats,
                          "WetnessIndex": stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.accumulation = filled, codes, acc
                self.tangent = outs["tangent"]
                stack.pop_all()                     # the caller's to free from here on
            return outs["twi"]


class DInfFlowDirection(Filter):  # pylint: disable=too-few-public-methods
    """Tarboton's D-infinity flow direction (new operator; TauDEM ``dinfflowdir``).  Input: a
    float32 H x W DEM, NaN where there is no data.  Returns one uint32 word per cell
    (``hydrodem_amd.dinf``): ``q`` in bits 0-15, the share of the outflow that goes to the
    diagonal receiver in units of 2^-15, and the facet 0 ... 8 in bits 16-19.  The steepest of the
    eight triangular facets wins, the first one on a tie; the slopes are float64 on the float32
    elevations.  Cells of the raster ring, NaN cells and cells without a downward facet get 0:
    no outflow.

    ``cellsize``: a number or ``(dx, dy)``.  ``fallback``: uint8 ESRI D8 codes of the DEM's shape
    (array or ``DeviceRaster``); a cell that would get 0 takes its code's direction, so that the
    flats of an exact fill routed by ``ResolveFlats`` keep draining.  With
    ``keep_partial_results=True`` the launch also writes ``angle`` (float32 radians
    counter-clockwise from east, -1 without outflow) and ``slope`` (the winner's, 0 where none
    won, NaN at NaN) and leaves them in the attributes of those names: host arrays after
    ``apply``, device rasters (the caller's to free) after ``apply_device``.

    ``ValueError`` for a dtype other than float32, a raster that is not 2-D, a ``cellsize`` that
    is not finite and positive, a ``fallback`` of another type, dtype or shape (all before the
    device is touched) and a fallback byte that is no D8 code.

    Attributes
    ----------
    stats : dict
        no_flow (cells with word 0), fallback_cells of the last call; ms_total when profiling.
    """

    auto_device = False     # words are uint32: no float32 chain goes on from them

    def __init__(self, cellsize=1.0, fallback=None, keep_partial_results=False):
        self.cellsize = cellsize
        self.fallback = _Given(fallback, "fallback", (np.uint8,)).value
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.angle = self.slope = None
        _dinf.dinf_args(np.zeros((1, 1), np.float32), cellsize, _Given(self.fallback).stand_in())

    def _want(self):
        return _dinf.EXTRAS if self.keep_partial_results else ()

    def _keep(self, words, extras, stats):
        self.stats = stats
        self.angle, self.slope = extras.get("angle"), extras.get("slope")
        return words

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _dinf.dinf_args(image_to_filter, self.cellsize, self.fallback)
        return self._keep(*_dinf.dinf(image_to_filter, self.cellsize,
                                      _Given(self.fallback).host(), self._want()))

    def apply_device(self, raster):
        _dinf.dinf_args(raster, self.cellsize, self.fallback)
        with _Given(self.fallback).device(raster.ctx) as fallback:
            return self._keep(*_dinf.dinf_dev(raster, self.cellsize, fallback, self._want()))


class DInfFlowAccumulation(Filter):  # pylint: disable=too-few-public-methods
    """D-infinity flow accumulation (new operator; TauDEM ``areadinf``).  Input: a uint32 H x W
    raster of D-infinity words as ``DInfFlowDirection`` returns them.  With ``U = 2^frac_bits``,
    ``A[c] = U + sum(share(d -> c))`` over the 8-neighbours ``d`` whose word names ``c``: a donor
    sends ``(A[d] * q[d]) >> 15`` to its diagonal receiver and the rest to its cardinal one.
    Integers throughout: every cell's outflow is conserved to the unit, ``A`` summed over the
    cells without outflow is ``H * W * U`` exactly, and the result is identical from run to run.

    ``output``: ``"value"`` float32 ``float32(float64(A) * 2^-frac_bits)``, the catchment area
    in cells; ``"sum"`` int64 ``A``.  ``frac_bits`` is 0 ... 16.

    ``ValueError`` for a dtype other than uint32, a raster that is not 2-D, ``frac_bits`` out of
    range, an unknown ``output`` (all before the device is touched), an invalid word, a
    receiver outside the raster, words that form a cycle (only user-supplied words can) and
    more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        split_cells, terminal_cells, invalid, outside, unresolved, rounds and tile_visits
        (these two depend on the schedule), tile_h / tile_w of the last call; phase times when
        profiling is on.
    """

    auto_device = False     # the input is uint32 words, not a float32 raster
    OUTPUTS = {name: np.dtype(dtype) for name, dtype in _dinf.OUTPUTS}

    def __init__(self, frac_bits=16, output="value"):
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self.frac_bits, self.output = _dinf.check_frac_bits(frac_bits), output
        self.dtype = self.OUTPUTS[output]
        self.stats = {}

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _dinf.dinfacc_args(image_to_filter, self.frac_bits, self.output)
        outs, self.stats = _dinf.dinfacc(image_to_filter, self.frac_bits, self.output)
        return outs[self.output]

    def apply_device(self, raster):
        _dinf.dinfacc_args(raster, self.frac_bits, self.output)
        outs, self.stats = _dinf.dinfacc_dev(raster, self.frac_bits, self.output)
        return outs[self.output]


class DemToDInfArea(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its D-infinity catchment area in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``DInfFlowDirection`` on the **filled** DEM with the chain's D8 codes as fallback, then
    ``DInfFlowAccumulation``.  Nothing is downloaded in between.  ``flats`` as in ``DemToHAND``:
    with ``"resolve"`` the fallback codes cross the flats, so an exact fill (``epsilon=0``)
    drains; ``cellsize``, ``frac_bits`` and ``output`` as in the two operators.

    ``stats`` maps ``SinkFill``, ``DInfFlowDirection`` and ``DInfFlowAccumulation`` (and
    ``ResolveFlats``) to the stats of their stage.  With ``keep_partial_results=True`` the last
    call leaves ``filled``, ``codes`` and ``words``: host arrays after ``apply``, device rasters
    (the caller's to free) after ``apply_device``; otherwise they are ``None``."""

    def __init__(self, *, epsilon=1e-3, flats="keep", cellsize=1.0, frac_bits=16,
                 output="value", keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(),
                        DInfFlowDirection(cellsize=cellsize),
                        DInfFlowAccumulation(frac_bits=frac_bits, output=output)]
        self.cellsize, self.frac_bits, self.output = cellsize, frac_bits, output
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.words = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToDInfArea", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "words") if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToDInfArea", raster, np.float32, "a float32 DEM")
        fill, _, direct, accumulate = self.filters
        self.filled = self.codes = self.words = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            words, _, direct.stats = _dinf.dinf_dev(filled, self.cellsize, codes)
            stack.enter_context(words)
            outs, accumulate.stats = _dinf.dinfacc_dev(words, self.frac_bits, self.output)
            self.stats = {"SinkFill": fill.stats, "DInfFlowDirection": direct.stats,
                          "DInfFlowAccumulation": accumulate.stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.words = filled, codes, words
                stack.pop_all()                     # the caller's to free from here on
            return outs[self.output]


class WeightedDInfFlowAccumulation(Filter):  # pylint: disable=too-few-public-methods
    """Weighted D-infinity flow accumulation (new operator; TauDEM ``areadinf -wg``).  Input: a
    uint32 H x W raster of D-infinity words as ``DInfFlowDirection`` returns them.  ``weights``:
    an H x W NumPy array or ``DeviceRaster`` of uint8, uint32 or float32 (float64 is refused, not
    narrowed).  Every cell's weight is quantised to an integer ``q``: ``w << frac_bits`` for the
    integer types (``frac_bits`` 0 ... 16: a cell that splits an integer load still needs
    resolution below one unit), ``rint(float64(w) * 2^frac_bits)`` for float32 (``frac_bits``
    0 ... 30).  ``A[c] = q[c] + sum(share(d -> c))`` with the shares of
    ``DInfFlowAccumulation``, in integers: every unit of every weight arrives at a cell without
    outflow, and the result is identical from run to run.

    ``output``: ``"value"`` float32 ``float32(float64(A) * 2^-frac_bits)``, in weight units;
    ``"sum"`` int64 ``A``.

    A NaN weight contributes 0 (``stats["nan_weights"]`` counts them).  ``ValueError`` for
    operands of another type, dtype or shape, ``frac_bits`` out of range for the weights, an
    unknown ``output`` (all before the device is touched), for a negative or infinite weight, a
    quantised weight above 2^31 - 1, quantised weights that sum to 2^48 or more (so that no
    share can overflow), an invalid word, a receiver outside the raster, words that form a
    cycle and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        those of ``DInfFlowAccumulation``, nan_weights, bad_weights and total (the sum of the
        quantised weights: what the cells without outflow hold between them) of the last call.
    """

    auto_device = False     # the input is uint32 words, not a float32 raster
    WEIGHT_TYPES = (np.uint8, np.uint32, np.float32)
    OUTPUTS = {name: np.dtype(dtype) for name, dtype in _dinf.OUTPUTS}

    def __init__(self, weights, frac_bits=16, output="value"):
        if weights is None:
            raise ValueError("WeightedDInfFlowAccumulation needs the weights it sums")
        self.weights = _Given(weights, "weights", self.WEIGHT_TYPES).value
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self.frac_bits, self.output = frac_bits, output
        self.dtype = self.OUTPUTS[output]
        self.stats = {}
        # everything but the shapes, on 1 x 1 stand-ins
        _dinf.dinfsum_args(np.empty((1, 1), np.uint32), _Given(self.weights).stand_in(),
                           frac_bits, output)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _dinf.dinfsum_args(image_to_filter, self.weights, self.frac_bits, self.output)
        outs, self.stats = _dinf.dinfsum(image_to_filter, _Given(self.weights).host(),
                                         self.frac_bits, self.output)
        return outs[self.output]

    def apply_device(self, raster):
        _dinf.dinfsum_args(raster, self.weights, self.frac_bits, self.output)
        with _Given(self.weights).device(raster.ctx) as weights:
            outs, self.stats = _dinf.dinfsum_dev(raster, weights, self.frac_bits, self.output)
        return outs[self.output]


class AreaWetnessIndex(Filter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """The topographic wetness index ``ln(a / max(tan b, min_slope))`` of a float32 DEM and a
    float32 catchment ``area`` in cells -- the ``value`` of ``DInfFlowAccumulation`` or
    ``WeightedDInfFlowAccumulation`` (TauDEM ``twi`` on ``sca`` and ``slp``).  ``a`` is the area
    times ``sqrt(dx dy)``; ``tan b`` is ``given_slope`` where one is passed (float32, the D-infinity
    ``slope``), else Horn's tangent of the DEM.  The arithmetic is ``TerrainAttributes``'s, with
    ``area`` where that has ``float32(accumulation)``.

    ``want`` names outputs of ``hydrodem_amd.terrain.TERRAIN_OUTPUTS`` (not ``d8_slope``); the
    first is returned, and with ``keep_partial_results=True`` the same launch writes the others
    and leaves them in the attributes of their names, as ``TerrainAttributes`` does.  ``area``
    and ``given_slope`` are arrays or ``DeviceRaster``s of the DEM's shape.  A NaN area gives
    NaN; zero and negative areas go through the arithmetic as they are
    (``stats["nonpositive_area"]`` counts them).

    ``ValueError`` for operands of another type, dtype or shape, unknown outputs, ``twi`` or
    ``spi`` without the area, a ``cellsize``, ``z_factor`` or ``min_slope`` that is not finite
    and positive: all before the device is touched.
    """

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, area, given_slope=None, cellsize=1.0, z_factor=1.0, min_slope=1e-3,
                 want=("twi",), keep_partial_results=False):
        self.want = (want,) if isinstance(want, str) else tuple(want)
        self.cellsize, self.z_factor, self.min_slope = cellsize, z_factor, min_slope
        self.area = _Given(area, "area", (np.float32,)).value
        self.given_slope = _Given(given_slope, "given_slope", (np.float32,)).value
        self.slope = "horn" if given_slope is None else "given"
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        for name in _terrain.TERRAIN_OUTPUTS:
            setattr(self, name, None)
        # everything but the shapes, on 1 x 1 stand-ins
        self._args(np.zeros((1, 1), np.float32), _Given(self.area).stand_in(),
                   _Given(self.given_slope).stand_in())

    def _args(self, dem, area, given_slope):
        return _terrain.terrain_area_args(dem, self.want, self.cellsize, self.z_factor, area,
                                          given_slope, None, self.min_slope, self.slope)

    def _run(self, run, dem, area, given_slope):
        want = self.want if self.keep_partial_results else self.want[:1]
        outs, self.stats = run(dem, want, self.cellsize, self.z_factor, area, given_slope, None,
                               self.min_slope, self.slope)
        for name in _terrain.TERRAIN_OUTPUTS:
            setattr(self, name, outs.get(name) if name != self.want[0] else None)
        return outs[self.want[0]]

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._args(image_to_filter, self.area, self.given_slope)
        return self._run(_terrain.terrain_area, image_to_filter, _Given(self.area).host(),
                         _Given(self.given_slope).host())

    def apply_device(self, raster):
        self._args(raster, self.area, self.given_slope)
        with _Given(self.area).device(raster.ctx) as area, \
                _Given(self.given_slope).device(raster.ctx) as given_slope:
            return self._run(_terrain.terrain_area_dev, raster, area, given_slope)


class DemToDInfWetness(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its D-infinity wetness index in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call), ``DInfFlowDirection`` on the
    **filled** DEM with the chain's D8 codes as fallback, ``DInfFlowAccumulation`` -- or
    ``WeightedDInfFlowAccumulation`` when ``weights`` (uint8, uint32 or float32, array or
    ``DeviceRaster``) is given -- and ``AreaWetnessIndex`` on the filled DEM with that area.
    ``slope="dinf"`` takes the D-infinity slope of the direction launch as ``tan b``,
    ``slope="horn"`` Horn's tangent.  Nothing is downloaded in between.  ``flats`` as in
    ``DemToHAND``; ``cellsize`` is a number or ``(dx, dy)`` as in ``DInfFlowDirection``.

    ``stats`` maps ``SinkFill``, ``DInfFlowDirection``, ``DInfFlowAccumulation`` (or
    ``WeightedDInfFlowAccumulation``) and ``AreaWetnessIndex`` (and ``ResolveFlats``) to the
    stats of their stage.  With ``keep_partial_results=True`` the last call leaves ``filled``,
    ``codes``, ``words``, ``area`` (and ``dinf_slope`` with ``slope="dinf"``): host arrays after
    ``apply``, device rasters (the caller's to free) after ``apply_device``; otherwise they are
    ``None``.  A failing stage leaves nothing allocated."""

    SLOPES = ("dinf", "horn")
    KEPT = ("filled", "codes", "words", "area", "dinf_slope")

    def __init__(self, *, epsilon=1e-3, flats="keep", cellsize=1.0, frac_bits=16,
                 min_slope=1e-3, slope="dinf", weights=None, keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        if slope not in self.SLOPES:
            raise ValueError(f"slope is 'dinf' or 'horn', got {slope!r}")
        self.weights = _Given(weights, "weights",
                              WeightedDInfFlowAccumulation.WEIGHT_TYPES).value
        dx, dy = _dinf.cellsizes(cellsize)
        # the checks of the later stages' operands, on stand-ins of the types the chain makes
        words, area = np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.float32)
        if weights is None:
            _dinf.dinfacc_args(words, frac_bits, "value")
        else:
            _dinf.dinfsum_args(words, _Given(self.weights).stand_in(), frac_bits, "value")
        _terrain.terrain_area_args(area, ("twi",), (dy, dx), 1.0, area,
                                   area if slope == "dinf" else None, None, min_slope,
                                   "given" if slope == "dinf" else "horn")
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(),
                        DInfFlowDirection(cellsize=cellsize)]
        self.cellsize, self.frac_bits, self.min_slope = cellsize, frac_bits, min_slope
        self.slope, self.keep_partial_results = slope, keep_partial_results
        self.stats = {}
        for name in self.KEPT:
            setattr(self, name, None)

    def _kept(self):
        return tuple(n for n in self.KEPT if n != "dinf_slope" or self.slope == "dinf")

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToDInfWetness", image_to_filter, np.float32, "a float32 DEM")
        if self.weights is not None:
            _dinf.dinfsum_args(np.empty(image_to_filter.shape, np.uint32), self.weights,
                               self.frac_bits, "value")
        return _through_device(self, image_to_filter,
                               self._kept() if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToDInfWetness", raster, np.float32, "a float32 DEM")
        fill, _, direct = self.filters
        for name in self.KEPT:
            setattr(self, name, None)
        dx, dy = _dinf.cellsizes(self.cellsize)
        given = self.slope == "dinf"
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            words, extras, direct.stats = _dinf.dinf_dev(filled, self.cellsize, codes,
                                                         ("slope",) if given else ())
            stack.enter_context(words)
            dinf_slope = stack.enter_context(extras["slope"]) if given else None
            if self.weights is None:
                stage = "DInfFlowAccumulation"
                outs, acc_stats = _dinf.dinfacc_dev(words, self.frac_bits, "value")
            else:
                stage = "WeightedDInfFlowAccumulation"
                with _Given(self.weights).device(raster.ctx) as weights:
                    outs, acc_stats = _dinf.dinfsum_dev(words, weights, self.frac_bits, "value")
            area = stack.enter_context(outs["value"])
            outs, stats = _terrain.terrain_area_dev(
                filled, ("twi",), (dy, dx), 1.0, area, dinf_slope, None, self.min_slope,
                "given" if given else "horn")
            self.stats = {"SinkFill": fill.stats, "DInfFlowDirection": direct.stats,
                          stage: acc_stats, "AreaWetnessIndex": stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.words, self.area = filled, codes, words, area
                self.dinf_slope = dinf_slope
                stack.pop_all()                     # the caller's to free from here on
            return outs["twi"]


class DInfDistanceDown(Filter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """D-infinity distance down (new operator; TauDEM ``dinfdistdown``).  Input: a uint32 H x W
    raster of D-infinity words as ``DInfFlowDirection`` returns them.  Returns float32: the
    distance from every cell down its D-infinity paths to the first *stop*, NaN where a path ends
    without one.  A stop cell reads 0.  A cell with one receiver adds its step to the receiver's
    distance; a cell with two combines the two sums by ``statistic``.

    ``kind``: ``"horizontal"`` (``dx`` / ``dy`` / the diagonal per step), ``"vertical"`` (the
    drop ``dem[c] - dem[r]`` per step: the height above the stop) or ``"surface"``
    (``sqrt(h^2 + v^2)`` per step); the last two need ``dem``, a float32 array or
    ``DeviceRaster`` of the words' shape.  ``statistic``: ``"average"`` weights the two receivers
    by their flow proportions and is NaN unless *every* path reaches a stop (TauDEM's rule);
    ``"maximum"`` is NaN in the same cells; ``"minimum"`` is the shortest way and NaN only where
    no path reaches a stop.  ``streams``: ``None`` (a stop is a cell without outflow: the
    distance to the outlet), a bool / uint8 mask, a uint32 raster with ``threshold`` (a stop where
    ``>= threshold``: a D8 ``FlowAccumulation`` result goes in as it is), or a ``DeviceRaster`` of
    uint8 or uint32.  ``cellsize``: a number or ``(dx, dy)``.  All arithmetic is float64 in a
    fixed order, rounded to float32 once: identical from run to run.

    ``ValueError`` for operands of another type, dtype or shape, an unknown ``kind`` or
    ``statistic``, a ``dem`` that is missing or (horizontal) not wanted, ``threshold`` without a
    uint32 raster, with a mask, or < 1, a ``cellsize`` that is not finite and positive (all
    before the device is touched), an invalid word, a receiver outside the raster, a cycle that
    holds no stop cell (only user-supplied words can form one) and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        stop_cells, unreached_cells (the NaN results), split_cells, terminal_cells, invalid,
        outside, unresolved, rounds and tile_visits (these two depend on the schedule), tile_h /
        tile_w of the last call; phase times when profiling is on.
    """

    auto_device = False     # the input is uint32 words, not a float32 raster

    def __init__(self, kind="horizontal", statistic="average", streams=None, threshold=None,
                 dem=None, cellsize=1.0):
        self.streams = _Given(streams, "streams", (np.bool_, np.uint8, np.uint32)).value
        self.dem = _Given(dem, "dem", (np.float32,)).value
        self.kind, self.statistic = kind, statistic
        self.threshold, self.cellsize = threshold, cellsize
        self.stats = {}
        # everything but the shapes: 1 x 1 stand-ins for the words and the operands
        _dinf.dinfdist_args(np.zeros((1, 1), np.uint32), _Given(self.streams).stand_in(),
                            threshold, _Given(self.dem).stand_in(), cellsize, kind, statistic)

    def _check(self, words):
        _dinf.dinfdist_args(words, self.streams, self.threshold, self.dem, self.cellsize,
                            self.kind, self.statistic)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._check(image_to_filter)
        out, self.stats = _dinf.dinfdist(
            image_to_filter, _Given(self.streams).host(), self.threshold,
            _Given(self.dem).host(), self.cellsize, self.kind, self.statistic)
        return out

    def apply_device(self, raster):
        self._check(raster)
        with _Given(self.streams).device(raster.ctx) as streams, \
                _Given(self.dem).device(raster.ctx) as dem:
            out, self.stats = _dinf.dinfdist_dev(raster, streams, self.threshold, dem,
                                                 self.cellsize, self.kind, self.statistic)
        return out


class DInfHeightAboveDrainage(DInfDistanceDown):  # pylint: disable=too-few-public-methods
    """D-infinity height above the nearest drainage (new operator): ``DInfDistanceDown`` with
    ``kind="vertical"`` and ``statistic="average"``.  Input: uint32 D-infinity words.  Returns
    float32: the drop from the cell to the stream cells its flow reaches, averaged over the flow
    proportions, and NaN where some of its flow ends without meeting a stream.

    ``dem``: float32 array or ``DeviceRaster`` of the words' shape; ``streams``, ``threshold``,
    ``cellsize``, the errors and ``stats`` as for ``DInfDistanceDown``."""

    def __init__(self, *, dem, streams, threshold=None, cellsize=1.0):
        if dem is None:
            raise ValueError("DInfHeightAboveDrainage needs the dem it is measured on")
        if streams is None:
            raise ValueError("DInfHeightAboveDrainage needs streams (a mask, or a uint32 raster "
                             "with a threshold)")
        super().__init__("vertical", "average", streams, threshold, dem, cellsize)


class DemToDInfHAND(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its D-infinity height above the nearest drainage in one device-resident
    chain, the way TauDEM users make HAND: ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one
    call, as in ``HydroConditioning``), ``FlowAccumulation`` on the D8 codes,
    ``DInfFlowDirection`` on the **filled** DEM with the codes as fallback, then the vertical
    ``DInfDistanceDown`` on the filled DEM down to the cells whose D8 accumulation is
    ``>= threshold``.  Nothing is downloaded in between.  ``flats`` as in ``DemToHAND``;
    ``statistic`` and ``cellsize`` as in ``DInfDistanceDown``.

    ``stats`` maps ``SinkFill``, ``FlowAccumulation``, ``DInfFlowDirection`` and
    ``DInfDistanceDown`` (and ``ResolveFlats``) to the stats of their stage.  With
    ``keep_partial_results=True`` the last call leaves ``filled``, ``codes``, ``accumulation``
    and ``words``: host arrays after ``apply``, device rasters (the caller's to free) after
    ``apply_device``; otherwise they are ``None``."""

    def __init__(self, *, threshold, epsilon=1e-3, flats="keep", cellsize=1.0,
                 statistic="average", keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the distance's operands, on stand-ins of the types the chain makes
        DInfDistanceDown("vertical", statistic, np.zeros((1, 1), np.uint32), threshold,
                         np.zeros((1, 1), np.float32), cellsize)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(), FlowAccumulation(),
                        DInfFlowDirection(cellsize=cellsize)]
        self.threshold, self.cellsize, self.statistic = threshold, cellsize, statistic
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.accumulation = self.words = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToDInfHAND", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "accumulation", "words")
                               if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToDInfHAND", raster, np.float32, "a float32 DEM")
        fill, _, accumulate, direct = self.filters
        self.filled = self.codes = self.accumulation = self.words = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            acc, accumulate.stats = backend.flowacc_dev(codes)
            stack.enter_context(acc)
            words, _, direct.stats = _dinf.dinf_dev(filled, self.cellsize, codes)
            stack.enter_context(words)
            hand, stats = _dinf.dinfdist_dev(words, acc, self.threshold, filled, self.cellsize,
                                             "vertical", self.statistic)
            self.stats = {"SinkFill": fill.stats, "FlowAccumulation": accumulate.stats,
                          "DInfFlowDirection": direct.stats, "DInfDistanceDown": stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.accumulation, self.words = filled, codes, acc, words
                stack.pop_all()                     # the caller's to free from here on
            return hand


class DInfDistanceUp(Filter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """D-infinity distance up to the ridge (new operator; TauDEM ``dinfdistup``).  Input: a
    uint32 H x W raster of D-infinity words as ``DInfFlowDirection`` returns them.  Returns
    float32: the distance from every cell up its D-infinity paths to the ridge.  A neighbour
    *counts* as a donor of a cell when it sends the cell at least ``min_proportion`` of its flow;
    a cell without such a neighbour is a ridge cell and reads 0.  A cell with one counted donor
    adds the step to the donor's distance; a cell with several combines the sums by ``statistic``.
    With ``DInfDistanceDown`` on the same words: hillslope length, and the slope position
    ``down / (down + up)``.

    ``kind``: ``"horizontal"`` (``dx`` / ``dy`` / the diagonal per step), ``"vertical"`` (the
    rise ``dem[donor] - dem[c]`` per step) or ``"surface"`` (``sqrt(h^2 + v^2)`` per step); the
    last two need ``dem``, a float32 array or ``DeviceRaster`` of the words' shape.
    ``statistic``: ``"average"`` weights the counted donors by the shares they send to the cell,
    normalised by their sum (this project's contract; not claimed to match TauDEM bit for bit);
    ``"minimum"`` and ``"maximum"`` are the shortest and the longest way.  ``min_proportion``: a
    number in (0, 1], 0.5 by default, compared as the integer ``min_share = max(1,
    ceil(min_proportion * 32768))``; ``min_share=`` gives that integer itself, 1 ... 32768, and
    not both.  ``cellsize``: a number or ``(dx, dy)``.  All arithmetic is float64 in a fixed
    order, rounded to float32 once: identical from run to run.

    ``ValueError`` for operands of another type, dtype or shape, an unknown ``kind`` or
    ``statistic``, a ``dem`` that is missing or (horizontal) not wanted, a ``min_proportion`` or
    ``min_share`` out of range or both of them, a ``cellsize`` that is not finite and positive
    (all before the device is touched), an invalid word, a receiver outside the raster, a cycle
    of counted links (only user-supplied words can form one) and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        ridge_cells, counted_links, ignored_links (below ``min_share``), merge_cells (more than
        one counted donor), nan_cells, invalid, outside, unresolved, rounds and tile_visits
        (these two depend on the schedule), tile_h / tile_w of the last call; phase times when
        profiling is on.
    """

    auto_device = False     # the input is uint32 words, not a float32 raster

    def __init__(self, kind="horizontal", statistic="average", dem=None, cellsize=1.0,
                 min_proportion=None, *, min_share=None):
        self.dem = _Given(dem, "dem", (np.float32,)).value
        self.kind, self.statistic, self.cellsize = kind, statistic, cellsize
        self.stats = {}
        # everything but the shapes: 1 x 1 stand-ins for the words and the dem
        self.min_share = _dinf.dinfdistup_args(
            np.zeros((1, 1), np.uint32), _Given(self.dem).stand_in(), cellsize, kind, statistic,
            min_proportion, min_share)[2]

    def _check(self, words):
        _dinf.dinfdistup_args(words, self.dem, self.cellsize, self.kind, self.statistic,
                              min_share=self.min_share)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self._check(image_to_filter)
        out, self.stats = _dinf.dinfdistup(
            image_to_filter, _Given(self.dem).host(), self.cellsize, self.kind, self.statistic,
            min_share=self.min_share)
        return out

    def apply_device(self, raster):
        self._check(raster)
        with _Given(self.dem).device(raster.ctx) as dem:
            out, self.stats = _dinf.dinfdistup_dev(raster, dem, self.cellsize, self.kind,
                                                   self.statistic, min_share=self.min_share)
        return out


class DemToDInfDistanceUp(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its D-infinity distance up to the ridge in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``DInfFlowDirection`` on the **filled** DEM with the codes as fallback, then
    ``DInfDistanceUp``, the vertical and surface kinds on the filled DEM.  Nothing is downloaded
    in between.  ``flats`` as in ``DemToHAND``; ``kind``, ``statistic``, ``min_proportion`` /
    ``min_share`` and ``cellsize`` as in ``DInfDistanceUp``.

    ``stats`` maps ``SinkFill``, ``DInfFlowDirection`` and ``DInfDistanceUp`` (and
    ``ResolveFlats``) to the stats of their stage.  With ``keep_partial_results=True`` the last
    call leaves ``filled``, ``codes`` and ``words``: host arrays after ``apply``, device rasters
    (the caller's to free) after ``apply_device``; otherwise they are ``None``."""

    def __init__(self, *, kind="horizontal", statistic="average", min_proportion=None,
                 min_share=None, epsilon=1e-3, flats="keep", cellsize=1.0,
                 keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the distance's operands, on a stand-in of the dem the chain makes
        stand_in = None if kind == "horizontal" else np.zeros((1, 1), np.float32)
        self.min_share = DInfDistanceUp(kind, statistic, stand_in, cellsize, min_proportion,
                                        min_share=min_share).min_share
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(),
                        DInfFlowDirection(cellsize=cellsize)]
        self.kind, self.statistic, self.cellsize = kind, statistic, cellsize
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.words = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToDInfDistanceUp", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "words") if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToDInfDistanceUp", raster, np.float32, "a float32 DEM")
        fill, _, direct = self.filters
        self.filled = self.codes = self.words = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            words, _, direct.stats = _dinf.dinf_dev(filled, self.cellsize, codes)
            stack.enter_context(words)
            up, stats = _dinf.dinfdistup_dev(
                words, None if self.kind == "horizontal" else filled, self.cellsize, self.kind,
                self.statistic, min_share=self.min_share)
            self.stats = {"SinkFill": fill.stats, "DInfFlowDirection": direct.stats,
                          "DInfDistanceUp": stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.words = filled, codes, words
                stack.pop_all()                     # the caller's to free from here on
            return up


class MFDFlowDirection(Filter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """Multiple-flow-direction flow direction (new operator; Quinn 1991, Freeman 1991, Holmgren
    1994; Whitebox ``FD8FlowAccumulation``, SAGA "MFD").  Input: a float32 H x W DEM, NaN where
    there is no data.  Returns one uint64 word per cell (``hydrodem_amd.mfd``): a cell sends
    flow to every lower neighbour in proportion to ``c * (slope / steepest slope) ** exponent``,
    ``c`` being ``w_card`` for the four cardinal and ``w_diag`` for the four diagonal
    neighbours; the shares are quantised to 2^-8 and the steepest-weighted receiver takes the
    rest.  The slopes are float64 on the float32 elevations, the power is the contract's own
    (no math library), so the words are the same bits everywhere.  Cells without a lower
    neighbour, NaN cells and infinite ones get 0: no outflow.  Cells on the raster's edge route
    like any other, among the neighbours they have.

    ``method``: ``"freeman"`` (exponent 1.1), ``"quinn"`` (exponent 1, contour-length weights
    0.5 and 0.354), ``"holmgren"`` with the caller's ``exponent`` (0.25 ... 16), or an
    ``(exponent, w_card, w_diag)`` triple.  ``cellsize``: a number or ``(dx, dy)``.
    ``fallback``: uint8 ESRI D8 codes of the DEM's shape (array or ``DeviceRaster``); a cell that
    would get 0 takes its code's direction, so that the flats of an exact fill routed by
    ``ResolveFlats`` keep draining.  With ``keep_partial_results=True`` the launch also writes
    ``slope`` (float32: the steepest downward slope, 0 where there is none, NaN at NaN; what
    ``AreaWetnessIndex`` takes as ``given_slope``) and leaves it in the attribute of that name:
    a host array after ``apply``, a device raster (the caller's to free) after ``apply_device``.

    ``ValueError`` for a dtype other than float32, a raster that is not 2-D, an unknown
    ``method``, an ``exponent`` out of range, a ``cellsize`` that is not finite and positive, a
    ``fallback`` of another type, dtype or shape (all before the device is touched) and a
    fallback byte that is no D8 code.

    Attributes
    ----------
    stats : dict
        no_flow (cells with word 0), fallback_cells, split_cells (cells with more than one
        receiver) of the last call; ms_total when profiling.
    """

    auto_device = False     # words are uint64: no float32 chain goes on from them

    def __init__(self, method="freeman", exponent=None, cellsize=1.0, fallback=None,
                 keep_partial_results=False):
        self.method, self.exponent, self.cellsize = method, exponent, cellsize
        self.fallback = _Given(fallback, "fallback", (np.uint8,)).value
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.slope = None
        _mfd.mfd_args(np.zeros((1, 1), np.float32), method, exponent, cellsize,
                      _Given(self.fallback).stand_in())

    def _want(self):
        return _mfd.EXTRAS if self.keep_partial_results else ()

    def _keep(self, words, extras, stats):
        self.stats = stats
        self.slope = extras.get("slope")
        return words

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _mfd.mfd_args(image_to_filter, self.method, self.exponent, self.cellsize, self.fallback)
        return self._keep(*_mfd.mfd(image_to_filter, self.method, self.exponent, self.cellsize,
                                    _Given(self.fallback).host(), self._want()))

    def apply_device(self, raster):
        _mfd.mfd_args(raster, self.method, self.exponent, self.cellsize, self.fallback)
        with _Given(self.fallback).device(raster.ctx) as fallback:
            return self._keep(*_mfd.mfd_dev(raster, self.method, self.exponent, self.cellsize,
                                            fallback, self._want()))


class MFDFlowAccumulation(Filter):  # pylint: disable=too-few-public-methods
    """Multiple-flow-direction flow accumulation (new operator).  Input: a uint64 H x W raster of
    MFD words as ``MFDFlowDirection`` returns them.  ``A[c] = own(c)`` plus what the
    8-neighbours whose word names ``c`` send it: a donor with amount ``A`` sends
    ``(A * p) >> 8`` along each share ``p`` and the rest to its main receiver.  ``own`` is
    ``2^frac_bits`` (``frac_bits`` 0 ... 16), or with ``weights`` (an H x W NumPy array or
    ``DeviceRaster`` of uint8, uint32 or float32) the weight quantised as
    ``WeightedDInfFlowAccumulation`` does (``frac_bits`` 0 ... 30 for float32).  Integers
    throughout: every unit arrives at a cell without outflow, and the result is identical from
    run to run.

    ``output``: ``"value"`` float32 ``float32(float64(A) * 2^-frac_bits)``; ``"sum"`` int64
    ``A``.

    ``ValueError`` for operands of another type, dtype or shape, ``frac_bits`` out of range, an
    unknown ``output`` (all before the device is touched), an invalid word, a receiver outside
    the raster, words that form a cycle (only user-supplied words can), weights that
    ``WeightedDInfFlowAccumulation`` refuses and more than 2^32 - 1 cells.

    Attributes
    ----------
    stats : dict
        split_cells (cells with more than one receiver), terminal_cells, invalid, outside,
        unresolved, rounds and tile_visits (these two depend on the schedule), tile_h / tile_w,
        nan_weights, bad_weights and total of the last call; phase times when profiling is on.
    """

    auto_device = False     # the input is uint64 words, not a float32 raster
    WEIGHT_TYPES = (np.uint8, np.uint32, np.float32)
    OUTPUTS = {name: np.dtype(dtype) for name, dtype in _mfd.OUTPUTS}

    def __init__(self, frac_bits=16, output="value", weights=None):
        self.weights = _Given(weights, "weights", self.WEIGHT_TYPES).value
        if not isinstance(output, str) or output not in self.OUTPUTS:
            raise ValueError(f"output is one of {list(self.OUTPUTS)}, got {output!r}")
        self.frac_bits, self.output = frac_bits, output
        self.dtype = self.OUTPUTS[output]
        self.stats = {}
        # everything but the shapes, on 1 x 1 stand-ins
        _mfd.mfdacc_args(np.empty((1, 1), np.uint64), _Given(self.weights).stand_in(),
                         frac_bits, output)

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _mfd.mfdacc_args(image_to_filter, self.weights, self.frac_bits, self.output)
        outs, self.stats = _mfd.mfdacc(image_to_filter, _Given(self.weights).host(),
                                       self.frac_bits, self.output)
        return outs[self.output]

    def apply_device(self, raster):
        _mfd.mfdacc_args(raster, self.weights, self.frac_bits, self.output)
        with _Given(self.weights).device(raster.ctx) as weights:
            outs, self.stats = _mfd.mfdacc_dev(raster, weights, self.frac_bits, self.output)
        return outs[self.output]


class DemToMFDArea(ComposedFilter):  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """A float32 DEM to its multiple-flow-direction catchment area in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``MFDFlowDirection`` on the **filled** DEM with the chain's D8 codes as fallback, then
    ``MFDFlowAccumulation``.  Nothing is downloaded in between.  ``flats`` as in ``DemToHAND``:
    with ``"resolve"`` the fallback codes cross the flats, so an exact fill (``epsilon=0``)
    drains; ``method``, ``exponent``, ``cellsize``, ``frac_bits`` and ``output`` as in the two
    operators.

    ``stats`` maps ``SinkFill``, ``MFDFlowDirection`` and ``MFDFlowAccumulation`` (and
    ``ResolveFlats``) to the stats of their stage.  With ``keep_partial_results=True`` the last
    call leaves ``filled``, ``codes`` and ``words``: host arrays after ``apply``, device rasters
    (the caller's to free) after ``apply_device``; otherwise they are ``None``."""

    def __init__(self, *, epsilon=1e-3, flats="keep", method="freeman", exponent=None,
                 cellsize=1.0, frac_bits=16, output="value", keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(),
                        MFDFlowDirection(method=method, exponent=exponent, cellsize=cellsize),
                        MFDFlowAccumulation(frac_bits=frac_bits, output=output)]
        self.method, self.exponent, self.cellsize = method, exponent, cellsize
        self.frac_bits, self.output = frac_bits, output
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.filled = self.codes = self.words = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToMFDArea", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter,
                               ("filled", "codes", "words") if self.keep_partial_results else ())

    def apply_device(self, raster):
        _check_raster("DemToMFDArea", raster, np.float32, "a float32 DEM")
        fill, _, direct, accumulate = self.filters
        self.filled = self.codes = self.words = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            words, _, direct.stats = _mfd.mfd_dev(filled, self.method, self.exponent,
                                                  self.cellsize, codes)
            stack.enter_context(words)
            outs, accumulate.stats = _mfd.mfdacc_dev(words, None, self.frac_bits, self.output)
            self.stats = {"SinkFill": fill.stats, "MFDFlowDirection": direct.stats,
                          "MFDFlowAccumulation": accumulate.stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.filled, self.codes, self.words = filled, codes, words
                stack.pop_all()                     # the caller's to free from here on
            return outs[self.output]


class DemToStreamOrder(ComposedFilter):  # pylint: disable=too-few-public-methods
    """A float32 DEM to the Strahler order (or the Shreve magnitude) of its streams in one
    device-resident chain: ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in
    ``HydroConditioning``), ``FlowAccumulation``, then ``StreamOrder`` with streams where the
    accumulation is ``>= threshold``.  Nothing is downloaded in between.

    ``stats`` maps ``SinkFill``, ``FlowAccumulation`` and ``StreamOrder`` to the stats of their
    stage (``ResolveFlats`` too with ``flats="resolve"``, which runs that stage between the D8
    and the accumulation as in ``DemToHAND``).  With ``keep_partial_results=True`` the last
    call leaves ``codes``, ``accumulation``, ``order``, ``magnitude`` and ``links``: host arrays
    after ``apply``, device rasters (the caller's to free; the one returned is among them) after
    ``apply_device``; otherwise they are ``None``."""

    KEPT = ("codes", "accumulation", "order", "magnitude", "links")

    def __init__(self, *, threshold, epsilon=1e-3, flats="keep", method="strahler",
                 keep_partial_results=False):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the order's operands, on a stand-in of the type the chain makes
        StreamOrder(np.zeros((1, 1), np.uint32), threshold=threshold, method=method)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(), FlowAccumulation()]
        self.threshold, self.method = threshold, method
        self.keep_partial_results = keep_partial_results
        self.stats = {}
        self.codes = self.accumulation = self.order = self.magnitude = self.links = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToStreamOrder", image_to_filter, np.float32, "a float32 DEM")
        with backend.DeviceRaster.from_host(image_to_filter, dtype=np.float32) as z, \
                contextlib.ExitStack() as stack:
            result = stack.enter_context(self.apply_device(z))
            out = result.to_host()
            for name in self.KEPT if self.keep_partial_results else ():
                raster = stack.enter_context(getattr(self, name))
                setattr(self, name, out if raster is result else raster.to_host())
        return out

    def apply_device(self, raster):
        _check_raster("DemToStreamOrder", raster, np.float32, "a float32 DEM")
        fill, _, accumulate = self.filters
        self.codes = self.accumulation = self.order = self.magnitude = self.links = None
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            acc, accumulate.stats = backend.flowacc_dev(codes)
            stack.enter_context(acc)
            order = StreamOrder(acc, threshold=self.threshold, method=self.method,
                                keep_partial_results=self.keep_partial_results)
            out = order.apply_device(codes)
            self.stats = {"SinkFill": fill.stats, "FlowAccumulation": accumulate.stats,
                          "StreamOrder": order.stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            if self.keep_partial_results:
                self.codes, self.accumulation = codes, acc
                self.order, self.magnitude, self.links = order.order, order.magnitude, order.links
                stack.pop_all()                     # the caller's to free from here on ...
                filled.free()                       # ... but for the filled DEM
            return out


class DemToStreamNetwork(ComposedFilter):  # pylint: disable=too-few-public-methods
    """A float32 DEM to the table of its stream network in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``FlowAccumulation``, then ``StreamNetwork`` with streams where the accumulation is
    ``>= threshold`` and the **filled** DEM for the elevation columns, so that ``z_top >= z_end``
    on every link.  Nothing is downloaded in between.

    Returns the ``row`` raster as ``StreamNetwork`` does and leaves ``table`` and ``count``;
    ``stats`` maps ``SinkFill``, ``FlowAccumulation`` and ``StreamNetwork`` to the stats of their
    stage (``ResolveFlats`` too with ``flats="resolve"``, which runs that stage between the D8
    and the accumulation as in ``DemToHAND``)."""

    def __init__(self, threshold, *, epsilon=1e-3, flats="keep", cellsize=1.0, columns=None):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the table's operands, on stand-ins of the types the chain makes
        StreamNetwork(np.zeros((1, 1), np.uint32), threshold=threshold,
                      dem=np.zeros((1, 1), np.float32), cellsize=cellsize, columns=columns)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(), FlowAccumulation()]
        self.threshold, self.cellsize, self.columns = threshold, cellsize, columns
        self.stats = {}
        self.table, self.count = None, 0

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToStreamNetwork", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter)

    def apply_device(self, raster):
        _check_raster("DemToStreamNetwork", raster, np.float32, "a float32 DEM")
        fill, _, accumulate = self.filters
        with contextlib.ExitStack() as stack:
            filled, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            acc, accumulate.stats = backend.flowacc_dev(codes)
            stack.enter_context(acc)
            network = StreamNetwork(acc, threshold=self.threshold, dem=filled,
                                    cellsize=self.cellsize, columns=self.columns)
            row = network.apply_device(codes)
            self.table, self.count = network.table, network.count
            self.stats = {"SinkFill": fill.stats, "FlowAccumulation": accumulate.stats,
                          "StreamNetwork": network.stats}
            if resolve_stats is not None:
                self.stats["ResolveFlats"] = resolve_stats
            return row


class DemToBasins(ComposedFilter):  # pylint: disable=too-few-public-methods
    """A float32 DEM to the table of its drainage basins in one device-resident chain:
    ``SinkFill(epsilon)`` and ``D8FlowDirection`` (one call, as in ``HydroConditioning``),
    ``Watersheds(labels="compact")``, then ``ZonalStatistics`` of the labels with the DEM itself
    as values: per basin its area, bounding box, lowest and highest point and where they are,
    and the sum behind its mean elevation.  Nothing is downloaded in between.

    Returns the compact labels as ``Watersheds`` does and leaves ``table`` and ``count``; the
    table carries one more column, ``outlet`` (the flat index of the basin's terminal cell:
    label ``k`` is row ``k - 1``).  ``stats`` maps ``SinkFill``, ``Watersheds`` and
    ``ZonalStatistics`` to the stats of their stage (``ResolveFlats`` too with
    ``flats="resolve"``, which runs that stage behind the D8 as in ``DemToHAND``)."""

    def __init__(self, *, epsilon=1e-3, flats="keep", columns=None, frac_bits=16):
        super().__init__()
        self.flats = _check_flats(flats)
        # the checks of the table's operands, on a stand-in of the type the chain is given
        ZonalStatistics(np.zeros((1, 1), np.float32), columns, frac_bits)
        self.filters = [SinkFill(epsilon=epsilon), D8FlowDirection(),
                        Watersheds(labels="compact")]
        self.columns, self.frac_bits = columns, frac_bits
        self.stats = {}
        self.table, self.count = None, 0

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        _check_raster("DemToBasins", image_to_filter, np.float32, "a float32 DEM")
        return _through_device(self, image_to_filter)

    def apply_device(self, raster):
        _check_raster("DemToBasins", raster, np.float32, "a float32 DEM")
        fill, _, basins = self.filters
        with contextlib.ExitStack() as stack:
            _, codes, resolve_stats = _fill_d8(stack, raster, fill, self.flats)
            with backend.result_raster(None, raster.shape, np.uint32, raster.ctx) as labels:
                _, outlets, basins.stats = backend.watershed_dev(codes, None, True, out=labels)
                zonal = ZonalStatistics(raster, self.columns, self.frac_bits)
                self.table = dict(zonal.apply_device(labels), outlet=outlets.copy())
                self.count = zonal.stats["zones"]
                self.stats = {"SinkFill": fill.stats, "Watersheds": basins.stats,
                              "ZonalStatistics": zonal.stats}
                if resolve_stats is not None:
                    self.stats["ResolveFlats"] = resolve_stats
            return labels


# ---------------------------------------------------------------------------
# Fourier destripe
# ---------------------------------------------------------------------------
class ExpandFilter(Filter):  # pylint: disable=too-few-public-methods
    """1 at the centres whose ``window_size`` square minus its four corners holds a
    cell > 0, 0 elsewhere -- including the ring of ``window_size // 2`` cells where
    the window does not fit (custom_filters.py:76-125)."""

    def __init__(self, *, window_size):
        self.window_size = window_size

    def apply(self, image_to_filter):
        return backend.expand(image_to_filter, self.window_size, np.float64)


class IsolatedPoints(Filter):  # pylint: disable=too-few-public-methods
    """Cells equal to 1 with no other cell > 0 in their window become 0; like the
    reference (custom_filters.py:320-366) this writes into its input and returns
    it.  Only centres whose window fits are looked at."""

    def __init__(self, *, window_size):
        self.window_size = window_size

    def apply(self, image_to_filter):
        img = image_to_filter
        g = np.asarray(img, dtype=np.float32)                # the window snapshot
        ones = np.trunc(g) == 1
        code = np.where(ones, 1, np.where(g > 0, 2, 0)).astype(np.uint8)
        res = backend.isolated_points(code, self.window_size)
        r = self.window_size // 2
        inner = np.zeros(g.shape, dtype=bool)
        inner[r:g.shape[0] - r, r:g.shape[1] - r] = True
        sel = ones & inner
        img[sel] = res[sel].astype(img.dtype)
        return img


class BlanksFourier(Filter):  # pylint: disable=too-few-public-methods
    """Peaks of a spectrum magnitude: cells above 4x the mean of their 55 x 55
    neighbourhood, its inner 5 x 5 and everything past the array edge left out.
    Returns (mask, image with the peaks zeroed) (custom_filters.py:369-429).
    Any odd window from 7 to 201; 55, the one the reference's pipeline uses, has a
    kernel instance of its own."""

    def __init__(self, *, window_size):
        self.window_size = window_size

    def apply(self, image_to_filter):
        return backend.blanks_fourier(image_to_filter, self.window_size)


class DetectBlanksFourier(Filter):  # pylint: disable=too-few-public-methods
    """Two ``BlanksFourier`` passes, the second on the image without the first
    pass's peaks; the masks are added (custom_filters.py:432-462)."""

    def apply(self, quarter_fourier):
        total = np.zeros(np.shape(quarter_fourier))
        blanks = BlanksFourier(window_size=55)
        for _ in (0, 1):
            found, quarter_fourier = blanks.apply(quarter_fourier)
            total += found
        return total


class MaskFourier(ComposedFilter):  # pylint: disable=too-few-public-methods
    """detect -> drop isolated points -> expand (custom_filters.py:537-561)."""

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [DetectBlanksFourier(), IsolatedPoints(window_size=3),
                        ExpandFilter(window_size=13)]


class FourierInitial(ComposedFilterResults):  # pylint: disable=too-few-public-methods
    """fft2 -> fftshift -> abs; keeps the shifted spectrum
    (custom_filters.py:834-877)."""

    def __init__(self):
        super().__init__()
        self.filters = [FourierTransform(), FourierShift(), AbsoluteValues()]
        self.fourier_shift = None

    def apply(self, image_to_filter):
        result = super().apply(image_to_filter)
        self.fourier_shift = self.results["FourierShift"]
        return result


class FourierProcessQuarters(Filter):  # pylint: disable=too-few-public-methods
    """Mask of the frequencies to drop, from the magnitude of the shifted
    spectrum: ``MaskFourier`` on the two upper quadrants (10-cell margin to the
    axes), point-mirrored into the lower half (custom_filters.py:880-1050).
    ``apply`` ignores its argument, as the reference does."""

    def __init__(self, fft_transform_abs):
        self.fft_transform_abs = fft_transform_abs
        self._ny, self._nx = fft_transform_abs.shape
        self._mid_y, self._y_odd = divmod(self._ny, 2)
        self._mid_x, self._x_odd = divmod(self._nx, 2)
        self.pair_mid = self._mid_y, self._mid_x
        self._margin = 10

    def apply(self, image_to_filter):  # pylint: disable=unused-argument
        ny, nx, my, mx, m = self._ny, self._nx, self._mid_y, self._mid_x, self._margin
        mag = self.fft_transform_abs
        first = MaskFourier().apply(np.array(mag[:my - m, :mx - m]))
        second = MaskFourier().apply(np.array(mag[:my - m, mx + m + self._x_odd:nx]))
        q1 = np.zeros(self.pair_mid)
        q2 = np.zeros(self.pair_mid)
        q1[:my - m, :mx - m] = first
        q2[:my - m, m:mx] = second
        full = np.zeros((ny, nx))
        full[:my, :mx] = q1
        full[:my, mx + self._x_odd:] = q2
        full[my + self._y_odd:, :mx] = q2[::-1, ::-1]
        full[my + self._y_odd:, mx + self._x_odd:] = q1[::-1, ::-1]
        return full


class DetectApplyFourier(ComposedFilter):  # pylint: disable=too-few-public-methods
    """Destripe: find the bright isolated frequencies of the spectrum, zero them,
    transform back (custom_filters.py:1053-1101).  One device-resident pass
    (``hdem_fourier_destripe_f32``): the shifts are index maps, the quadrant masks
    are applied straight to the spectrum.  Returns float32 (the reference: float64
    from a complex128 inverse; values agree to ~1e-5 m).  With
    ``keep_mask=True`` the full mask is kept in ``.mask`` afterwards."""

    auto_device = True      # device form == host form for a float32 raster

    def __init__(self, keep_mask=False):  # pylint: disable=super-init-not-called
        self.initial = FourierInitial()
        self.fft_transform_abs = None
        self.keep_mask = keep_mask
        self.mask = None
        self.filters = []

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        if self.keep_mask:
            out, mask = backend.fourier_destripe(image_to_filter, return_mask=True)
            self.mask = mask.astype(np.float64)
            return out
        return backend.fourier_destripe(image_to_filter)

    def apply_device(self, raster):
        return backend.fourier_destripe_dev(raster)


# ---------------------------------------------------------------------------
# HydroSHEDS / lagoon branch
# ---------------------------------------------------------------------------
def _write_back_repaired(image, uploaded, fixed, window_size):
    """``CorrectNANValues`` works in place: ``fixed``, the repair of ``uploaded`` (``image`` as
    contiguous float32), goes back into ``image``.  The kernel passes every other cell through
    bit for bit, so an ``image`` that went up as it is receives the repaired raster whole; any
    other only its repaired cells, the voids inside the ring of ``window_size // 2`` cells
    (its other values need not be float32 numbers)."""
    if uploaded is image:
        fixed.to_host(out=image)
        return
    r = int(window_size) // 2
    sel = uploaded < 0
    sel[:r] = sel[uploaded.shape[0] - r:] = False
    sel[:, :r] = sel[:, uploaded.shape[1] - r:] = False
    np.copyto(image, fixed.to_host(), where=sel, casting="unsafe")


class MajorityFilter(Filter):  # pylint: disable=too-few-public-methods
    """The value that fills more than 70 % of ``window_size**2 - 1`` cells of the
    circular window (square minus corners, the centre counts), else 0; the ring
    where the window does not fit stays 0 (custom_filters.py:22-73)."""

    def __init__(self, *, window_size):
        self.window_size = window_size

    def apply(self, image_to_filter):
        with backend.DeviceRaster.from_host(image_to_filter, dtype=np.float32) as img, \
                backend.majority_dev(img, self.window_size) as out:
            return backend.widened_to_host(out, np.float64)

    def apply_device(self, raster):
        return backend.majority_dev(raster, self.window_size)


class CorrectNANValues(Filter):  # pylint: disable=too-few-public-methods
    """Voids (cells < 0) become the mean of their non-negative neighbours; like the
    reference (custom_filters.py:260-317) this writes into its input and returns
    it.  Odd windows 3 to 11 (the reference's pipeline uses 3)."""

    def __init__(self, *, window_size=3):
        self.window_size = window_size

    def apply(self, image_to_filter):
        g = np.ascontiguousarray(image_to_filter, dtype=np.float32)
        with backend.DeviceRaster.from_host(g) as dem, \
                backend.correct_nan_dev(dem, window_size=self.window_size) as fixed:
            _write_back_repaired(image_to_filter, g, fixed, self.window_size)
        return image_to_filter

    def apply_device(self, raster):
        return backend.correct_nan_dev(raster, window_size=self.window_size)


class MaskNegatives(ComposedFilter):  # pylint: disable=too-few-public-methods
    """1 where the image is negative (custom_filters.py:465-487)."""

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [LowerThan(value=0.0), BooleanToInteger()]


class MaskPositives(ComposedFilter):  # pylint: disable=too-few-public-methods
    """1 where the image is positive (custom_filters.py:490-510)."""

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [GreaterThan(value=0.0), BooleanToInteger()]


class TidyingLagoons(ComposedFilter):  # pylint: disable=too-few-public-methods
    """Erode twice, expand by 7, multiply with the input, 7 x 7 grey dilation
    (custom_filters.py:564-610).  ``apply`` runs the four steps in one
    device-resident call when the list is the stock one; ``filters`` stays
    inspectable and patchable like the reference's."""

    def __init__(self):  # pylint: disable=super-init-not-called
        self.filters = [BinaryErosion(iterations=2), ExpandFilter(window_size=7),
                        ProductFilter(), GreyDilation(size=(7, 7))]

    def _stock(self):
        f = self.filters
        return (len(f) == 4 and isinstance(f[0], BinaryErosion) and f[0].iterations == 2 and
                isinstance(f[1], ExpandFilter) and f[1].window_size == 7 and
                isinstance(f[2], ProductFilter) and isinstance(f[3], GreyDilation) and
                tuple(np.atleast_1d(f[3].size)) in ((7, 7), (7,)))

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        self.filters[2].factor = content = image_to_filter
        if self._stock():
            with backend.DeviceRaster.from_host(image_to_filter, dtype=np.float32) as img, \
                    backend.tidying_lagoons_dev(img) as out:
                return backend.widened_to_host(out, np.float64)
        for filter_ in self.filters:
            content = filter_.apply(content)
        return content

    def apply_device(self, raster):
        return backend.tidying_lagoons_dev(raster)


class LagoonsDetection(ComposedFilterResults):  # pylint: disable=too-few-public-methods
    """NaN repair -> majority (11) -> tidying -> mask of positives, keeping the
    intermediate results the orchestration reads (custom_filters.py:613-661).
    One device-resident call (``hdem_lagoons_detection_f32_dev``); like the
    reference the void repair is also written into the input array."""

    def __init__(self):
        super().__init__()
        self.filters = [CorrectNANValues(), MajorityFilter(window_size=11),
                        TidyingLagoons(), MaskPositives()]
        self.hsheds_nan_fixed = None
        self.mask_lagoons = None
        self.lagoons_values = None

    def apply(self, image_to_filter):
        Filter.apply(self, image_to_filter)
        g = np.ascontiguousarray(image_to_filter, dtype=np.float32)
        with backend.DeviceRaster.from_host(g) as hsheds, contextlib.ExitStack() as stack:
            mask, fixed, values = map(stack.enter_context, backend.lagoons_detection_dev(hsheds))
            _write_back_repaired(image_to_filter, g, fixed, 3)
            self.hsheds_nan_fixed = image_to_filter
            self.lagoons_values = backend.widened_to_host(values, np.float64)
            self.mask_lagoons = backend.widened_to_host(mask, np.int64)
        self.results = {"CorrectNANValues": self.hsheds_nan_fixed,
                        "TidyingLagoons": self.lagoons_values,
                        "MaskPositives": self.mask_lagoons}
        return self.mask_lagoons


# ---------------------------------------------------------------------------
# River branch (host side; SURVEY section 2 #9: serial by construction)
# ---------------------------------------------------------------------------
class RouteRivers(Filter):  # pylint: disable=too-few-public-methods
    """Route a river mask downhill on a reference DEM
    (custom_filters.py:128-199).

    Every cell of the mask whose value truncates to 1 and whose
    ``window_size`` window fits is visited in raster order; all cells of its
    DEM window that hold the window minimum become river and are then raised
    to 10000 in the working copy of the DEM, so a later window sees the
    earlier ones' marks -- the one Gauss-Seidel stencil of the reference, and
    the reason it stays on the host.  The DEM is deep-copied at construction
    (`:163`) and read as float32 (`sliding_window.py:132`); a window holding a
    NaN marks nothing (``window == nan`` is never true).  Returns float64."""

    def __init__(self, *, window_size, dem):
        self.window_size = window_size
        self.dem = copy.deepcopy(dem)

    def apply(self, image_to_filter):
        mask = SlidingWindow(image_to_filter, window_size=self.window_size)
        work = SlidingWindow(self.dem, window_size=self.window_size).grid
        reach = self.window_size // 2
        routed = np.zeros(self.dem.shape)
        height, width = mask.grid.shape
        inner = mask.grid[reach:height - reach, reach:width - reach]
        rows, cols = np.nonzero(np.trunc(inner) == 1)           # raster order
        for row, col in zip(rows.tolist(), cols.tolist()):
            window = work[row:row + 2 * reach + 1, col:col + 2 * reach + 1]
            lowest = window == np.amin(window)
            routed[row:row + 2 * reach + 1, col:col + 2 * reach + 1][lowest] = 1
            window[lowest] = 10000
        return routed


class ProcessRivers(ComposedFilter):  # pylint: disable=too-few-public-methods
    """Mask of positives -> expand by 3 -> route on the HydroSHEDS DEM ->
    binary closing (custom_filters.py:770-798)."""

    def __init__(self, hsheds):  # pylint: disable=super-init-not-called
        self.filters = [MaskPositives(), ExpandFilter(window_size=3),
                        RouteRivers(window_size=3, dem=hsheds), BinaryClosing()]


class ClipLagoonsRivers(ComposedFilter):  # pylint: disable=too-few-public-methods
    """Rivers minus their intersection with the lagoons: ``rivers XOR
    (mask_lagoons * rivers)`` (custom_filters.py:801-831)."""

    def __init__(self, mask_lagoons, rivers_routed_closing):  # pylint: disable=super-init-not-called
        self.filters = [ProductFilter(factor=mask_lagoons),
                        BitwiseXOR(operand=rivers_routed_closing)]
