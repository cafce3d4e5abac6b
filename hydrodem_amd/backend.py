"""
ctypes binding of ``libhydrodem_hip.so`` (C ABI: ``include/hydrodem_hip.h``).

This is the whole host side of the boundary: load the library, map status
codes to the reference's exception classes, and move NumPy arrays across.
There is deliberately no CPU implementation behind it -- when the library or
a GPU is missing every operator raises :class:`BackendError`.
"""

import contextlib
import ctypes
import importlib.util
import os
import sys
import threading
import weakref

import numpy as np

from .exceptions import (BackendError, HydroDEMException, NotConvergedError,
                         WindowSizeEvenError, WindowSizeHighError)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhydrodem_hip.so")

# status codes (include/hydrodem_hip.h)
OK, BAD_ARG, WINDOW_EVEN, WINDOW_HIGH, HIP_ERR, NOT_CONVERGED, NO_DEVICE, OOM = range(8)

# kernel ids for the timing query
K_D8, K_FILL_INIT, K_FILL_TILE, K_BOXMEAN, K_GROVES, K_CONVOLVE, K_COPY, K_FILL_ROUND = range(8)
K_BLOCKMAX, K_FFT, K_FOURIER_ROWSUM, K_FOURIER_DETECT, K_FOURIER_MASK, K_FOURIER_POINT = range(8, 14)
K_LAGOON, K_MAJORITY, K_FILL_COARSE, K_FILL_FLAT, K_ELEMENTWISE = 14, 15, 16, 17, 18
K_FILL_HUB = 19
K_FLOWACC = 20

# element-wise operators and raster types of hdem_elementwise_dev
EW_MUL, EW_ADD, EW_RSUB, EW_GT, EW_LT, EW_NONZERO = range(6)
_EW_TYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2,
             np.dtype(np.int64): 3}

FILL_INIT, FILL_WARM, FILL_ACT_TOP, FILL_ACT_BOTTOM = 0, 1, 2, 4
FILL_GHOST_TOP, FILL_GHOST_BOTTOM, FILL_SYNC_ONLY, FILL_NO_VERIFY = 0x10, 0x20, 0x40, 0x80
FILL_RESUME, FILL_GHOST_GIVEN, FILL_NO_COARSE = 0x100, 0x200, 0x400
FILL_DEFER = 0x800


class KernelStat(ctypes.Structure):
    _fields_ = [("launches", ctypes.c_int64), ("ms", ctypes.c_double),
                ("units", ctypes.c_int64)]


class _Stats(ctypes.Structure):
    """What the stats structs of the C ABI share: their fields as a dict."""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_
                if k not in ("struct_size", "reserved")}


class _SizedStats(_Stats):
    """A stats struct that opens with ``struct_size``, set on construction as the C ABI asks."""

    def __init__(self):
        super().__init__()
        self.struct_size = ctypes.sizeof(self)


class FillStats(_Stats):
    _fields_ = [("rounds", ctypes.c_int32), ("converged", ctypes.c_int32),
                ("tile_visits", ctypes.c_int64), ("tiles", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("visits_flat", ctypes.c_int32), ("async_timed_out", ctypes.c_int32),
                ("iterations", ctypes.c_int64), ("visits_unchanged", ctypes.c_int64),
                ("visits_requeued", ctypes.c_int64), ("round_visits", ctypes.c_int64),
                ("pending", ctypes.c_int64), ("partial_residency", ctypes.c_int32),
                ("flat_unchanged", ctypes.c_int32),
                ("deferred_visits", ctypes.c_int64), ("deferred_unchanged", ctypes.c_int64)]


class FlowAccStats(_Stats):
    _fields_ = [("exits", ctypes.c_int64), ("max_hops", ctypes.c_int32),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float)]


class WatershedStats(_SizedStats):
    """``hdem_watershed_stats``."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("forest_rounds", ctypes.c_int32),
                ("basins", ctypes.c_int64), ("exits", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


WS_COMPACT = 1      # HDEM_WS_COMPACT


class FlowTraceStats(_SizedStats):
    """``hdem_flowtrace_stats``."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("forest_rounds", ctypes.c_int32),
                ("stops", ctypes.c_int64), ("unreached", ctypes.c_int64),
                ("exits", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class ResolveFlatsStats(_SizedStats):
    """``hdem_resolve_flats_stats``."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("rounds", ctypes.c_int32),
                ("flat_cells", ctypes.c_int64), ("unresolved", ctypes.c_int64),
                ("tile_visits", ctypes.c_int64), ("max_distance", ctypes.c_uint32),
                ("active_tiles", ctypes.c_int32),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_classify", ctypes.c_float), ("ms_relax", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class DepressionsStats(_SizedStats):
    """``hdem_depressions_stats``."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_int32),
                ("depressions", ctypes.c_int64), ("raised_cells", ctypes.c_int64),
                ("tile_components", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_seam", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved2", ctypes.c_int32)]

    def as_dict(self):
        fields = super().as_dict()
        del fields["reserved2"]
        return fields


class _UpstreamStats(_SizedStats):
    """``hdem_upstream_stats`` (the binding is hydrodem_amd/upstream.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_hops", ctypes.c_int32),
                ("exits", ctypes.c_int64), ("heads", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _StreamOrderStats(_SizedStats):
    """``hdem_streamorder_stats`` (the binding is hydrodem_amd/streamorder.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_order", ctypes.c_int32),
                ("stream_cells", ctypes.c_int64), ("heads", ctypes.c_int64),
                ("junctions", ctypes.c_int64), ("links", ctypes.c_int64),
                ("max_hops", ctypes.c_int32),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_nodes", ctypes.c_float), ("ms_walk", ctypes.c_float),
                ("ms_gather", ctypes.c_float)]


class _StreamLinksStats(_SizedStats):
    """``hdem_streamlinks_stats`` (the binding is hydrodem_amd/streamnet.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_int32),
                ("links", ctypes.c_int64), ("stream_cells", ctypes.c_int64),
                ("catchment_cells", ctypes.c_int64), ("tops", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_rank", ctypes.c_float), ("ms_trace", ctypes.c_float),
                ("ms_tile", ctypes.c_float), ("ms_final", ctypes.c_float)]


class _ZonalStats(_SizedStats):
    """``hdem_zonal_stats`` (the binding is hydrodem_amd/zonal.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_int32),
                ("zones", ctypes.c_int64), ("unzoned", ctypes.c_int64),
                ("clamped", ctypes.c_int64), ("overflow", ctypes.c_int64),
                ("over_range", ctypes.c_int64), ("capped", ctypes.c_int64),
                ("max_id", ctypes.c_uint32),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_rank", ctypes.c_float), ("ms_tile", ctypes.c_float),
                ("ms_final", ctypes.c_float)]


class _TerrainStats(_SizedStats):
    """``hdem_terrain_stats`` (the binding is hydrodem_amd/terrain.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("ms_total", ctypes.c_float),
                ("nan_cells", ctypes.c_int64), ("flat_cells", ctypes.c_int64),
                ("floored_cells", ctypes.c_int64), ("invalid_codes", ctypes.c_int64)]


class _ProximityStats(_SizedStats):
    """``hdem_proximity_stats`` (the binding is hydrodem_amd/proximity.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("ms_row", ctypes.c_float),
                ("ms_column", ctypes.c_float), ("ms_final", ctypes.c_float),
                ("sources", ctypes.c_int64), ("unreached", ctypes.c_int64)]


class _FlowSumStats(_SizedStats):
    """``hdem_flowsum_stats`` (the binding is hydrodem_amd/flowsum.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_hops", ctypes.c_int32),
                ("exits", ctypes.c_int64), ("nan_weights", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _UpExtremeStats(_SizedStats):
    """``hdem_upextreme_stats`` (the binding is hydrodem_amd/upextreme.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_hops", ctypes.c_int32),
                ("exits", ctypes.c_int64), ("absent", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _FlowPathStats(_SizedStats):
    """``hdem_flowpath_stats`` (the binding is hydrodem_amd/flowpath.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("forest_rounds", ctypes.c_int32),
                ("stops", ctypes.c_int64), ("unreached", ctypes.c_int64),
                ("exits", ctypes.c_int64), ("nan_weights", ctypes.c_int64),
                ("absent", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_tile", ctypes.c_float), ("ms_forest", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _BreachStats(_SizedStats):
    """``hdem_breach_stats``: the extreme's fields, then the pits and the cells lowered."""
    _fields_ = _UpExtremeStats._fields_ + [("pits", ctypes.c_int64),
                                           ("lowered", ctypes.c_int64)]


class _DInfStats(_SizedStats):
    """``hdem_dinf_stats`` (the binding is hydrodem_amd/dinf.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("ms_total", ctypes.c_float),
                ("no_flow", ctypes.c_int64), ("fallback_cells", ctypes.c_int64)]


class _DInfAccStats(_SizedStats):
    """``hdem_dinfacc_stats`` (the binding is hydrodem_amd/dinf.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("rounds", ctypes.c_int32),
                ("tile_visits", ctypes.c_int64), ("split_cells", ctypes.c_int64),
                ("terminal_cells", ctypes.c_int64), ("invalid", ctypes.c_int64),
                ("outside", ctypes.c_int64), ("unresolved", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_classify", ctypes.c_float), ("ms_relax", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _DInfSumStats(_SizedStats):
    """``hdem_dinfsum_stats``: the accumulation's fields, then what the weights came to."""
    _fields_ = _DInfAccStats._fields_ + [("nan_weights", ctypes.c_int64),
                                         ("bad_weights", ctypes.c_int64),
                                         ("total", ctypes.c_uint64)]


class _DInfDistStats(_SizedStats):
    """``hdem_dinfdist_stats`` (the binding is hydrodem_amd/dinf.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("rounds", ctypes.c_int32),
                ("tile_visits", ctypes.c_int64), ("split_cells", ctypes.c_int64),
                ("terminal_cells", ctypes.c_int64), ("stop_cells", ctypes.c_int64),
                ("unreached_cells", ctypes.c_int64), ("invalid", ctypes.c_int64),
                ("outside", ctypes.c_int64), ("unresolved", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_classify", ctypes.c_float), ("ms_relax", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _DInfDistUpStats(_SizedStats):
    """``hdem_dinfdistup_stats`` (the binding is hydrodem_amd/dinf.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("rounds", ctypes.c_int32),
                ("tile_visits", ctypes.c_int64), ("ridge_cells", ctypes.c_int64),
                ("counted_links", ctypes.c_int64), ("ignored_links", ctypes.c_int64),
                ("merge_cells", ctypes.c_int64), ("nan_cells", ctypes.c_int64),
                ("invalid", ctypes.c_int64), ("outside", ctypes.c_int64),
                ("unresolved", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_classify", ctypes.c_float), ("ms_relax", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("reserved", ctypes.c_int32)]


class _CostDistanceStats(_SizedStats):
    """``hdem_costdistance_stats`` (the binding is hydrodem_amd/costdistance.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("rounds", ctypes.c_int32),
                ("tile_visits", ctypes.c_int64), ("sources", ctypes.c_int64),
                ("barriers", ctypes.c_int64), ("unreached", ctypes.c_int64),
                ("tie_cells", ctypes.c_int64), ("invalid", ctypes.c_int64),
                ("max_units", ctypes.c_int64),
                ("tile_h", ctypes.c_int32), ("tile_w", ctypes.c_int32),
                ("ms_classify", ctypes.c_float), ("ms_relax", ctypes.c_float),
                ("ms_final", ctypes.c_float), ("ms_trace", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 2)]


class _MFDStats(_SizedStats):
    """``hdem_mfd_stats`` (the binding is hydrodem_amd/mfd.py)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("ms_total", ctypes.c_float),
                ("no_flow", ctypes.c_int64), ("fallback_cells", ctypes.c_int64),
                ("split_cells", ctypes.c_int64)]


class _MFDAccStats(_SizedStats):
    """``hdem_mfdacc_stats``: the struct of the weighted D-infinity accumulation."""
    _fields_ = list(_DInfSumStats._fields_)


class _TerrainAreaStats(_SizedStats):
    """``hdem_terrain_area_stats``: the terrain fields, then the cells whose area is <= 0."""
    _fields_ = _TerrainStats._fields_ + [("nonpositive_area", ctypes.c_int64)]


DEPR_COMPACT = 1    # HDEM_DEPR_COMPACT
# columns of the depression table, in the order of the C ABI's pointers
DEPR_COLUMNS = (("first", np.uint32), ("area", np.uint32), ("level", np.float32),
                ("max_depth", np.float32), ("volume_q20", np.uint64))

# HDEM_FT_STREAMS_*
FT_STREAMS_NONE, FT_STREAMS_MASK_U8, FT_STREAMS_ACC_U32 = 0, 1, 2
# outputs of the flow trace, in the order of the C ABI's pointers
FT_OUTPUTS = (("stop", np.uint32), ("ncard", np.uint32), ("ndiag", np.uint32),
              ("distance", np.float32), ("hand", np.float32))

_c = ctypes
_vp, _i, _f = _c.c_void_p, _c.c_int, _c.c_float
# name -> argtypes; every function returns int except the three noted
SIGNATURES = {
    "hdem_device_count": [_c.POINTER(_i)],
    "hdem_init": [_i, _c.POINTER(_vp)],
    "hdem_shutdown": [_vp],
    "hdem_set_stream": [_vp, _vp],
    "hdem_synchronize": [_vp],
    "hdem_set_fill_slice_us": [_vp, _i],
    "hdem_set_fill_seam_words": [_vp, _vp],
    "hdem_fill_seam_apply_dev": [_vp, _vp, _i, _i, _vp, _vp, ctypes.c_int64, _vp],
    "hdem_set_fill_coarse_start": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_fill_hub_prepare_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_fill_hub_raster_dev": [_vp, _vp],
    "hdem_set_fill_hub_levels": [_vp, _vp],
    "hdem_malloc": [_vp, _c.c_size_t, _c.POINTER(_vp)],
    "hdem_free": [_vp, _vp],
    "hdem_trim": [_vp, _c.POINTER(_c.c_size_t)],
    "hdem_set_scribble": [_vp, _i],
    "hdem_memcpy_h2d": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_memcpy_d2h": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_memcpy_d2d": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_memset_dev": [_vp, _vp, _i, _c.c_size_t],
    "hdem_host_alloc": [_vp, _c.c_size_t, _c.POINTER(_vp)],
    "hdem_host_free": [_vp, _vp],
    "hdem_memcpy_h2d_async": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_memcpy_d2h_async": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_profile_enable": [_vp, _i],
    "hdem_profile_reset": [_vp],
    "hdem_profile_get": [_vp, _i, _c.POINTER(KernelStat)],
    "hdem_d8_f32": [_vp, _vp, _i, _i, _vp],
    "hdem_d8_f32_dev": [_vp, _vp, _i, _i, _vp],
    "hdem_sinkfill_f32": [_vp, _vp, _i, _i, _f, _i, _vp, _c.POINTER(FillStats)],
    "hdem_sinkfill_f32_dev": [_vp, _vp, _i, _i, _f, _i, _i, _vp,
                              _c.POINTER(FillStats)],
    "hdem_blockmax_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_copy_rate_dev": [_vp, _vp, _vp, _c.c_size_t],
    "hdem_elementwise_dev": [_vp, _i, _vp, _i, _vp, _i, _c.c_double, _c.c_int64, _vp, _i],
    "hdem_fourier_destripe_f32": [_vp, _vp, _i, _i, _vp, _vp],
    "hdem_fourier_destripe_f32_dev": [_vp, _vp, _i, _i, _vp, _vp],
    "hdem_blanks_fourier_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_isolated_points_u8_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_expand_u8_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_fft2_c2c_f32_dev": [_vp, _vp, _i, _i, _i],
    "hdem_fft2_c2c_f64_dev": [_vp, _vp, _i, _i, _i],
    "hdem_correct_nan_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_majority_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_binary_erosion_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp],
    "hdem_binary_closing_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp],
    "hdem_grey_dilation_f32_dev": [_vp, _vp, _i, _i, _i, _i, _vp],
    "hdem_grey_dilation_f64_dev": [_vp, _vp, _i, _i, _i, _i, _vp],
    "hdem_tidying_lagoons_f32_dev": [_vp, _vp, _i, _i, _vp],
    "hdem_lagoons_detection_f32_dev": [_vp, _vp, _i, _i, _vp, _vp, _vp],
    "hdem_sinkfill_d8_f32_dev": [_vp, _vp, _i, _i, _f, _i, _i, _vp, _vp,
                                 _c.POINTER(FillStats)],
    "hdem_boxmean3_f32": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_boxmean3_f64": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_boxmean3_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_boxmean3_f64_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_convolve_f32": [_vp, _vp, _i, _i, _vp, _i, _i, _vp],
    "hdem_convolve_f64": [_vp, _vp, _i, _i, _vp, _i, _i, _vp],
    "hdem_around_f32": [_vp, _vp, _c.c_int64, _vp],
    "hdem_around_f64": [_vp, _vp, _c.c_int64, _vp],
    "hdem_quadratic_f32": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_quadratic_f32_dev": [_vp, _vp, _i, _i, _i, _vp],
    "hdem_groves_f32": [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp],
    "hdem_groves_f32_dev": [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp],
    "hdem_flowacc_u8": [_vp, _vp, _i, _i, _vp, _c.POINTER(FlowAccStats)],
    "hdem_flowacc_u8_dev": [_vp, _vp, _i, _i, _vp, _c.POINTER(FlowAccStats)],
    "hdem_watershed_u8": [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _c.POINTER(WatershedStats)],
    "hdem_watershed_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _vp, _vp,
                              _c.POINTER(WatershedStats)],
    "hdem_flowtrace_u8": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _c.c_double,
                          _vp, _vp, _vp, _vp, _vp, _i, _c.POINTER(FlowTraceStats)],
    "hdem_flowtrace_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _c.c_double,
                              _vp, _vp, _vp, _vp, _vp, _i, _c.POINTER(FlowTraceStats)],
    "hdem_resolve_flats_u8": [_vp, _vp, _vp, _i, _i, _vp, _vp, _i,
                              _c.POINTER(ResolveFlatsStats)],
    "hdem_resolve_flats_u8_dev": [_vp, _vp, _vp, _i, _i, _vp, _vp, _i,
                                  _c.POINTER(ResolveFlatsStats)],
    "hdem_depressions_f32": [_vp, _vp, _vp, _i, _i, _i, _vp, _c.POINTER(DepressionsStats)],
    "hdem_depressions_f32_dev": [_vp, _vp, _vp, _i, _i, _i, _vp,
                                 _c.POINTER(DepressionsStats)],
    "hdem_depression_table_f32": [_vp, _vp, _vp, _vp, _i, _i, _c.c_int64,
                                  _vp, _vp, _vp, _vp, _vp],
    "hdem_depression_table_f32_dev": [_vp, _vp, _vp, _vp, _i, _i, _c.c_int64,
                                      _vp, _vp, _vp, _vp, _vp],
    "hdem_upstream_u8": [_vp, _vp, _i, _i, _c.c_double, _vp, _vp, _vp, _i,
                         _c.POINTER(_UpstreamStats)],
    "hdem_upstream_u8_dev": [_vp, _vp, _i, _i, _c.c_double, _vp, _vp, _vp, _i,
                             _c.POINTER(_UpstreamStats)],
    "hdem_streamorder_u8": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _vp, _vp, _i,
                            _c.POINTER(_StreamOrderStats)],
    "hdem_streamorder_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _vp, _vp, _i,
                                _c.POINTER(_StreamOrderStats)],
    "hdem_streamlinks_u8": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _vp, _vp, _vp,
                            _c.c_double, _c.c_int64] + [_vp] * 13 +
                           [_i, _c.POINTER(_StreamLinksStats)],
    "hdem_streamlinks_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _vp, _vp, _vp,
                                _c.c_double, _c.c_int64] + [_vp] * 13 +
                               [_i, _c.POINTER(_StreamLinksStats)],
    "hdem_zonal_count_u32": [_vp, _vp, _i, _i, _c.POINTER(_c.c_int64),
                             _c.POINTER(_ZonalStats)],
    "hdem_zonal_count_u32_dev": [_vp, _vp, _i, _i, _c.POINTER(_c.c_int64),
                                 _c.POINTER(_ZonalStats)],
    "hdem_zonal_table_u32": [_vp, _vp, _i, _i, _vp, _i, _i, _c.c_int64] + [_vp] * 13 +
                            [_i, _c.POINTER(_ZonalStats)],
    "hdem_zonal_table_u32_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _c.c_int64] + [_vp] * 13 +
                                [_i, _c.POINTER(_ZonalStats)],
    "hdem_zonal_broadcast_dev": [_vp, _vp, _i, _i, _c.c_int64, _vp, _c.c_uint32, _vp],
    "hdem_terrain_f32": [_vp, _vp, _i, _i, _vp, _vp] + [_c.c_double] * 4 + [_vp] * 8 +
                        [_i, _c.POINTER(_TerrainStats)],
    "hdem_terrain_f32_dev": [_vp, _vp, _i, _i, _vp, _vp] + [_c.c_double] * 4 + [_vp] * 8 +
                            [_i, _c.POINTER(_TerrainStats)],
    "hdem_proximity": [_vp, _vp, _i, _c.c_uint32, _i, _i, _vp, _c.c_double, _c.c_uint32] +
                      [_c.c_double] * 3 + [_vp] * 6 + [_c.POINTER(_ProximityStats)],
    "hdem_proximity_dev": [_vp, _vp, _i, _c.c_uint32, _i, _i, _vp, _c.c_double, _c.c_uint32] +
                          [_c.c_double] * 3 + [_vp] * 6 + [_c.POINTER(_ProximityStats)],
    "hdem_flowsum_u8": [_vp, _vp, _i, _i, _vp, _i, _i, _c.c_int64, _vp, _vp, _vp,
                        _c.POINTER(_FlowSumStats)],
    "hdem_flowsum_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _c.c_int64, _vp, _vp, _vp,
                            _c.POINTER(_FlowSumStats)],
    "hdem_upextreme_u8": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp,
                          _c.POINTER(_UpExtremeStats)],
    "hdem_upextreme_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp,
                              _c.POINTER(_UpExtremeStats)],
    "hdem_breach_f32": [_vp, _vp, _vp, _i, _i, _vp, _vp, _c.POINTER(_BreachStats)],
    "hdem_breach_f32_dev": [_vp, _vp, _vp, _i, _i, _vp, _vp, _c.POINTER(_BreachStats)],
    "hdem_flowpath_u8": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _i, _vp, _i, _i, _i, _vp,
                         _vp, _vp, _vp, _vp, _vp, _i, _c.POINTER(_FlowPathStats)],
    "hdem_flowpath_u8_dev": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _i, _vp, _i, _i, _i, _vp,
                             _vp, _vp, _vp, _vp, _vp, _i, _c.POINTER(_FlowPathStats)],
    "hdem_dinf_f32": [_vp, _vp, _i, _i, _vp, _c.c_double, _c.c_double, _vp, _vp, _vp, _i,
                      _c.POINTER(_DInfStats)],
    "hdem_dinf_f32_dev": [_vp, _vp, _i, _i, _vp, _c.c_double, _c.c_double, _vp, _vp, _vp, _i,
                          _c.POINTER(_DInfStats)],
    "hdem_dinfacc_u32": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _c.POINTER(_DInfAccStats)],
    "hdem_dinfacc_u32_dev": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _c.POINTER(_DInfAccStats)],
    "hdem_dinfsum_u32": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i,
                         _c.POINTER(_DInfSumStats)],
    "hdem_dinfsum_u32_dev": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i,
                             _c.POINTER(_DInfSumStats)],
    "hdem_terrain_area_f32": [_vp, _vp, _i, _i, _vp, _vp, _vp] + [_c.c_double] * 4 +
                             [_vp] * 8 + [_i, _c.POINTER(_TerrainAreaStats)],
    "hdem_terrain_area_f32_dev": [_vp, _vp, _i, _i, _vp, _vp, _vp] + [_c.c_double] * 4 +
                                 [_vp] * 8 + [_i, _c.POINTER(_TerrainAreaStats)],
    # one symbol each: HDEM_ON_DEVICE in the flags says whose pointers (hydrodem_amd/mfd.py)
    "hdem_mfd_f32": [_vp, _vp, _i, _i, _vp] + [_c.c_double] * 5 + [_vp, _vp, _i,
                                                                  _c.POINTER(_MFDStats)],
    "hdem_mfdacc_u64": [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _c.POINTER(_MFDAccStats)],
    "hdem_dinfdist_u32": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _vp, _c.c_double, _c.c_double,
                          _i, _i, _vp, _i, _c.POINTER(_DInfDistStats)],
    "hdem_dinfdistup_u32": [_vp, _vp, _i, _i, _vp, _c.c_double, _c.c_double, _i, _i, _c.c_uint32,
                            _vp, _i, _c.POINTER(_DInfDistUpStats)],
    "hdem_costdistance_f32": [_vp, _vp, _i, _i, _vp, _i, _c.c_uint32, _i, _c.c_double,
                              _c.c_int64, _vp, _vp, _vp, _vp, _vp, _i,
                              _c.POINTER(_CostDistanceStats)],
}
OTHER_SYMBOLS = {"hdem_last_error": _c.c_char_p, "hdem_version": _i}

_lib = None
_lock = threading.Lock()


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    ``libamdhip64.so`` (soname ``libamdhip64.so.7``, same as ``/opt/rocm``'s) and look
    it up by file name, so if this library pulled in the system runtime first, a later
    ``import torch`` would load a second runtime and report no usable GPU.  Loading
    torch's copy first (without importing torch) makes both bind to the same one.
    ``HYDRODEM_HIP_RUNTIME=system`` keeps the system runtime (processes that never
    import torch)."""
    if os.environ.get("HYDRODEM_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for base in (spec.submodule_search_locations or []) if spec else []:
        cand = os.path.join(base, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load_library(path=None):
    """dlopen the HIP library and declare every prototype.  Needs no GPU."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        _share_torch_hip_runtime()
        p = path or os.environ.get("HYDRODEM_HIP_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise BackendError(
                f"HIP library not found at {p}: build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` "
                f"(there is no CPU fallback)")
        try:
            lib = ctypes.CDLL(p)
        except OSError as exc:
            raise BackendError(f"cannot load {p}: {exc}") from exc
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        lib.hdem_last_error.argtypes = []
        lib.hdem_last_error.restype = ctypes.c_char_p
        lib.hdem_version.argtypes = []
        lib.hdem_version.restype = ctypes.c_int
        if path is None:
            _lib = lib
        return lib


def _raise(lib, rc, window=None, shape=None):
    msg = (lib.hdem_last_error() or b"").decode("utf-8", "replace")
    if rc == WINDOW_EVEN:
        raise WindowSizeEvenError(window)
    if rc == WINDOW_HIGH:
        raise WindowSizeHighError(window, shape)
    if rc == NOT_CONVERGED:
        raise NotConvergedError(msg)
    if rc == BAD_ARG:
        raise ValueError(msg)
    if rc == OOM:
        raise MemoryError(msg)
    raise BackendError(msg or f"hydrodem_hip status {rc}")


class Context:
    """One ``hdem_ctx`` (device, stream, workspace).  Use :func:`context`."""

    def __init__(self, device=0):
        self.lib = load_library()
        handle = ctypes.c_void_p()
        rc = self.lib.hdem_init(int(device), ctypes.byref(handle))
        if rc != OK:
            _raise(self.lib, rc)
        self.handle = handle
        self.device = int(device)

    def check(self, rc, **kw):
        if rc != OK:
            _raise(self.lib, rc, **kw)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hdem_shutdown(self.handle)
            self.handle = None

    def synchronize(self):
        self.check(self.lib.hdem_synchronize(self.handle))

    def set_fill_seam_words(self, dptr):
        """Three device ints for FILL_DEFER calls (``hdem_set_fill_seam_words``); 0: none."""
        self.check(self.lib.hdem_set_fill_seam_words(self.handle, ctypes.c_void_p(int(dptr) or None)))

    def fill_seam_apply(self, w_ptr, H, W, recv_top_ptr, recv_bot_ptr, pending, words_ptr):
        """``hdem_fill_seam_apply_dev``: received rows into the ghost rows, seam words set."""
        vp = lambda p: ctypes.c_void_p(int(p) or None)
        self.check(self.lib.hdem_fill_seam_apply_dev(self.handle, vp(w_ptr), int(H), int(W),
                                                     vp(recv_top_ptr), vp(recv_bot_ptr),
                                                     int(pending), vp(words_ptr)))

    def set_fill_slice_us(self, microseconds):
        """Time slice of the asynchronous sink-fill phase (0 = to convergence)."""
        self.check(self.lib.hdem_set_fill_slice_us(self.handle, int(microseconds)))

    def set_fill_coarse_start(self, coarse_ptr, ch, cw, block, row_map_ptr=None):
        """Device pointers; see ``hdem_set_fill_coarse_start``."""
        self.check(self.lib.hdem_set_fill_coarse_start(
            self.handle, ctypes.c_void_p(coarse_ptr or 0), int(ch), int(cw), int(block),
            ctypes.c_void_p(row_map_ptr or 0)))

    def fill_hub_prepare(self, z_ptr, h, w, flags, w_ptr):
        """``hdem_fill_hub_prepare_dev``: d of a row block into the interior of ``w``."""
        self.check(self.lib.hdem_fill_hub_prepare_dev(
            self.handle, ctypes.c_void_p(z_ptr), int(h), int(w), int(flags), ctypes.c_void_p(w_ptr)))

    def fill_hub_raster(self, out_ptr):
        """``hdem_fill_hub_raster_dev``: the prepared block's hub raster into ``out_ptr``."""
        self.check(self.lib.hdem_fill_hub_raster_dev(self.handle, ctypes.c_void_p(out_ptr)))

    def set_fill_hub_levels(self, levels_ptr):
        self.check(self.lib.hdem_set_fill_hub_levels(self.handle, ctypes.c_void_p(levels_ptr or 0)))

    def set_stream(self, stream_ptr):
        self.check(self.lib.hdem_set_stream(self.handle,
                                            ctypes.c_void_p(stream_ptr or 0)))

    def trim(self):
        """Hand the context's cached device blocks and scratch buffers back to the
        device (``hdem_trim``); returns the bytes released."""
        n = ctypes.c_size_t(0)
        self.check(self.lib.hdem_trim(self.handle, ctypes.byref(n)))
        return int(n.value)

    @contextlib.contextmanager
    def scribble(self, byte):
        """Scribble mode for the length of a ``with`` block (``hdem_set_scribble``): every
        block ``hdem_malloc`` hands out, every allocation of the library's own and the part of
        the scratch arena an operator asks for are filled with ``byte`` (0 ... 255) first.  A
        result that depends on ``byte`` comes from memory nobody wrote.  Off again on exit."""
        if isinstance(byte, bool) or int(byte) != byte or not 0 <= int(byte) <= 255:
            raise ValueError(f"the scribble byte is 0 ... 255, got {byte!r}")
        self.check(self.lib.hdem_set_scribble(self.handle, int(byte)))
        try:
            yield self
        finally:
            self.check(self.lib.hdem_set_scribble(self.handle, -1))

    # -- timing ----------------------------------------------------------
    def profile(self, on=True):
        self.check(self.lib.hdem_profile_enable(self.handle, int(bool(on))))

    def profile_reset(self):
        self.check(self.lib.hdem_profile_reset(self.handle))

    def profile_get(self, kernel_id):
        st = KernelStat()
        self.check(self.lib.hdem_profile_get(self.handle, kernel_id,
                                             ctypes.byref(st)))
        return {"launches": st.launches, "ms": st.ms, "units": st.units}


_contexts = {}


def context(device=None):
    """Per-process context of ``device`` (default: ``HYDRODEM_DEVICE`` or 0)."""
    if device is None:
        device = int(os.environ.get("HYDRODEM_DEVICE", "0"))
    with _lock:
        ctx = _contexts.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _contexts[device] = ctx
    return ctx


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    lib.hdem_device_count(ctypes.byref(n))
    return n.value


_DTYPES = {np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.uint8),
           np.dtype(np.complex64), np.dtype(np.complex128), np.dtype(np.int64),
           np.dtype(np.uint32), np.dtype(np.uint64)}


class _HostBlocks:
    """Page-locked host memory for the arrays the host entry points return.

    A result that comes back into a fresh ``np.empty`` pays for its pages three times: the
    faults when they are first written (taken on 16 threads by the library, still ~10 ms per
    GiB), a device-to-host copy that stages through the driver at 40 instead of 56 GB/s, and
    ~50 ms per GiB of unmapping when the array is dropped -- more than the kernels and the
    bus together for every operator here.  Results of 32 MiB and more are therefore NumPy
    arrays over page-locked blocks that return here when the array (and every view of it)
    has gone, and are handed out again for the next result of that size.  The cache is capped
    (``HDEM_HOST_POOL_MIB``, default 8 GiB; 0 = plain ``np.empty``), and so is what may be
    page-locked at any one time, arrays in the caller's hands included
    (``HDEM_HOST_PINNED_MAX_MIB``, default 4 x the cache): beyond it results are plain
    ``np.empty`` arrays.  A block the cache has no room for is unlocked by the next call that
    asks for memory here, not by the finalizer that returned it -- that one runs on whatever
    thread drops the last reference and makes no device call."""

    MIN_BYTES = 32 << 20

    def __init__(self):
        self.lock = threading.Lock()
        self.spare = {}                      # nbytes -> [address, ...]
        self.cached = 0
        self.outstanding = 0                 # page-locked bytes in callers' hands
        self.to_free = []                    # blocks waiting to be unlocked
        mib = os.environ.get("HDEM_HOST_POOL_MIB")
        self.cap = (int(mib) << 20) if mib is not None else (8 << 30)
        mib = os.environ.get("HDEM_HOST_PINNED_MAX_MIB")
        self.pinned_max = (int(mib) << 20) if mib is not None else 4 * self.cap

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        count = int(np.prod(shape, dtype=np.int64))
        nbytes = count * dtype.itemsize
        if nbytes < self.MIN_BYTES or self.cap <= 0:
            return np.empty(shape, dtype)
        try:
            ctx = context()
            with self.lock:
                doomed, self.to_free = self.to_free, []
                stack = self.spare.get(nbytes)
                addr = stack.pop() if stack else None
                if addr is not None:
                    self.cached -= nbytes
                elif self.outstanding + self.cached + nbytes > self.pinned_max:
                    addr = 0                     # enough is page-locked already
                if addr != 0:
                    self.outstanding += nbytes
            for old in doomed:
                ctx.lib.hdem_host_free(ctx.handle, ctypes.c_void_p(old))
            if addr == 0:
                return np.empty(shape, dtype)
            if addr is None:
                ptr = ctypes.c_void_p()
                if ctx.lib.hdem_host_alloc(ctx.handle, nbytes, ctypes.byref(ptr)) != 0 or not ptr.value:
                    with self.lock:
                        self.outstanding -= nbytes
                    return np.empty(shape, dtype)
                addr = ptr.value
            buf = (ctypes.c_char * nbytes).from_address(addr)
            root = np.frombuffer(buf, dtype=dtype, count=count)
            weakref.finalize(root, self._give_back, addr, nbytes)
            return root.reshape(shape)
        except Exception:  # pylint: disable=broad-except
            return np.empty(shape, dtype)

    def _give_back(self, addr, nbytes):
        # (a finalizer: any thread, possibly during interpreter shutdown -- no device call)
        with self.lock:
            self.outstanding -= nbytes
            if self.cached + nbytes <= self.cap:
                self.spare.setdefault(nbytes, []).append(addr)
                self.cached += nbytes
            else:
                self.to_free.append(addr)


_host_blocks = _HostBlocks()


def host_empty(shape, dtype):
    """An uninitialised host array for a result of the library (see :class:`_HostBlocks`)."""
    return _host_blocks.empty(shape, dtype)


class DeviceRaster:
    """A 2-D raster resident in HBM (owning unless wrapped)."""

    def __init__(self, ctx, ptr, shape, dtype, owner=True, keepalive=None):
        self.ctx, self.ptr, self.shape = ctx, ptr, tuple(shape)
        self.dtype = np.dtype(dtype)
        self._owner = owner
        self._keepalive = keepalive

    @property
    def nbytes(self):
        return int(np.prod(self.shape)) * self.dtype.itemsize

    @classmethod
    def empty(cls, shape, dtype, ctx=None):
        ctx = ctx or context()
        dtype = np.dtype(dtype)
        if dtype not in _DTYPES:
            raise ValueError(f"unsupported raster dtype {dtype}")
        ptr = ctypes.c_void_p()
        nbytes = int(np.prod(shape)) * dtype.itemsize
        ctx.check(ctx.lib.hdem_malloc(ctx.handle, nbytes, ctypes.byref(ptr)))
        return cls(ctx, ptr.value, shape, dtype)

    @classmethod
    def from_host(cls, array, dtype=None, ctx=None):
        a = np.ascontiguousarray(array, dtype=dtype or (
            array.dtype if array.dtype in _DTYPES else np.float32))
        _need2d(a)
        r = cls.empty(a.shape, a.dtype, ctx)
        r.ctx.check(r.ctx.lib.hdem_memcpy_h2d(r.ctx.handle, r.ptr,
                                              a.ctypes.data, a.nbytes))
        return r

    @classmethod
    def wrap(cls, ptr, shape, dtype, ctx=None, keepalive=None):
        """Non-owning view of device memory someone else allocated (e.g. a
        torch tensor: ``wrap(t.data_ptr(), t.shape, np.float32, keepalive=t)``)."""
        return cls(ctx or context(), int(ptr), shape, dtype, owner=False,
                   keepalive=keepalive)

    def to_host(self, out=None):
        """The raster as a host array: a fresh one (:func:`host_empty`), or ``out``, a
        C-contiguous array of the raster's type and size that the caller wants written."""
        if out is None:
            out = host_empty(self.shape, self.dtype)
        elif not out.flags.c_contiguous or (out.dtype, out.nbytes) != (self.dtype, self.nbytes):
            raise ValueError(f"out is not a contiguous {self.dtype} array of {self.nbytes} bytes")
        self.ctx.check(self.ctx.lib.hdem_memcpy_d2h(self.ctx.handle,
                                                    out.ctypes.data, self.ptr,
                                                    out.nbytes))
        return out

    def free(self):
        if self._owner and self.ptr:
            self.ctx.lib.hdem_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:  # pylint: disable=broad-except
            pass


def is_device_raster(x):
    """A :class:`DeviceRaster`, or anything that quacks like one."""
    return hasattr(x, "ptr") and hasattr(x, "to_host")


@contextlib.contextmanager
def on_device(operand, dtype=None, ctx=None):
    """``operand`` as a device raster for the length of a call.  A device raster (and ``None``,
    an operand left out) is handed through and stays its owner's; a host array is uploaded
    as ``dtype`` on ``ctx`` and freed on the way out."""
    if operand is None or is_device_raster(operand):
        yield operand
        return
    with DeviceRaster.from_host(operand, dtype=dtype, ctx=ctx) as raster:
        yield raster


@contextlib.contextmanager
def result_raster(out, shape, dtype, ctx):
    """The raster an operator writes a result into: ``out``, or a fresh one when ``None``.

    Who frees what, all over the package.  A raster a function allocates and does not return
    (an uploaded operand, a scratch, a stage of a chain) is released by a ``with`` block.  One
    it allocates for the caller is the caller's once returned, and is freed here if the block
    raises first; one the caller passed in is never freed.  ``DeviceRaster.__del__`` is the
    net under user code: nothing in here counts on it."""
    if out is not None:
        yield out
        return
    fresh = DeviceRaster.empty(shape, dtype, ctx)
    try:
        yield fresh
    except BaseException:
        fresh.free()
        raise


# ---------------------------------------------------------------------------
# device-resident operators (thin: one C call each)
# ---------------------------------------------------------------------------

def _need(r, dtype):
    if r.dtype != np.dtype(dtype):
        raise ValueError(f"expected a {np.dtype(dtype)} raster, got {r.dtype}")


def _need2d(r):
    if len(r.shape) != 2:
        raise ValueError(f"expected a 2-D raster, got shape {r.shape}")


def _one_call_dev(name, x, dtype, out, out_dtype, *args, window=None):
    """The device operators that are one C call ``name(ctx, x, H, W, *args, out)`` on a raster
    of ``dtype``; a ``window`` is what the call may refuse."""
    _need(x, dtype)
    c = x.ctx
    with result_raster(out, x.shape, out_dtype, c) as out:
        c.check(getattr(c.lib, name)(c.handle, x.ptr, *x.shape, *args, out.ptr),
                window=window, shape=x.shape)
    return out


def d8_dev(z, out=None):
    return _one_call_dev("hdem_d8_f32_dev", z, np.float32, out, np.uint8)


# ---------------------------------------------------------------------------
# the terrain operators: one body each, entered from a host side and a device side
# ---------------------------------------------------------------------------

class _Side:
    """Who calls the body of a terrain operator: ``_HOST`` with NumPy arrays, for the C entry
    point of the operator's name, or ``_DEVICE`` with device rasters, for its ``_dev`` twin."""

    def __init__(self, device):
        self.device, self.suffix = device, "_dev" if device else ""

    def take(self, name, a, required=False, mask=False):
        """The operand ``name``: a device raster as it is; a host operand as a contiguous
        ``ndarray`` (a bool ``mask`` as bytes; ``None``, left out, unless ``required``)."""
        if self.device or (a is None and not required):
            return a
        if not isinstance(a, np.ndarray):
            raise ValueError(f"{name} is a NumPy array, got {type(a)}")
        return np.ascontiguousarray(a.view(np.uint8) if mask and a.dtype == np.bool_ else a)

    def address(self, a):
        return None if a is None else a.ptr if self.device else a.ctypes.data

    def context(self, raster):
        return raster.ctx if self.device else context()

    def result(self, stack, out, shape, dtype, ctx):
        """Where a result goes: a :func:`host_empty` array, or a :func:`result_raster`
        entered in the body's ``stack``, so that its ownership rule is the one rule."""
        if not self.device:
            return host_empty(shape, dtype)
        return stack.enter_context(result_raster(out, shape, dtype, ctx))

    def call(self, c, name, *args):
        c.check(getattr(c.lib, name + self.suffix)(c.handle, *args))


_HOST, _DEVICE = _Side(False), _Side(True)


def _check(raster, dtype, says, what=None, flat=None, like=None):
    """The one operand check of the terrain operators, in the words of the caller: ``raster``
    (anything with ``dtype`` and ``shape``) ``says`` it is of ``dtype`` (``what``: another
    name for that; ``None``: any), is 2-D for the operator that ``flat`` names, and has the
    shape ``like = (noun, shape)``.  Returns its shape as a tuple."""
    shape = tuple(raster.shape)
    if dtype is not None and np.dtype(raster.dtype) != np.dtype(dtype):
        raise ValueError(f"{says} {what or np.dtype(dtype)}, got {raster.dtype}")
    if flat is not None and len(shape) != 2:
        raise ValueError(f"{flat} a 2-D raster, got {len(shape)} dimensions")
    if like is not None and shape != like[1]:
        raise ValueError(f"{says} {shape}, {like[0]} {like[1]}")
    return shape


def _d8_codes(codes, operator):
    _check(codes, np.uint8, f"{operator} takes", "uint8 D8 codes")
    _need2d(codes)


def _cellsize(cellsize):
    """``cellsize`` as a float: a number, finite and positive."""
    try:
        cellsize = float(cellsize)
    except (TypeError, ValueError):
        raise ValueError(f"cellsize is a number, got {cellsize!r}") from None
    if not np.isfinite(cellsize) or cellsize <= 0:
        raise ValueError(f"cellsize must be finite and positive, got {cellsize}")
    return cellsize


def _flowacc(side, codes, out):
    _d8_codes(codes, "flow accumulation")
    codes = side.take("codes", codes)
    c = side.context(codes)
    st = FlowAccStats()
    with contextlib.ExitStack() as stack:
        out = side.result(stack, out, codes.shape, np.uint32, c)
        side.call(c, "hdem_flowacc_u8", side.address(codes), *codes.shape, side.address(out),
                  ctypes.byref(st))
    return out, st.as_dict()


def flowacc_dev(codes, out=None):
    """D8 flow accumulation of a uint8 code raster (``hdem_flowacc_u8_dev``): a uint32
    raster and the stats dict.  Synchronises (the call reads its validity counters)."""
    return _flowacc(_DEVICE, codes, out)


def flowacc(codes, return_stats=False):
    """D8 flow accumulation of a uint8 code raster (``hdem_flowacc_u8``): uint32."""
    out, stats = _flowacc(_HOST, np.asarray(codes), None)
    return (out, stats) if return_stats else out


def _watershed(side, codes, seeds, compact, out):
    _d8_codes(codes, "watershed labelling")
    codes = side.take("codes", codes)
    if seeds is not None:
        _check(seeds, np.uint32, "seeds are", like=("the codes", tuple(codes.shape)))
        if compact:
            raise ValueError("compact labels number the outlets: no pour points with them")
        seeds = side.take("seeds", seeds)
    c = side.context(codes)
    st = WatershedStats()
    with contextlib.ExitStack() as stack:
        out = side.result(stack, out, codes.shape, np.uint32, c)
        # every cell may be an outlet: room for all, the first K come back -- in host memory
        # (untouched pages cost nothing), or in a device scratch that K entries are read from
        room = None
        if compact:
            room = np.empty(codes.size, np.uint32) if not side.device else \
                stack.enter_context(DeviceRaster.empty(codes.shape, np.uint32, c))
        side.call(c, "hdem_watershed_u8", side.address(codes), *codes.shape,
                  side.address(seeds), WS_COMPACT if compact else 0, side.address(out),
                  side.address(room), ctypes.byref(st))
        outlets = None
        if compact and not side.device:
            outlets = room[:st.basins].copy()
        elif compact:
            first = DeviceRaster.wrap(room.ptr, (st.basins,), np.uint32, c)
            outlets = first.to_host(np.empty(st.basins, np.uint32))
    return out, outlets, st.as_dict()


def watershed_dev(codes, seeds=None, compact=False, out=None):
    """D8 watershed labels of a uint8 code raster (``hdem_watershed_u8_dev``): a uint32
    raster, the ``outlets`` of the compact numbering (a host uint32 array of K flat indices,
    ``None`` otherwise) and the stats dict.  ``seeds``: a uint32 raster of pour points or
    ``None``.  Synchronises (the call reads its validity counters)."""
    return _watershed(_DEVICE, codes, seeds, compact, out)


def watershed(codes, seeds=None, compact=False):
    """D8 watershed labels of a uint8 code raster (``hdem_watershed_u8``): the uint32
    labels, the ``outlets`` of the compact numbering (``None`` otherwise) and the stats
    dict.  ``seeds``: a uint32 raster of pour points of the codes' shape, or ``None``."""
    return _watershed(_HOST, np.asarray(codes), None if seeds is None else np.asarray(seeds),
                      compact, None)


def flowtrace_args(codes, streams, threshold, dem, cellsize, want):
    """The checks of the flow trace that need no device: ``codes``, ``streams`` and ``dem`` are
    anything with ``dtype`` and ``shape`` (NumPy arrays or device rasters).  Returns the
    stream kind, the threshold for the C call and ``want`` as a tuple in the ABI's order."""
    shape = _check(codes, np.uint8, "the flow trace takes", "uint8 D8 codes",
                   flat="the flow trace takes")
    if isinstance(want, str):
        want = (want,)
    names = [n for n, _ in FT_OUTPUTS]
    unknown = [w for w in want if w not in names]
    if unknown:
        raise ValueError(f"unknown flow trace outputs {unknown}: choose among {names}")
    want = tuple(n for n in names if n in want)
    if not want:
        raise ValueError(f"no output wanted: choose among {names}")
    if streams is None:
        kind = FT_STREAMS_NONE
        if threshold is not None:
            raise ValueError("a threshold needs the uint32 raster it applies to")
        threshold = 0
    else:
        _check(streams, None, "streams are", like=("the codes", shape))
        if np.dtype(streams.dtype) == np.uint8:
            kind = FT_STREAMS_MASK_U8
            if threshold is not None:
                raise ValueError("a uint8 stream mask takes no threshold")
            threshold = 0
        elif np.dtype(streams.dtype) == np.uint32:
            kind = FT_STREAMS_ACC_U32
            if threshold is None:
                raise ValueError("a uint32 stream raster needs a threshold")
            if isinstance(threshold, bool) or int(threshold) != threshold or \
                    not 1 <= int(threshold) <= 0xFFFFFFFF:
                raise ValueError(f"threshold is an integer in 1 ... 2^32 - 1, got {threshold!r}")
            threshold = int(threshold)
        else:
            raise ValueError("streams are a uint8 mask or a uint32 raster with a threshold, "
                             f"got {streams.dtype}")
    if dem is not None:
        _check(dem, np.float32, "the dem is", like=("the codes", shape))
    elif "hand" in want:
        raise ValueError("hand needs the dem it is measured on")
    _cellsize(cellsize)
    return kind, threshold, want


def _flowtrace(side, codes, streams, threshold, dem, cellsize, want):
    codes, streams, dem = (side.take("codes", codes), side.take("streams", streams, mask=True),
                           side.take("dem", dem))
    kind, threshold, want = flowtrace_args(codes, streams, threshold, dem, cellsize, want)
    c = side.context(codes)
    st = FlowTraceStats()
    with contextlib.ExitStack() as stack:
        outs = {name: side.result(stack, None, codes.shape, dtype, c)
                for name, dtype in FT_OUTPUTS if name in want}
        side.call(c, "hdem_flowtrace_u8", side.address(codes), *codes.shape,
                  side.address(streams), kind, threshold, side.address(dem), float(cellsize),
                  *[side.address(outs.get(name)) for name, _ in FT_OUTPUTS], 0, ctypes.byref(st))
    return outs, st.as_dict()


def flowtrace_dev(codes, streams=None, threshold=None, dem=None, cellsize=1.0,
                  want=("distance",)):
    """D8 flow trace of a uint8 code raster (``hdem_flowtrace_u8_dev``): for every cell the
    first stop on its path and the steps to it.  ``streams``: ``None`` (paths end at terminal
    cells), a uint8 mask raster, or a uint32 raster with ``threshold`` (stream where
    ``>= threshold``).  ``want``: any of ``stop``, ``ncard``, ``ndiag`` (uint32), ``distance``,
    ``hand`` (float32; ``hand`` needs the float32 ``dem``).  Returns ``{name: DeviceRaster}``
    and the stats dict.  Synchronises (the call reads its validity counters)."""
    return _flowtrace(_DEVICE, codes, streams, threshold, dem, cellsize, want)


def flowtrace(codes, streams=None, threshold=None, dem=None, cellsize=1.0, want=("distance",)):
    """D8 flow trace of host arrays (``hdem_flowtrace_u8``; see :func:`flowtrace_dev`):
    ``{name: ndarray}`` and the stats dict.  A bool ``streams`` array is a mask."""
    return _flowtrace(_HOST, codes, streams, threshold, dem, cellsize, want)


def resolve_flats_args(codes, dem):
    """The checks of the flat resolution that need no device: ``codes`` and ``dem`` are
    anything with ``dtype`` and ``shape`` (NumPy arrays or device rasters)."""
    shape = _check(codes, np.uint8, "flat resolution takes", "uint8 D8 codes",
                   flat="flat resolution takes")
    if dem is None:
        raise ValueError("flat resolution needs the dem the codes were made on")
    _check(dem, np.float32, "the dem is", like=("the codes", shape))


def _resolve_flats(side, codes, dem, want_distance, out):
    codes, dem = side.take("codes", codes), side.take("dem", dem)
    resolve_flats_args(codes, dem)
    c = side.context(codes)
    st = ResolveFlatsStats()
    with contextlib.ExitStack() as stack:
        out = side.result(stack, out, codes.shape, np.uint8, c)
        dist = side.result(stack, None, codes.shape, np.uint32, c) if want_distance else None
        side.call(c, "hdem_resolve_flats_u8", side.address(codes), side.address(dem),
                  *codes.shape, side.address(out), side.address(dist), 0, ctypes.byref(st))
    return out, dist, st.as_dict()


def resolve_flats_dev(codes, dem, want_distance=False, out=None):
    """D8 directions across the flats of ``dem`` (``hdem_resolve_flats_u8_dev``): the uint8
    codes with every flat cell pointed along a shortest equal-elevation path to where its
    flat drains, the uint32 distance raster (``None`` unless ``want_distance``) and the
    stats dict.  ``out`` may be ``codes`` itself.  Synchronises once per relaxation round."""
    return _resolve_flats(_DEVICE, codes, dem, want_distance, out)


def resolve_flats(codes, dem, want_distance=False):
    """D8 directions across flats of host arrays (``hdem_resolve_flats_u8``; see
    :func:`resolve_flats_dev`): the codes, the distances or ``None``, the stats dict."""
    return _resolve_flats(_HOST, codes, dem, want_distance, None)


def depressions_args(dem, filled, labels=None):
    """The checks of the depression operators that need no device: ``dem``, ``filled`` and
    ``labels`` are anything with ``dtype`` and ``shape`` (NumPy arrays or device rasters)."""
    shape = _check(filled, np.float32, "the filled raster is", flat="depressions take")
    if dem is None:
        raise ValueError("depressions need the dem the filled raster is compared with")
    _check(dem, np.float32, "the dem is", like=("the filled raster", shape))
    if labels is not None:
        _check(labels, np.uint32, "the labels are", like=("the filled raster", shape))


def _depression_count(count):
    if isinstance(count, bool) or int(count) != count or int(count) < 0:
        raise ValueError(f"count is the number of depressions, got {count!r}")
    return int(count)


def depression_table_of(columns, cellsize=1.0):
    """The table as the operators hand it out: the five columns of the C ABI and ``volume``,
    float64, ``volume_q20 / 2**20 * cellsize**2``."""
    table = dict(columns)
    table["volume"] = table["volume_q20"].astype(np.float64) / 2.0 ** 20 * float(cellsize) ** 2
    return table


def _depressions(side, dem, filled, compact, out):
    dem, filled = (side.take("dem", dem, required=True),
                   side.take("filled", filled, required=True))
    depressions_args(dem, filled)
    c = side.context(filled)
    st = DepressionsStats()
    with contextlib.ExitStack() as stack:
        out = side.result(stack, out, filled.shape, np.uint32, c)
        side.call(c, "hdem_depressions_f32", side.address(dem), side.address(filled),
                  *filled.shape, DEPR_COMPACT if compact else 0, side.address(out),
                  ctypes.byref(st))
    return out, st.as_dict()


def depressions_dev(dem, filled, compact=True, out=None):
    """Depression labels of a ``dem`` / ``filled`` pair of float32 rasters
    (``hdem_depressions_f32_dev``): a uint32 raster and the stats dict, whose ``depressions``
    is K.  ``compact``: labels 1 ... K in scan order of the first cell (the numbering of
    ``scipy.ndimage.label``), else 1 + the flat index of the first cell.  Synchronises (the
    call reads K and its validity counters)."""
    return _depressions(_DEVICE, dem, filled, compact, out)


def depressions(dem, filled, compact=True):
    """Depression labels of host arrays (``hdem_depressions_f32``; see
    :func:`depressions_dev`): the uint32 labels and the stats dict."""
    return _depressions(_HOST, dem, filled, compact, None)


def _depression_table(side, dem, filled, labels, count, cellsize):
    dem, filled, labels = (side.take("dem", dem, required=True),
                           side.take("filled", filled, required=True),
                           side.take("labels", labels, required=True))
    depressions_args(dem, filled, labels)
    count = _depression_count(count)
    if not side.device:     # five columns, written where they are (``offsets``: addresses)
        columns = {name: np.empty(count, dtype) for name, dtype in DEPR_COLUMNS}
        offsets = {name: column.ctypes.data for name, column in columns.items()}
    else:
        # one device block, downloaded and freed here: the uint64 column first, then the
        # four 4-byte columns
        order = sorted(DEPR_COLUMNS, key=lambda col: -np.dtype(col[1]).itemsize)
        host = np.empty(sum(np.dtype(t).itemsize for _, t in order) * count, np.uint8)
        columns, offsets, at = {}, {}, 0
        for name, dtype in order:
            n = np.dtype(dtype).itemsize * count
            columns[name], offsets[name] = host[at:at + n].view(dtype), at
            at += n
    if count:
        c = side.context(filled)
        with contextlib.ExitStack() as stack:
            if side.device:
                block = stack.enter_context(DeviceRaster.empty(host.shape, np.uint8, c))
                offsets = {name: block.ptr + at for name, at in offsets.items()}
            side.call(c, "hdem_depression_table_f32", side.address(dem), side.address(filled),
                      side.address(labels), *filled.shape, count,
                      *[offsets[name] for name, _ in DEPR_COLUMNS])
            if side.device:
                block.to_host(host)
    return depression_table_of({name: columns[name] for name, _ in DEPR_COLUMNS}, cellsize)


def depression_table_dev(dem, filled, labels, count, cellsize=1.0):
    """One row per compact label of ``labels`` (``hdem_depression_table_f32_dev``; ``count``
    is K of the labelling): a dict of host arrays of length K, ``first``, ``area``, ``level``,
    ``max_depth``, ``volume_q20`` and ``volume``.  The columns are gathered in one device block
    that is downloaded and freed here; ``count == 0`` allocates and launches nothing."""
    return _depression_table(_DEVICE, dem, filled, labels, count, cellsize)


def depression_table(dem, filled, labels, count, cellsize=1.0):
    """The depression table of host arrays (``hdem_depression_table_f32``; see
    :func:`depression_table_dev`)."""
    return _depression_table(_HOST, dem, filled, labels, count, cellsize)


def sinkfill_dev(z, eps=0.0, max_rounds=0, out=None, flags=FILL_INIT):
    _need(z, np.float32)
    c = z.ctx
    st = FillStats()
    with result_raster(out, z.shape, np.float32, c) as out:
        c.check(c.lib.hdem_sinkfill_f32_dev(c.handle, z.ptr, z.shape[0], z.shape[1],
                                            float(eps), int(max_rounds), int(flags),
                                            out.ptr, ctypes.byref(st)))
    return out, st.as_dict()


def blockmax_dev(z, block, out=None):
    """Block-maximum coarsening (``hdem_blockmax_f32_dev``)."""
    _need(z, np.float32)
    shape = (-(-z.shape[0] // block), -(-z.shape[1] // block))
    c = z.ctx
    with result_raster(out, shape, np.float32, c) as out:
        c.check(c.lib.hdem_blockmax_f32_dev(c.handle, z.ptr, z.shape[0], z.shape[1],
                                            int(block), out.ptr))
    return out


def logical_type(dtype):
    """The NumPy type a raster of ``dtype`` stands for in the element-wise algebra: a uint8
    raster is the device form of NumPy's bool / int64 masks and counts as int64."""
    dtype = np.dtype(dtype)
    return np.dtype(np.int64) if dtype == np.uint8 else dtype


def elementwise_work_type(image_dtype, operand):
    """The type NumPy would do ``ufunc(image, operand)`` in: ``np.result_type`` of the
    logical types.  ``operand`` is a dtype (a raster's logical type) or a scalar; a Python
    scalar is weak (it takes the image's float width), a NumPy scalar or 0-d array counts
    with its own type.  One of float32, float64 and int64."""
    if isinstance(operand, (np.dtype, type)):
        other = logical_type(operand)
    elif isinstance(operand, (np.generic, np.ndarray)):
        other = operand.dtype
    elif isinstance(operand, (bool, int, float)):
        other = operand
    else:
        raise ValueError(f"element-wise operand {type(operand).__name__} is neither a "
                         "raster nor a real scalar")
    work = np.result_type(logical_type(image_dtype), other)
    if work not in (np.float32, np.float64, np.int64):
        raise ValueError(f"element-wise operators work in float32, float64 or int64, "
                         f"not {work}")
    return work


def elementwise_dev(op, image, operand, out_dtype=None, out=None, operand_type=None):
    """``op(image, operand)`` cell by cell on device rasters (``hdem_elementwise_dev``), with
    the values and the result type of the NumPy ufunc on the *logical* types
    (:func:`logical_type`: a uint8 raster stands for an int64 mask).

    ``operand`` is a :class:`DeviceRaster` of the same shape or a scalar; ``operand_type``
    names the NumPy type an operand raster stands for where that is not its own (a bool
    array that went up as bytes).  The work type is ``np.result_type`` of the two
    (:func:`elementwise_work_type`): float32 with int64 is float64, a Python scalar takes
    the raster's float width, an ``np.float64`` scalar makes float64.  The kernel computes
    in double, so a scalar that NumPy would round to float32 is rounded here before it is
    passed; the double result of two float32 values, rounded once on the store, is then the
    float32 result (the product is exact in double; 53 >= 2 * 24 + 2 bits make the second
    rounding of a sum or difference harmless).

    Result type: ``out.dtype``, ``out_dtype``, or uint8 for comparisons / NONZERO and the
    work type for the arithmetic.  An int64 result is stored as uint8 only for a uint8
    image times the scalar 0 or 1 (``mask * 1``); nothing says of two uint8 rasters that
    they hold masks, so their product is int64.  Integers are exact within +-2^53.

    A given type is where the double result is stored, once.  A float64 ``out_dtype`` --
    or a float64 ``out``, which means the same here -- is therefore NumPy's
    ``ufunc(..., dtype=float64)``: float32 values are combined in double and a Python
    scalar stays unrounded.  It is not NumPy's ``out=``, which would work in float32 and
    widen afterwards; the kernel has no float32 rounding in front of a wider store.  A
    type narrower than the work type is one cast of the result, as NumPy's ``out=`` does.
    ``out`` and ``out_dtype`` together must name the same type."""
    c = image.ctx
    raster = operand if isinstance(operand, DeviceRaster) else None
    if raster is not None and raster.shape != image.shape:
        raise ValueError(f"operand shape {raster.shape} != image shape {image.shape}")
    if image.dtype not in _EW_TYPES or (raster is not None and raster.dtype not in _EW_TYPES):
        raise ValueError("element-wise operators take float32, float64, uint8 or int64 rasters")
    if raster is not None:
        work = elementwise_work_type(
            image.dtype, np.dtype(raster.dtype if operand_type is None else operand_type))
    else:
        work = elementwise_work_type(image.dtype, operand)
    if out is not None:
        if out_dtype is not None and np.dtype(out_dtype) != out.dtype:
            raise ValueError(f"out is a {out.dtype} raster, out_dtype says {np.dtype(out_dtype)}")
        out_dtype = out.dtype
    elif out_dtype is None:
        if op in (EW_GT, EW_LT, EW_NONZERO):
            out_dtype = np.uint8
        elif op == EW_MUL and work == np.int64 and image.dtype == np.uint8 and \
                raster is None and operand in (0, 1):
            out_dtype = np.uint8
        else:
            out_dtype = work
    scalar = 0.0
    if raster is None:
        # np.multiply(a, s, dtype=float64) would take the Python scalar unrounded
        narrow = work == np.float32 and np.dtype(out_dtype) != np.float64
        scalar = float(np.float32(operand)) if narrow else float(operand)
    if out is not None and (out.shape != image.shape or out.dtype not in _EW_TYPES):
        raise ValueError(f"out is {out.dtype} {out.shape}, the image has shape {image.shape}")
    n = int(np.prod(image.shape))
    with result_raster(out, image.shape, out_dtype, c) as out:
        c.check(c.lib.hdem_elementwise_dev(
            c.handle, int(op), image.ptr, _EW_TYPES[image.dtype],
            raster.ptr if raster is not None else None,
            _EW_TYPES[raster.dtype] if raster is not None else 0,
            scalar, n, out.ptr, _EW_TYPES[out.dtype]))
    return out


def copy_rate(ctx=None, nbytes=1 << 30, reps=5):
    """Measured device copy rate in GB/s (bytes moved through HBM = 2 x copied bytes per
    second): the achievable roof SURVEY 8d asks the kernels to be quoted against."""
    c = ctx or context()
    with DeviceRaster.empty((nbytes // 4096, 1024), np.float32, c) as src, \
            DeviceRaster.empty(src.shape, np.float32, c) as dst:
        c.check(c.lib.hdem_copy_rate_dev(c.handle, src.ptr, dst.ptr, src.nbytes))   # warm
        c.synchronize()
        was = c.profile_get(K_COPY)
        c.profile(True)
        for _ in range(reps):
            c.check(c.lib.hdem_copy_rate_dev(c.handle, src.ptr, dst.ptr, src.nbytes))
        now = c.profile_get(K_COPY)
        ms = now["ms"] - was["ms"]
        return 2.0 * (now["units"] - was["units"]) / max(ms, 1e-9) / 1e6


def _destripe_quarter(shape):
    """What the destripe's 55-cell window has to fit: a quadrant less its 10-cell margin."""
    return tuple(max(n // 2 - 10, 0) for n in shape)


def fourier_destripe_dev(dem, out=None, mask=None):
    """DetectApplyFourier on a device raster; ``mask`` (uint8 raster) optionally
    receives the reference's ``masks_fourier`` (shifted coordinates)."""
    _need(dem, np.float32)
    c = dem.ctx
    if mask is not None:
        _need(mask, np.uint8)
    with result_raster(out, dem.shape, np.float32, c) as out:
        c.check(c.lib.hdem_fourier_destripe_f32_dev(
            c.handle, dem.ptr, dem.shape[0], dem.shape[1], out.ptr,
            mask.ptr if mask is not None else None),
            window=55, shape=_destripe_quarter(dem.shape))
    return out


def blanks_fourier_dev(q, found=None, window_size=55):
    """One BlanksFourier pass: returns the byte mask of cells above 4x their hollow
    mean; ``q`` is rewritten with those cells zeroed."""
    return _one_call_dev("hdem_blanks_fourier_f32_dev", q, np.float32, found, np.uint8,
                         int(window_size), window=window_size)


def isolated_points_dev(mask, window_size=3, out=None):
    return _one_call_dev("hdem_isolated_points_u8_dev", mask, np.uint8, out, np.uint8,
                         int(window_size), window=window_size)


def expand_dev(mask, window_size=13, out=None):
    return _one_call_dev("hdem_expand_u8_dev", mask, np.uint8, out, np.uint8,
                         int(window_size), window=window_size)


def fft2_dev(data, inverse=False):
    """In-place 2-D transform of a complex64 or complex128 raster; the inverse is
    unnormalised."""
    c = data.ctx
    if data.dtype == np.complex128:
        fn = c.lib.hdem_fft2_c2c_f64_dev
    else:
        _need(data, np.complex64)
        fn = c.lib.hdem_fft2_c2c_f32_dev
    c.check(fn(c.handle, data.ptr, data.shape[0], data.shape[1], int(bool(inverse))))
    return data


def widened_to_host(raster, dtype):
    """``raster.to_host().astype(dtype)`` with the conversion on the device: the wider array
    crosses the bus at 56 GB/s instead of being written by one host thread at ~10 (the
    reference hands back float64 / int64 where the kernels hold float32 / bytes)."""
    dtype = np.dtype(dtype)
    if raster.dtype == dtype:
        return raster.to_host()
    with elementwise_dev(EW_MUL, raster, 1.0, out_dtype=dtype) as wide:
        return wide.to_host()


def correct_nan_dev(dem, out=None, window_size=3):
    return _one_call_dev("hdem_correct_nan_f32_dev", dem, np.float32, out, np.float32,
                         int(window_size), window=window_size)


def majority_dev(img, window_size=11, out=None):
    return _one_call_dev("hdem_majority_f32_dev", img, np.float32, out, np.float32,
                         int(window_size), window=window_size)


@contextlib.contextmanager
def _scratch(shape, dtype, ctx, wanted=True):
    """A scratch raster for the length of a call (``None`` when not ``wanted``).  ``hdem_free``
    is stream-ordered now: dropping the synchronize in front of it is a speed change of its own."""
    if not wanted:
        yield None
        return
    with DeviceRaster.empty(shape, dtype, ctx) as raster:
        try:
            yield raster
        finally:
            ctx.synchronize()


def _structure_arg(structure):
    if structure is None:
        return None, 0, 0, None
    st = np.ascontiguousarray(np.asarray(structure) != 0, dtype=np.uint8)
    if st.ndim != 2:
        raise ValueError(f"expected a 2-D structure, got shape {st.shape}")
    return st.ctypes.data, st.shape[0], st.shape[1], st


def binary_erosion_dev(mask, iterations=1, structure=None, out=None):
    _need(mask, np.uint8)
    c = mask.ctx
    ptr, sh, sw, _alive = _structure_arg(structure)
    with result_raster(out, mask.shape, np.uint8, c) as out, \
            _scratch(mask.shape, np.uint8, c, iterations > 1) as tmp:
        c.check(c.lib.hdem_binary_erosion_u8_dev(c.handle, mask.ptr, mask.shape[0],
                                                 mask.shape[1], ptr, sh, sw, int(iterations),
                                                 tmp.ptr if tmp else None, out.ptr))
    return out


def binary_closing_dev(mask, structure=None, out=None):
    _need(mask, np.uint8)
    c = mask.ctx
    ptr, sh, sw, _alive = _structure_arg(structure)
    with result_raster(out, mask.shape, np.uint8, c) as out, \
            _scratch(mask.shape, np.uint8, c) as tmp:
        c.check(c.lib.hdem_binary_closing_u8_dev(c.handle, mask.ptr, mask.shape[0],
                                                 mask.shape[1], ptr, sh, sw, tmp.ptr, out.ptr))
    return out


def grey_dilation_dev(img, size, out=None):
    """float32 or float64 raster; the result has the input's type."""
    c = img.ctx
    if img.dtype == np.float64:
        fn = c.lib.hdem_grey_dilation_f64_dev
    else:
        _need(img, np.float32)
        fn = c.lib.hdem_grey_dilation_f32_dev
    sy, sx = (size, size) if np.isscalar(size) else size
    with result_raster(out, img.shape, img.dtype, c) as out:
        c.check(fn(c.handle, img.ptr, img.shape[0], img.shape[1], int(sy), int(sx), out.ptr))
    return out


def tidying_lagoons_dev(img, out=None):
    return _one_call_dev("hdem_tidying_lagoons_f32_dev", img, np.float32, out, np.float32,
                         window=7)


def lagoons_detection_dev(hsheds):
    """(mask uint8, hsheds_nan_fixed, lagoons_values) device rasters."""
    _need(hsheds, np.float32)
    c = hsheds.ctx
    with result_raster(None, hsheds.shape, np.float32, c) as fixed, \
            result_raster(None, hsheds.shape, np.float32, c) as values, \
            result_raster(None, hsheds.shape, np.uint8, c) as mask:
        c.check(c.lib.hdem_lagoons_detection_f32_dev(c.handle, hsheds.ptr, hsheds.shape[0],
                                                     hsheds.shape[1], fixed.ptr, values.ptr,
                                                     mask.ptr), window=11, shape=hsheds.shape)
    return mask, fixed, values


def sinkfill_d8_dev(z, eps=0.0, max_rounds=0, out=None, codes=None, flags=FILL_INIT):
    """Sink fill + D8 of the filled surface (``hdem_sinkfill_d8_f32_dev``).
    Returns (filled raster, D8 raster, stats)."""
    _need(z, np.float32)
    c = z.ctx
    st = FillStats()
    with result_raster(out, z.shape, np.float32, c) as out, \
            result_raster(codes, z.shape, np.uint8, c) as codes:
        c.check(c.lib.hdem_sinkfill_d8_f32_dev(c.handle, z.ptr, z.shape[0], z.shape[1],
                                               float(eps), int(max_rounds), int(flags),
                                               out.ptr, codes.ptr, ctypes.byref(st)))
    return out, codes, st.as_dict()


def boxmean3_dev(x, do_round=True, out=None):
    c = x.ctx
    fn = (c.lib.hdem_boxmean3_f32_dev if x.dtype == np.float32
          else c.lib.hdem_boxmean3_f64_dev)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"box mean needs a float raster, got {x.dtype}")
    with result_raster(out, x.shape, x.dtype, c) as out:
        c.check(fn(c.handle, x.ptr, x.shape[0], x.shape[1], int(bool(do_round)), out.ptr))
    return out


def quadratic_dev(dem, window_size=15, out=None):
    return _one_call_dev("hdem_quadratic_f32_dev", dem, np.float32, out, np.float32,
                         int(window_size), window=window_size)


def groves_dev(img, groves, window_size=15, threshold=1.5, iterations=3, out=None,
               scratch=None):
    """``scratch``: a float32 raster of the same shape for the ping-pong between
    passes (allocated and freed here when not given)."""
    _need(img, np.float32)
    _need(groves, np.uint8)
    c = img.ctx
    if scratch is not None:
        _need(scratch, np.float32)
    with result_raster(out, img.shape, np.float32, c) as out, \
            _scratch(img.shape, np.float32, c, scratch is None and iterations > 1) as mine:
        scratch = scratch or mine
        c.check(c.lib.hdem_groves_f32_dev(c.handle, img.ptr, groves.ptr, img.shape[0],
                                          img.shape[1], int(window_size),
                                          float(threshold), int(iterations),
                                          scratch.ptr if scratch else None, out.ptr),
                window=window_size, shape=img.shape)
    return out


# ---------------------------------------------------------------------------
# host-array operators (what Filter.apply binds): NumPy in, NumPy out
# ---------------------------------------------------------------------------

def _host2d(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    _need2d(a)
    return a


def d8(z):
    c = context()
    z = _host2d(z, np.float32)
    out = host_empty(z.shape, np.uint8)
    c.check(c.lib.hdem_d8_f32(c.handle, z.ctypes.data, z.shape[0], z.shape[1],
                              out.ctypes.data))
    return out


def sinkfill(z, eps=0.0, max_rounds=0, return_stats=False):
    c = context()
    z = _host2d(z, np.float32)
    out = host_empty(z.shape, z.dtype)
    st = FillStats()
    c.check(c.lib.hdem_sinkfill_f32(c.handle, z.ctypes.data, z.shape[0], z.shape[1],
                                    float(eps), int(max_rounds), out.ctypes.data,
                                    ctypes.byref(st)))
    return (out, st.as_dict()) if return_stats else out


def boxmean3(x, do_round=True):
    c = context()
    if np.asarray(x).dtype == np.float32:
        x = _host2d(x, np.float32)
        fn = c.lib.hdem_boxmean3_f32
    else:
        x = _host2d(x, np.float64)
        fn = c.lib.hdem_boxmean3_f64
    out = host_empty(x.shape, x.dtype)
    c.check(fn(c.handle, x.ctypes.data, x.shape[0], x.shape[1], int(bool(do_round)),
               out.ctypes.data))
    return out


def convolve(x, weights):
    """General odd weights: float32 rasters in float32, anything else in float64 -- the
    type scipy.ndimage.convolve works in for a float64 raster (extension_filters.py:183)."""
    c = context()
    if np.asarray(x).dtype == np.float32:
        x, fn = _host2d(x, np.float32), c.lib.hdem_convolve_f32
    else:
        x, fn = _host2d(x, np.float64), c.lib.hdem_convolve_f64
    w = _host2d(weights, np.float64)
    out = host_empty(x.shape, x.dtype)
    c.check(fn(c.handle, x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data, w.shape[0],
               w.shape[1], out.ctypes.data))
    return out


def around(x):
    """``np.around(x)``: float32 and float64 on the device (other floats as float64); an
    integer or bool array has nothing to round and comes back as ``np.around`` returns it."""
    if np.asarray(x).dtype.kind in "iub":
        return np.around(x)
    c = context()
    if np.asarray(x).dtype == np.float32:
        a, fn = np.ascontiguousarray(x, dtype=np.float32), c.lib.hdem_around_f32
    else:
        a, fn = np.ascontiguousarray(x, dtype=np.float64), c.lib.hdem_around_f64
    out = host_empty(a.shape, a.dtype)
    if a.size:
        c.check(fn(c.handle, a.ctypes.data, a.size, out.ctypes.data))
    return out


def quadratic(dem, window_size=15):
    c = context()
    dem = _host2d(dem, np.float32)
    out = host_empty(dem.shape, dem.dtype)
    c.check(c.lib.hdem_quadratic_f32(c.handle, dem.ctypes.data, dem.shape[0],
                                     dem.shape[1], int(window_size), out.ctypes.data),
            window=window_size, shape=dem.shape)
    return out


def fourier_destripe(dem, return_mask=False):
    c = context()
    dem = _host2d(dem, np.float32)
    out = host_empty(dem.shape, dem.dtype)
    mask = host_empty(dem.shape, np.uint8) if return_mask else None
    c.check(c.lib.hdem_fourier_destripe_f32(c.handle, dem.ctypes.data, dem.shape[0],
                                            dem.shape[1], out.ctypes.data,
                                            mask.ctypes.data if return_mask else None),
            window=55, shape=_destripe_quarter(dem.shape))
    return (out, mask) if return_mask else out


def blanks_fourier(q, window_size=55):
    """(found float64 0/1, q * (1 - found)) like BlanksFourier.apply."""
    with DeviceRaster.from_host(_host2d(q, np.float32)) as qd, \
            blanks_fourier_dev(qd, window_size=window_size) as found:
        return widened_to_host(found, np.float64), qd.to_host()


def isolated_points(mask, window_size=3):
    with DeviceRaster.from_host(_host2d(mask, np.uint8)) as m, \
            isolated_points_dev(m, window_size) as out:
        return out.to_host()


def expand(mask, window_size=13, dtype=np.uint8):
    """ExpandFilter on a host raster (cells > 0 are set); the 0 / 1 result in ``dtype``."""
    g = np.asarray(mask)
    set_ = _host2d(g, g.dtype) if g.dtype in (np.uint8, np.bool_) else \
        _host2d(np.greater(g, 0), np.bool_)
    with DeviceRaster.from_host(set_.view(np.uint8)) as m, expand_dev(m, window_size) as out:
        return widened_to_host(out, dtype)


def fft2(x, inverse=False):
    """fft2 / ifft2 (normalised) of a 2-D array: complex64 for float32 / complex64 input,
    complex128 for anything else -- scipy.fftpack's rule (extension_filters.py:379,414)."""
    single = np.asarray(x).dtype in (np.dtype(np.float32), np.dtype(np.complex64))
    a = _host2d(x, np.complex64 if single else np.complex128)
    with DeviceRaster.from_host(a) as data:
        d = fft2_dev(data, inverse).to_host()
    if not inverse:
        return d
    return d / (np.float32(a.size) if single else np.float64(a.size))


def mask_bytes(groves_class):
    """The class raster as the bytes the groves kernel reads (non-zero = grove).  One-byte
    dtypes go as they are -- at 16384^2 a ``!= 0`` and an ``astype`` are 100 ms of NumPy
    in front of 2 ms of kernels."""
    g = np.asarray(groves_class)
    if g.dtype in (np.uint8, np.bool_, np.int8):
        return _host2d(g, g.dtype).view(np.uint8)
    return _host2d(np.not_equal(g, 0), np.bool_).view(np.uint8)


def groves(img, groves_class, window_size=15, threshold=1.5, iterations=1):
    c = context()
    img = _host2d(img, np.float32)
    g = mask_bytes(groves_class)
    if g.shape != img.shape:
        raise ValueError(f"groves class shape {g.shape} != image shape {img.shape}")
    out = host_empty(img.shape, img.dtype)
    c.check(c.lib.hdem_groves_f32(c.handle, img.ctypes.data, g.ctypes.data,
                                  img.shape[0], img.shape[1], int(window_size),
                                  float(threshold), int(iterations), out.ctypes.data),
            window=window_size, shape=img.shape)
    return out


__all__ = [n for n in dir() if not n.startswith("_")]
_ = HydroDEMException  # re-exported for callers that catch the base class
