"""
The final assembly of the reference's orchestration, device resident.

`hydro_dem_process.py:60-91` (``_prepare_final_terms``) and `:147-149` combine the three
branches with the element-wise filters and smooth the sum:

    mask_rivers_lagoons = AdditionFilter(addend=lagoons.mask_lagoons).apply(rivers)
    not_rivers_lagoons  = SubtractionFilter(minuend=1).apply(mask_rivers_lagoons)
    first_term          = ProductFilter(factor=srtm).apply(not_rivers_lagoons)
    third_term          = ProductFilter(factor=lagoons.hsheds_nan_fixed).apply(rivers)
    dem_complete        = first_term + lagoons.lagoons_values + third_term
    final_dem           = PostProcessingFinal().apply(dem_complete)

Called like that -- unchanged, through the drop-in package -- every ``apply`` is a host
array in, a host array out.  :func:`final_dem` is the same sequence of the same filter
objects on device rasters (``apply_device``): each input goes up once, the eight
operators run in HBM, the result comes down once.  The arithmetic and the types are the
reference's: the masks count as the int64 grids the orchestration holds there (``mask * 1``,
the XOR of the clip), so the complement is int64 and both products are float64 whatever
the elevations' float type (float32 * int64 promotes).  The result is bit for bit the
reference's (`tests/golden/assembly.npz`, tests/test_gpu_elementwise.py).
"""

import contextlib

import numpy as np

from . import backend
from .filters.custom_filters import PostProcessingFinal
from .filters.simple_filters import AdditionFilter, ProductFilter, SubtractionFilter


def _mask(a):
    """A 0 / 1 grid of any type as the bytes that stand for the reference's int64 mask."""
    a = np.asarray(a)
    return a.astype(np.uint8) if a.dtype != np.uint8 else a


def _elevations(a):
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def final_dem(srtm, mask_lagoons, hsheds_nan_fixed, lagoons_values, rivers, ctx=None,
              keep_terms=False):
    """``final_dem`` of `hydro_dem_process.py:147-149` from the results of the three
    branches: ``srtm`` (`image_srtm.py:199`), ``lagoons.mask_lagoons`` /
    ``.hsheds_nan_fixed`` / ``.lagoons_values`` (`custom_filters.py:656-660`) and ``rivers``
    (`image_hsheds.py:203-205`), host arrays; the masks are 0 / 1 grids (bool, uint8 or
    int64) and are read as int64.  Returns the host array the reference returns (float64,
    also for float32 elevations); with ``keep_terms`` also the three terms."""
    with contextlib.ExitStack() as stack:
        own = stack.enter_context               # every raster made here goes on leaving
        up = lambda a: own(backend.DeviceRaster.from_host(a, ctx=ctx))      # noqa: E731
        d_srtm, d_hs = up(_elevations(srtm)), up(_elevations(hsheds_nan_fixed))
        d_values = up(_elevations(lagoons_values))
        d_lagoons, d_rivers = up(_mask(mask_lagoons)), up(_mask(rivers))
        both = own(AdditionFilter(addend=d_lagoons).apply_device(d_rivers))
        neither = own(SubtractionFilter(minuend=1).apply_device(both))
        first = own(ProductFilter(factor=d_srtm).apply_device(neither))
        third = own(ProductFilter(factor=d_hs).apply_device(d_rivers))
        partial = own(AdditionFilter(addend=first).apply_device(d_values))
        complete = own(AdditionFilter(addend=partial).apply_device(third))
        result = own(PostProcessingFinal().apply_device(complete))
        out = result.to_host()
        if keep_terms:
            return out, (first.to_host(), d_values.to_host(), third.to_host())
        return out
