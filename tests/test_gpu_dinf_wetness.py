"""
``DemToDInfWetness`` on the MI355X: the chain DEM -> fill -> D-infinity direction -> (weighted)
D-infinity area -> wetness index on a 1024^2 ``synth_dem`` "rough", against the references applied
stage by stage to the chain's own kept partial results, as tests/test_gpu_dinf.py does for
``DemToDInfArea``.  The area is byte-equal; ``twi`` is inside the bar of
tests/test_gpu_terrain_attributes.py (N = 6, floor 1).  The direction and the two accumulation
references are made once per fill and shared by the cases.
"""
import functools

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, dinf
from hydrodem_amd.backend import DeviceRaster
from test_dinf import accumulate_ref, counts_of, direction_ref, value_of
from test_dinfsum import accumulate_weighted_ref, area_reference
from test_gpu_dinf import schedule_free
from test_gpu_terrain_area import assert_twi

pytestmark = pytest.mark.gpu

F32 = np.float32
CELL, MIN_SLOPE, FRAC_BITS = 30.0, 1e-3, 16
FILLS = [("keep", 1e-3), ("resolve", 0.0)]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


@functools.lru_cache(maxsize=None)
def rough_1024():
    z = hdem_synth.synth_dem(1024, 1024, variant="rough")
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def rain():
    """float32 weights in [0, 2) with dry cells and NaN; quantised at 16 bits they sum to about
    2^37, far below 2^48."""
    rng = np.random.default_rng(1024)
    w = (rng.random((1024, 1024)) * 2).astype(F32)
    w[rng.random(w.shape) < 0.05] = 0.0
    w[rng.random(w.shape) < 0.01] = np.nan
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def stages(flats, epsilon):
    """The chain's own fill and codes (from one run with everything kept) and the references on
    them: words, D-infinity slope, the unweighted and the weighted sum."""
    chain = hd.DemToDInfWetness(epsilon=epsilon, flats=flats, cellsize=CELL,
                                keep_partial_results=True)
    chain.apply(rough_1024())
    words, _, slope, taken = direction_ref(chain.filled, CELL, CELL, fallback=chain.codes)
    q = dinf.quantise(rain(), FRAC_BITS)
    return {"filled": chain.filled, "codes": chain.codes, "words": words, "slope": slope,
            "taken": taken, "sum": accumulate_ref(words, FRAC_BITS),
            "wsum": accumulate_weighted_ref(words, q), "total": int(q.sum())}


@pytest.mark.parametrize("slope", hd.DemToDInfWetness.SLOPES)
@pytest.mark.parametrize("weighted", [False, True], ids=["cells", "rain"])
@pytest.mark.parametrize("flats,epsilon", FILLS)
def test_the_chain_on_1024_against_the_reference_on_its_own_stages(flats, epsilon, weighted, slope):
    want = stages(flats, epsilon)
    chain = hd.DemToDInfWetness(epsilon=epsilon, flats=flats, cellsize=CELL, slope=slope,
                                weights=rain() if weighted else None, min_slope=MIN_SLOPE,
                                keep_partial_results=True)
    twi = chain.apply(rough_1024())
    assert twi.dtype == F32 and chain.filled.dtype == F32 and chain.codes.dtype == np.uint8
    assert chain.filled.tobytes() == want["filled"].tobytes()
    assert chain.codes.tobytes() == want["codes"].tobytes()
    assert np.array_equal(chain.words, want["words"])
    total = want["wsum"] if weighted else want["sum"]
    assert chain.area.tobytes() == value_of(total, FRAC_BITS).tobytes()        # byte-equal
    stage = "WeightedDInfFlowAccumulation" if weighted else "DInfFlowAccumulation"
    assert set(chain.stats) - {"ResolveFlats"} == {"SinkFill", "DInfFlowDirection", stage,
                                                  "AreaWetnessIndex"}
    assert ("ResolveFlats" in chain.stats) == (flats == "resolve")
    assert chain.stats["DInfFlowDirection"]["fallback_cells"] == want["taken"]
    assert schedule_free(chain.stats[stage]) == counts_of(want["words"])
    if weighted:
        assert chain.stats[stage]["total"] == want["total"]
        assert chain.stats[stage]["nan_weights"] == int(np.isnan(rain()).sum())
        assert int(total[want["words"] >> 16 == 0].sum()) == want["total"]
    if slope == "dinf":
        assert chain.dinf_slope.tobytes() == want["slope"].tobytes()
    else:
        assert chain.dinf_slope is None
    ref = area_reference(chain.filled, chain.area, CELL, CELL, 1.0, MIN_SLOPE,
                         chain.dinf_slope if slope == "dinf" else None)
    seen = assert_twi(twi, ref["twi"], np.ones(twi.shape, bool), (flats, weighted, slope))
    print(f"\nDemToDInfWetness {flats} {'rain' if weighted else 'cells'} {slope}: twi {seen:.3f}")
    assert {k: v for k, v in chain.stats["AreaWetnessIndex"].items() if k != "ms_total"} == \
        ref["stats"]
    assert ref["stats"]["floored_cells"] > 0


@pytest.mark.parametrize("flats,epsilon", FILLS)
def test_the_device_form_hands_over_what_it_keeps_and_nothing_else(flats, epsilon):
    want = stages(flats, epsilon)
    kept = hd.DemToDInfWetness(epsilon=epsilon, flats=flats, cellsize=CELL,
                               keep_partial_results=True)
    plain = hd.DemToDInfWetness(epsilon=epsilon, flats=flats, cellsize=CELL)
    with DeviceRaster.from_host(rough_1024(), dtype=F32) as dz:
        twi = kept.apply_device(dz)
        rasters = [twi, kept.filled, kept.codes, kept.words, kept.area, kept.dinf_slope]
        assert all(isinstance(r, DeviceRaster) and r.ptr for r in rasters)
        assert kept.area.to_host().tobytes() == value_of(want["sum"], FRAC_BITS).tobytes()
        first = twi.to_host()
        for raster in rasters:
            raster.free()
        with plain.apply_device(dz) as again:
            assert again.dtype == F32 and again.to_host().tobytes() == first.tobytes()
    for name in hd.DemToDInfWetness.KEPT:
        assert getattr(plain, name) is None
