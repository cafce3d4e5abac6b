"""
The terrain operators on the GPU in every elevation regime of tests/elevation_regimes.py:
below sea level, across zero, at 8000 m where an ulp is of the size of epsilon, relief of
millimetres and of 1e-29, elevations of 1e32, elevations on both sides of the hub raster's
3.0e38 wall constant, and a ladder of single ulps -- plus the D8 tie rasters.  Every comparison
is ``np.array_equal`` against the CPU references that tests/test_elevation_regimes.py holds
to each other; there is no tolerance in this file.

  a  the exact fill with D8 from every start (default, hub graph, block-maximum pre-solve,
     round driver alone), and the hub / coarse start values as upper bounds of the fill;
  b  the gradient fill on the default path and from the epsilon-coarse start;
  c  lakes that take the flat path (one gap, three gaps, a second fill into the same output);
  d  D8 alone and fused with the fill on the tie patterns, also one column off alignment;
  e  ResolveFlats, HeightAboveDrainage / FlowDistance and the depression inventory;
  f  the row-block partition's own hub start (partition.hub_start's copy of the wall constant).

The epsilon-coarse start needs elevations whose doubled magnitude is finite: for ``near_max``
the fill falls back to the +inf start (hdem_sinkfill.hip), and that regime runs on 200 x 333
there because ``synth_dem(333, 1100)`` reaches 115.6 m, which times 3.0e36 is past FLT_MAX.
"""
import numpy as np
import pytest

import hydrodem_amd as hd
from hydrodem_amd import backend
from oracle import c_oracle
import elevation_regimes as er
from test_flats import resolve_flats_bfs
from test_flowacc import acc_kahn
from test_flowtrace import distance_of, hand_of, trace_walk
from test_gpu_depressions import assert_table, check
from test_gpu_parity import _crater

pytestmark = pytest.mark.gpu

SHAPE = (200, 333)                 # 4 x 6 tiles of 62, partial tiles on both edges
COARSE_SHAPE = (333, 1100)
DOWNSTREAM = ("below_sea", "zero_cross", "high_8000", "huge_1e30", "near_max")
CASES = [(name, variant) for name in er.REGIMES for variant in er.VARIANTS]
# start: (environment, flags, the kernel that must have been launched)
STARTS = {
    "default": ({}, backend.FILL_INIT, None),
    "hub": ({"HDEM_HUB_MIN_TILES": "1"}, backend.FILL_INIT, backend.K_FILL_HUB),
    "coarse": ({"HDEM_COARSE_MIN_CELLS": "1", "HDEM_FILL_HUB": "0"}, backend.FILL_INIT,
               backend.K_FILL_COARSE),
    "rounds": ({}, backend.FILL_SYNC_ONLY, None),
}


@pytest.fixture(scope="module", autouse=True)
def _lib(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


def fill_d8(z, eps=0.0, flags=backend.FILL_INIT, kernel=None):
    """(filled, codes, stats, launches of ``kernel``) of one fused call."""
    ctx = backend.context()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        with backend.DeviceRaster.from_host(z) as zd:
            wd, cd, st = backend.sinkfill_d8_dev(zd, eps=eps, flags=flags)
            with wd, cd:
                got = wd.to_host(), cd.to_host()
        launches = ctx.profile_get(kernel)["launches"] if kernel is not None else None
    finally:
        ctx.profile(False)
    return got[0], got[1], st, launches


def start_values(z, eps, monkeypatch):
    """What the fill starts from: the relaxation cut before its first visit, no certifying
    pass."""
    monkeypatch.setenv("HDEM_FILL_TEST_BUDGET_US", "0")
    with backend.DeviceRaster.from_host(z) as zd:
        ud, _ = backend.sinkfill_dev(zd, eps=eps, flags=backend.FILL_INIT | backend.FILL_NO_VERIFY)
        with ud:
            u = ud.to_host()
    monkeypatch.delenv("HDEM_FILL_TEST_BUDGET_US")
    return u


def assert_bounds(u, want):
    with np.errstate(invalid="ignore"):
        ok = np.isnan(want) | (u >= want)
    assert ok.all(), f"{int((~ok).sum())} start values below the fill"


# ---------------------------------------------------------------------------
# a. the exact fill from every start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name,variant", CASES)
def test_the_exact_fill_from_every_start(monkeypatch, name, variant, start):
    env, flags, kernel = STARTS[start]
    z, want, want_d8 = er.regime_fill(name, SHAPE, variant, variant == "rough")
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    got, codes, st, launches = fill_d8(z, 0.0, flags, kernel)
    assert st["converged"] == 1 and st["async_timed_out"] == 0
    if kernel == backend.K_FILL_HUB:
        assert launches == 1
    elif kernel is not None:
        assert launches >= 1
    if start == "rounds":
        assert st["rounds"] >= 1
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(codes, want_d8)
    if kernel is not None:
        assert_bounds(start_values(z, 0.0, monkeypatch), want)


# ---------------------------------------------------------------------------
# b. the gradient fill
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-3, 1e-4])
@pytest.mark.parametrize("name,variant", CASES)
def test_the_gradient_fill_on_the_default_path(name, variant, eps):
    z, want, want_d8 = er.regime_fill(name, SHAPE, variant, variant == "rough", eps)
    got, codes, st, _ = fill_d8(z, eps)
    assert st["converged"] == 1 and st["async_timed_out"] == 0
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(codes, want_d8)


@pytest.mark.parametrize("eps", [1e-3, 1e-4])
@pytest.mark.parametrize("name", er.RASTERS)
def test_the_gradient_fill_from_the_coarse_start(monkeypatch, name, eps):
    """The rounding allowance of the coarse start is sized by twice the largest block maximum
    under the 3.0e38 wall.  In ``near_max`` every block holds a cell above the wall, the whole
    coarse raster is walls and the allowance is that of 1 m; ``near_max_basin`` has block
    maxima of 2.3e38 ... 2.6e38, twice that is no float32, the allowance has no finite value
    and the fill starts from +inf instead (it used to hand a NaN epsilon to the pre-solve and
    fail with "eps must be >= 0, got nan")."""
    shape = SHAPE if name.startswith("near_max") else COARSE_SHAPE
    z, want, want_d8 = er.regime_fill(name, shape, "rough", True, eps)
    monkeypatch.setenv("HDEM_COARSE_MIN_CELLS", "1")
    monkeypatch.setenv("HDEM_FILL_EPS_COARSE", "1")
    got, codes, st, launches = fill_d8(z, eps, kernel=backend.K_FILL_COARSE)
    assert st["converged"] == 1 and st["async_timed_out"] == 0
    assert launches == (0 if name == "near_max_basin" else 1)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(codes, want_d8)
    assert_bounds(start_values(z, eps, monkeypatch), want)


# ---------------------------------------------------------------------------
# c. lakes on the flat path
# ---------------------------------------------------------------------------
CRATER = 400                       # the smallest size tried; the lake is 5 tiles across
GAPS = {"one_gap": ((0.5, 33.0),), "three_gaps": ((0.2, 36.0), (0.5, 34.0), (0.8, 31.5))}


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("name", ["below_sea", "high_8000", "near_max"])
def test_a_lake_takes_the_flat_path_and_stays_exact(monkeypatch, name, gaps):
    """(The rim stands at 105 m so that ``near_max`` puts it above 3.0e38 and the lake below.)"""
    monkeypatch.setenv("HDEM_FILL_HUB", "0")           # from +inf: the lake finds its level by visits
    z = er.REGIMES[name](_crater(CRATER, 105.0, GAPS[gaps]))
    assert z.dtype == np.float32 and np.isfinite(z).all()
    want = c_oracle.sinkfill_pflood(z)
    assert ((want > z).sum()) > 16 * er.TILE * er.TILE   # there is a lake, tiles wide
    with backend.DeviceRaster.from_host(z) as zd:
        wd, cd, st = backend.sinkfill_d8_dev(zd)
        with wd, cd:
            assert st["converged"] == 1 and st["async_timed_out"] == 0
            assert np.array_equal(wd.to_host(), want)
            assert np.array_equal(cd.to_host(), c_oracle.d8(want))
            assert st["visits_flat"] > 0
            # stale interiors of flat tiles from the first call must not leak into the second
            _, st2 = backend.sinkfill_dev(zd, out=wd)
            assert st2["converged"] == 1
            assert np.array_equal(wd.to_host(), want)


# ---------------------------------------------------------------------------
# d. D8 ties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("base", er.TIE_BASES)
def test_d8_gives_a_float32_tie_to_the_first_neighbour_in_window_order(base, shift):
    z, rows, cols, expected = er.d8_tie_raster(base)
    if shift:
        z, rows, cols = er.shifted_right(z, rows, cols, base)
    with backend.DeviceRaster.from_host(z) as zd, backend.d8_dev(zd) as cd:
        got = cd.to_host()
    assert np.array_equal(got[rows, cols], expected)
    assert np.array_equal(got, c_oracle.d8(z))
    assert np.array_equal(hd.D8FlowDirection().apply(z), got)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("base", er.TIE_BASES)
def test_the_fused_fill_and_d8_keep_the_strip_and_its_ties(base, shift):
    z, rows, cols, expected = er.d8_tie_strip(base)
    if shift:
        z, rows, cols = er.shifted_right(z, rows, cols, base)
    for eps in (0.0, 1e-3):
        want = c_oracle.sinkfill_pflood(z, eps=eps)
        got, codes, st, _ = fill_d8(z, eps)
        assert st["converged"] == 1
        assert np.array_equal(got, z)                   # its own fill
        if eps == 0.0:
            assert np.array_equal(codes[rows, cols], expected)
        assert np.array_equal(codes, c_oracle.d8(want))


# ---------------------------------------------------------------------------
# e. the operators behind the fill
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", er.VARIANTS)
@pytest.mark.parametrize("name", DOWNSTREAM)
def test_resolve_flats_on_the_exact_fill(name, variant):
    _, filled, codes = er.regime_fill(name, SHAPE, variant, variant == "rough")
    want_out, want_dist = resolve_flats_bfs(filled, codes)
    op = hd.ResolveFlats(dem=np.array(filled), keep_partial_results=True)
    out = op.apply(np.array(codes))
    assert out.dtype == np.uint8 and np.array_equal(out, want_out)
    assert op.distance.dtype == np.uint32 and np.array_equal(op.distance, want_dist)


@pytest.mark.parametrize("variant", er.VARIANTS)
@pytest.mark.parametrize("name", DOWNSTREAM)
def test_hand_and_flow_distance_on_the_gradient_fill(name, variant):
    _, filled, codes = er.regime_fill(name, SHAPE, variant, variant == "rough", 1e-3)
    filled, codes = np.array(filled), np.array(codes)
    acc = acc_kahn(codes).astype(np.uint32)
    # (where epsilon vanishes in one ulp the integer-metre fill is all flats and no cell
    # gathers 20: the largest accumulation there is then is the stream)
    threshold = max(2, min(20, int(acc.max())))
    stop, ncard, ndiag = trace_walk(codes, acc >= threshold)
    assert stop.any()                                   # some cell does reach a stream
    op = hd.HeightAboveDrainage(dem=filled, streams=acc, threshold=threshold, cellsize=30,
                                keep_partial_results=True)
    hand = op.apply(codes)
    want_distance = distance_of(stop, ncard, ndiag, 30)
    assert hand.dtype == np.float32
    assert np.array_equal(hand, hand_of(stop, filled), equal_nan=True)
    assert np.array_equal(op.drainage, stop)
    assert np.array_equal(op.distance, want_distance, equal_nan=True)
    distance = hd.FlowDistance(acc, threshold=threshold, cellsize=30).apply(codes)
    assert distance.dtype == np.float32
    assert np.array_equal(distance, want_distance, equal_nan=True)


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("variant", er.VARIANTS)
@pytest.mark.parametrize("name", DOWNSTREAM)
def test_the_depression_inventory(name, variant, eps):
    z, filled, _ = er.regime_fill(name, SHAPE, variant, variant == "rough", eps)
    z = np.array(z)
    inventory = hd.DepressionInventory(epsilon=eps, cellsize=30)
    labels = inventory.apply(z)
    assert np.array_equal(inventory.filled, filled, equal_nan=True)
    want, count, table, _ = check(z, inventory.filled, cellsize=30)
    assert count >= 1                                   # (of the reference: a real input)
    assert np.array_equal(labels, want) and inventory.count == count
    assert_table(inventory.table, table)
    if eps == 0.0:
        assert np.array_equal(table["level"], inventory.filled.ravel()[table["first"]])


# ---------------------------------------------------------------------------
# f. the partition's hub start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["below_sea", "near_max"])
def test_virtual_rank_partition_from_its_hub_start(name):
    """tests/test_gpu_parity.py::test_virtual_rank_partition_on_hip with every block started
    from partition.hub_start (ONE hub graph over the blocks, its walls at partition.HUB_BIG):
    fill and D8 of the blocks equal those of the undivided raster."""
    import torch
    from hydrodem_amd import partition as P
    world, (H, W) = 3, (260, 330)
    z, want, want_d8 = er.regime_fill(name, (H, W))

    def first_solve(rank, comm):
        g0, g1, top, bot = P.local_range(rank, world, H)
        zt = torch.from_numpy(z[g0:g1].copy()).cuda()
        block = {"z": zt, "w": torch.empty_like(zt), "top": top, "bot": bot,
                 "solver": P.HipLocalSolver(0, turn=comm.gpu_turn)}
        flags = (backend.FILL_GHOST_TOP if top else 0) | (backend.FILL_GHOST_BOTTOM if bot else 0)
        levels = P.hub_start(zt, block["w"], comm, block["solver"], flags, 1)
        block["solver"].fill(zt, block["w"], 0.0, backend.FILL_INIT | flags
                             | backend.FILL_GHOST_GIVEN | backend.FILL_NO_VERIFY)
        torch.cuda.synchronize()
        del levels                                      # (alive until the solve has consumed them)
        return block

    blocks = P.ThreadWorld(world).run(first_solve)
    try:
        for _ in range(1000):
            torch.cuda.synchronize()
            sends = [(b["w"][1].clone(), b["w"][-2].clone()) for b in blocks]
            any_changed = False
            for r, b in enumerate(blocks):
                flags = backend.FILL_WARM
                if b["top"]:
                    new = sends[r - 1][1]
                    if not torch.equal(new, b["w"][0]):
                        b["w"][0].copy_(new)
                        flags |= backend.FILL_ACT_TOP
                if b["bot"]:
                    new = sends[r + 1][0]
                    if not torch.equal(new, b["w"][-1]):
                        b["w"][-1].copy_(new)
                        flags |= backend.FILL_ACT_BOTTOM
                if flags != backend.FILL_WARM:
                    any_changed = True
                    torch.cuda.synchronize()
                    b["solver"].fill(b["z"], b["w"], 0.0, flags | backend.FILL_NO_VERIFY)
            if not any_changed:
                break
        torch.cuda.synchronize()
        got = np.concatenate([b["w"][P.owned_slice(r, world)].cpu().numpy()
                              for r, b in enumerate(blocks)])
        assert np.array_equal(got, want)
        codes = []
        for r, b in enumerate(blocks):
            d = P.d8_distributed(b["w"], b["solver"])
            torch.cuda.synchronize()
            codes.append(d[P.owned_slice(r, world)].cpu().numpy())
        assert np.array_equal(np.concatenate(codes), want_d8)
    finally:
        for b in blocks:
            b["solver"].ctx.close()
