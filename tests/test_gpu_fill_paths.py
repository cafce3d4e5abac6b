"""
The paths through the sink-fill driver (hdem_sinkfill.hip), one small raster each: which
kernels a call launches -- its own and those of the fills nested in it: the coarse pre-solve,
the hub raster's fill and that raster's own hub start -- whether it converges without rounds,
and that every path ends in the bits of the C priority flood.  The launch counts are the
driver's as it stood before it was split into phases; a change of the driver that moves one
of them has changed what a call does on the stream.

The raster is 130 x 190: 3 x 4 tiles of 62, partial in both directions, so its hub raster is
7 x 9 (one tile) and that raster's own hub raster 3 x 3 (one cell of interior).
"""
import numpy as np
import pytest

from hydrodem_amd import backend
import oracle
from oracle import c_oracle

pytestmark = pytest.mark.gpu

KERNELS = ("K_FILL_INIT", "K_FILL_HUB", "K_FILL_COARSE", "K_FILL_TILE", "K_FILL_FLAT",
           "K_FILL_ROUND")
HUB = {"HDEM_HUB_MIN_TILES": "1"}
HUB_NESTED = {"HDEM_HUB_MIN_TILES": "1", "HDEM_HUB_MIN_TILES_NESTED": "1"}
FILL_ENV = ("HDEM_HUB_MIN_TILES", "HDEM_HUB_MIN_TILES_NESTED", "HDEM_FILL_HUB",
            "HDEM_COARSE_MIN_CELLS", "HDEM_FILL_TEST_BUDGET_US")

# row: (environment, eps, flags, launches INIT / HUB / COARSE / TILE / FLAT / ROUND -- None: not
# pinned, it depends on the raster --, rounds == 0)
ROWS = {
    "plain": ({}, 0.0, backend.FILL_INIT, (1, 0, 0, 1, 1, 1), True),
    "hub": (HUB, 0.0, backend.FILL_INIT, (1, 1, 1, 1, 2, 1), True),     # (INIT: of the hub raster)
    "hub_nested": (HUB_NESTED, 0.0, backend.FILL_INIT, (1, 2, 2, 1, 3, 1), True),
    "own_coarse": ({"HDEM_FILL_HUB": "0", "HDEM_COARSE_MIN_CELLS": "1"}, 0.0, backend.FILL_INIT,
                   (2, 0, 1, 1, 2, 1), True),
    "eps": ({}, 1e-3, backend.FILL_INIT, (1, 0, 0, 1, 0, 1), True),
    "sync_only": ({}, 0.0, backend.FILL_SYNC_ONLY, (1, 0, 0, 0, 0, None), False),
    # the launch is cut before its first visit: the certifying stream finds work, rounds finish
    "cut_short": ({"HDEM_FILL_TEST_BUDGET_US": "0"}, 0.0, backend.FILL_INIT,
                  (1, 0, 0, 1, 1, None), False),
}


@pytest.fixture(scope="module", autouse=True)
def _lib(built):
    assert backend.device_count() >= 1, "these tests need a GPU"
    yield


@pytest.fixture(scope="module")
def base():
    """{eps: (raster, filled oracle, its D8 oracle)}, made once and left alone."""
    z = oracle.synth_dem(130, 190, variant="rough")
    z[65, 95] = np.nan
    out = {}
    for eps in (0.0, 1e-3):
        want = c_oracle.sinkfill_pflood(z, eps=eps)
        out[eps] = (z, want, c_oracle.d8(want))
    return out


def set_env(monkeypatch, env):
    for name in FILL_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def profiled(call):
    """(what ``call`` returns, {kernel: launches}) with the profile reset in front of it."""
    ctx = backend.context()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        got = call()
        launches = {k: ctx.profile_get(getattr(backend, k))["launches"] for k in KERNELS}
    finally:
        ctx.profile(False)
    return got, launches


@pytest.mark.parametrize("row", list(ROWS))
def test_fill_path_launches_and_bits(monkeypatch, base, row):
    env, eps, flags, expected, no_rounds = ROWS[row]
    z, want, want_d8 = base[eps]
    set_env(monkeypatch, env)
    with backend.DeviceRaster.from_host(z) as zd:
        (wd, cd, st), launches = profiled(
            lambda: backend.sinkfill_d8_dev(zd, eps=eps, flags=flags))
        with wd, cd:
            filled, codes = wd.to_host(), cd.to_host()
    print(row, launches, {k: st[k] for k in ("converged", "rounds", "tile_visits")})
    for kernel, n in zip(KERNELS, expected):
        if n is not None:
            assert launches[kernel] == n, (kernel, launches)
    assert st["tiles"] == 12 and st["converged"]
    if no_rounds:
        assert st["rounds"] == 0
    else:
        assert st["rounds"] > 0 and launches["K_FILL_ROUND"] > 0
    assert np.array_equal(filled, want, equal_nan=True)
    assert np.array_equal(codes, want_d8)


def test_plain_fill_after_a_nested_d8_fill(monkeypatch, base):
    """The D8 request and the nesting of one call are gone when it returns: the next call of
    the context, of another raster and without codes, fills right and leaves the first
    call's codes alone."""
    z, want, want_d8 = base[0.0]
    other = oracle.synth_dem(97, 150, variant="srtm")
    want_other = c_oracle.sinkfill_pflood(other)
    set_env(monkeypatch, HUB_NESTED)
    with backend.DeviceRaster.from_host(z) as zd, backend.DeviceRaster.from_host(other) as od:
        (wd, cd, st), launches = profiled(lambda: backend.sinkfill_d8_dev(zd))
        assert launches["K_FILL_HUB"] == 2 and st["converged"]
        set_env(monkeypatch, {})
        (wo, st2), launches2 = profiled(lambda: backend.sinkfill_dev(od))
        print(launches, launches2)
        with wd, cd, wo:
            assert [launches2[k] for k in KERNELS] == [1, 0, 0, 1, 1, 1]
            assert st2["converged"] and st2["rounds"] == 0
            assert np.array_equal(wo.to_host(), want_other, equal_nan=True)
            assert np.array_equal(wd.to_host(), want, equal_nan=True)
            assert np.array_equal(cd.to_host(), want_d8)


def test_resume_after_a_nested_fill(monkeypatch, base):
    """A nested pre-solve leaves no resume state of its own behind: WARM | RESUME on the
    pair the nested call filled converges to the same bits."""
    z, want, _ = base[0.0]
    set_env(monkeypatch, HUB_NESTED)
    with backend.DeviceRaster.from_host(z) as zd, \
            backend.DeviceRaster.empty(z.shape, np.float32) as wd:
        (_, st), launches = profiled(lambda: backend.sinkfill_dev(zd, out=wd))
        assert launches["K_FILL_HUB"] == 2 and st["converged"]
        (_, st2), launches2 = profiled(lambda: backend.sinkfill_dev(
            zd, out=wd, flags=backend.FILL_WARM | backend.FILL_RESUME))
        print(launches, launches2, st2)
        assert st2["converged"] and st2["pending"] == 0 and st2["async_timed_out"] == 0
        # WARM: no start values are written, so no nested fill either; the first call ended
        # in a certifying pass, which leaves no worklist: every tile is due once, and the
        # resumed call trusts its launch
        assert [launches2[k] for k in KERNELS] == [0, 0, 0, 1, 1, 0]
        assert st2["tile_visits"] == st2["tiles"] == 12 and st2["rounds"] == 0
        assert np.array_equal(wd.to_host(), want, equal_nan=True)
