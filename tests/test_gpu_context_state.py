"""
What a context was told, or left holding, by the calls before this one.

The other GPU tests vary what an operator is given (values, sizes, windows, alignment), what its
scratch holds (tests/test_gpu_scribble.py) and where it runs (tests/test_gpu_streams.py).  Here
the variable is the history of the context.  The sink fill is the one operator whose result
depends on it: ``hdem_ctx`` carries a prepared hub start (``hdem_fill_hub_prepare_dev``), hub
levels and a coarse start "for the next fill" (``hdem_set_fill_hub_levels``,
``hdem_set_fill_coarse_start``) and a resumable worklist, each set by one C call and used by a
later one; and ``hdem_trim`` may come between any two calls of any operator.

Every context is a fresh ``B.Context()`` closed in a ``finally``; every comparison is byte
equality with the C oracle or with the same calls on a fresh context.

a.  ``hdem_trim`` after every step of the hub protocol (prepare, raster, the raster's fill,
    levels, fill).  The trimmed runs are made under scribble byte 0xFF, so that a buffer that
    was freed and allocated again does not come back with its old bytes by luck.
b.  A preparation that another fill's own hub start, or another preparation, has written over:
    ``hdem_fill_hub_raster_dev`` refuses.  The legitimate order, where the hub raster's own fill
    takes a hub start of its own, keeps working.
c.  Hub levels armed for one fill and met by another: refused, and gone.
d.  A refused call (``eps`` NaN, a null ``d8``) takes the armed coarse start or hub levels with
    it.  The fill behind it is of ``z + 1000``: from a surviving coarse start of ``z`` every
    free cell would begin at ``max(z + 1000, coarse) = z + 1000`` and stay there, so the result
    would be the raster itself, which is not its fill.
e.  A coarse raster one column or one row short of the raster: refused before any launch.
f.  ``FILL_WARM | FILL_RESUME`` after the context has done other work.
g.  ``hdem_trim`` before every call of the device table, one context, forward and backward.
h.  The row-block partition with ``hdem_trim`` before every call of its solver.

Also here: the three protocol cases of ``tests/device_cases.py`` under the poison bytes of
tests/test_gpu_scribble.py (its own parametrisation reads its own table only).

Against the library of the parent commit, run once, the tests of (a), (b) and (d) all failed.
(a): "trim behind prepare: raster differs in 42 of 63 cells" at 130 x 190 and "in 259 of 361" at
519 x 508, the first 98.31 for 101.18: the hub raster was built from a buffer ``hdem_trim`` had
freed, and its crossings came out too low.  (b): "DID NOT RAISE" in both variants.  (d): with the
coarse start armed, "filled differs in 6125 of 24700 cells" behind both refusals, which are all
6125 cells the fill raises, each left at ``z + 1000``; with the hub levels armed the good fill
itself was refused with "hub levels were set for another fill than this one".  (e) was never
run there: the parent reads past the end of the coarse raster.
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import device_cases as D
import elevation_regimes as er
import oracle
import test_gpu_mfd as MFD
import test_gpu_scribble as S
from hydrodem_amd import backend as B
from hydrodem_amd.backend import DeviceRaster
from oracle import c_oracle
from test_gpu_fill_paths import FILL_ENV, HUB, HUB_NESTED, KERNELS, ROWS
from test_gpu_mfd import clean_runs                      # noqa: F401  (a fixture, used in g)

pytestmark = pytest.mark.gpu

LARGE = (519, 508)
COARSE_SHAPE, BLOCK = (200, 333), 16
PARTITION_SHAPE = (260, 330)      # where test_gpu_elevation_regimes runs the partition's hub start
STEPS = ("prepare", "raster", "raster_fill", "levels", "fill")
OVERWRITTEN = "the prepared hub start was overwritten"
ANOTHER_FILL = "hub levels were set for another fill than this one"


@pytest.fixture(scope="module", autouse=True)
def _lib(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


class Raster:
    """A host raster with its oracle fill and D8, made once and left alone."""

    def __init__(self, z):
        self.z = z
        self.filled = c_oracle.sinkfill_pflood(z)
        self.codes = c_oracle.d8(self.filled)
        for a in (self.z, self.filled, self.codes):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def rasters():
    small = oracle.synth_dem(130, 190, variant="rough")
    return {"small": Raster(small), "small+1000": Raster(small + np.float32(1000.0)),
            "large": Raster(oracle.synth_dem(*LARGE)),
            "other": Raster(oracle.synth_dem(97, 150, variant="srtm")),
            "coarse": Raster(oracle.synth_dem(*COARSE_SHAPE))}


@contextlib.contextmanager
def fresh_context():
    ctx = B.Context()
    try:
        with contextlib.ExitStack() as stack:
            yield ctx, stack
    finally:
        ctx.close()


def set_env(monkeypatch, env):
    for name in FILL_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def up(ctx, stack, array):
    return stack.enter_context(DeviceRaster.from_host(array, ctx=ctx))


def empty(ctx, stack, shape, dtype=np.float32):
    return stack.enter_context(DeviceRaster.empty(shape, dtype, ctx))


def launches_of(ctx, call):
    """(what ``call`` returns, {kernel: launches}) with the profile reset in front of it."""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        got = call()
        counts = {k: ctx.profile_get(getattr(B, k))["launches"] for k in KERNELS}
    finally:
        ctx.profile(False)
    return got, counts


def assert_oracle(raster, filled, codes=None, what=""):
    S.assert_same_bytes({"filled": filled}, {"filled": raster.filled}, what)
    if codes is not None:
        S.assert_same_bytes({"codes": codes}, {"codes": raster.codes}, what)


def fill_d8(ctx, stack, zd, out=None, flags=B.FILL_INIT):
    """(filled, codes, stats, launches) of one fused call on ``ctx``."""
    (wd, cd, st), counts = launches_of(ctx, lambda: B.sinkfill_d8_dev(zd, out=out, flags=flags))
    stack.enter_context(cd)
    if out is None:
        stack.enter_context(wd)
    return wd.to_host(), cd.to_host(), st, counts


def assert_row(counts, row, what):
    for kernel, n in zip(KERNELS, ROWS[row][3]):
        assert n is None or counts[kernel] == n, (what, kernel, counts)


# ---------------------------------------------------------------------------
# the hub protocol of a partition of one block, step by step
# ---------------------------------------------------------------------------
def hub_levels(ctx, stack, zd, w, after=lambda step: None):
    """prepare -> raster -> the raster's fill; returns (raster, levels) on the device."""
    shape = D.hub_raster_shape(zd.shape)
    ctx.fill_hub_prepare(zd.ptr, zd.shape[0], zd.shape[1], 0, w.ptr)
    after("prepare")
    raster = empty(ctx, stack, shape)
    ctx.fill_hub_raster(raster.ptr)
    after("raster")
    levels, _ = B.sinkfill_dev(raster, out=empty(ctx, stack, shape),
                               flags=B.FILL_INIT | B.FILL_NO_VERIFY)
    after("raster_fill")
    return raster, levels


def hub_protocol(ctx, stack, z, after=lambda step: None):
    """Every step of ``fill-hub-given``; ``after(step)`` is called behind each."""
    zd, w = up(ctx, stack, z), empty(ctx, stack, z.shape)
    raster, levels = hub_levels(ctx, stack, zd, w, after)
    ctx.set_fill_hub_levels(levels.ptr)
    after("levels")
    (_, codes, stats), counts = launches_of(
        ctx, lambda: B.sinkfill_d8_dev(zd, out=w, codes=empty(ctx, stack, z.shape, np.uint8)))
    after("fill")
    got = {"raster": raster.to_host(), "levels": levels.to_host(), "filled": w.to_host(),
           "codes": codes.to_host()}
    return got, stats, counts


# ---------------------------------------------------------------------------
# a. trim inside the hub protocol
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("small", HUB), ("large", {})])
def test_trim_after_every_step_of_the_hub_protocol(monkeypatch, rasters, name, env):
    set_env(monkeypatch, env)
    raster = rasters[name]
    with fresh_context() as (ctx, stack):
        want, stats, _ = hub_protocol(ctx, stack, raster.z)
    assert stats["converged"] and stats["tiles"] == {"small": 12, "large": 81}[name]
    assert_oracle(raster, want["filled"], want["codes"], name)
    for trimmed in [(step,) for step in STEPS] + [STEPS]:
        with fresh_context() as (ctx, stack):
            def trim(step, ctx=ctx):
                if step in trimmed:
                    ctx.trim()
                    assert ctx.trim() == 0, f"a second trim behind {step} released something"
            with ctx.scribble(0xFF):
                got, stats, _ = hub_protocol(ctx, stack, raster.z, trim)
                stack.close()
        S.assert_same_bytes(got, want, f"{name}: trim behind {' and '.join(trimmed)}")
        assert stats["converged"]


# ---------------------------------------------------------------------------
# b. the preparation overwritten
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["a_fill_with_its_own_hub_start", "another_preparation"])
def test_a_preparation_that_was_overwritten_is_refused(monkeypatch, rasters, by):
    set_env(monkeypatch, HUB)
    raster, other = rasters["small"], rasters["other"]
    with fresh_context() as (ctx, stack):
        zd, w = up(ctx, stack, raster.z), empty(ctx, stack, raster.z.shape)
        od = up(ctx, stack, other.z)
        ctx.fill_hub_prepare(zd.ptr, zd.shape[0], zd.shape[1], 0, w.ptr)
        if by == "another_preparation":
            ow = empty(ctx, stack, other.z.shape)
            ctx.fill_hub_prepare(od.ptr, od.shape[0], od.shape[1], 0, ow.ptr)
        else:
            filled, _, st, counts = fill_d8(ctx, stack, od)
            assert counts["K_FILL_HUB"] == 1 and st["converged"]       # (it took its hub start)
            assert_oracle(other, filled, None, "the fill between prepare and raster")
        out = empty(ctx, stack, D.hub_raster_shape(raster.z.shape))
        with pytest.raises(ValueError, match=OVERWRITTEN):
            ctx.fill_hub_raster(out.ptr)
        # the refusal dropped the preparation: nothing to make a raster of, nothing kept by trim
        with pytest.raises(ValueError, match="no prepared hub start"):
            ctx.fill_hub_raster(out.ptr)
        ctx.trim()
        assert ctx.trim() == 0
        got, stats, _ = hub_protocol(ctx, stack, raster.z)
        assert stats["converged"]
        assert_oracle(raster, got["filled"], got["codes"], f"prepared again after {by}")


def test_the_hub_rasters_own_fill_may_take_a_hub_start_of_its_own(monkeypatch, rasters):
    """prepare -> raster -> fill of the raster, which at depth 0 writes the buffer the preparation
    lives in -> levels -> fill: the raster was made, the preparation is no longer needed."""
    raster = rasters["small"]
    with fresh_context() as (ctx, stack):
        set_env(monkeypatch, {})
        want, _, _ = hub_protocol(ctx, stack, raster.z)
    with fresh_context() as (ctx, stack):
        set_env(monkeypatch, HUB_NESTED)
        seen = {}

        def count(step, ctx=ctx):
            if step == "raster":
                ctx.profile(True)
                ctx.profile_reset()
            if step == "raster_fill":
                seen["hub"] = ctx.profile_get(B.K_FILL_HUB)["launches"]
                ctx.profile(False)
        got, stats, counts = hub_protocol(ctx, stack, raster.z, count)
    assert seen["hub"] == 2                     # (the raster's own hub start, and that one's)
    assert counts["K_FILL_HUB"] == 0 and counts["K_FILL_INIT"] == 0, counts
    assert stats["converged"] and stats["rounds"] == 0
    assert_oracle(raster, got["filled"], got["codes"])
    S.assert_same_bytes(got, want, "the raster and its levels, whatever start the raster's fill took")


# ---------------------------------------------------------------------------
# c. levels for another fill
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["plain", "hub"])
def test_levels_armed_for_one_fill_are_refused_and_gone_at_another(monkeypatch, rasters, row):
    set_env(monkeypatch, ROWS[row][0])
    raster, other = rasters["small"], rasters["other"]
    with fresh_context() as (ctx, stack):
        zd, w = up(ctx, stack, raster.z), empty(ctx, stack, raster.z.shape)
        od = up(ctx, stack, other.z)
        _, levels = hub_levels(ctx, stack, zd, w)
        ctx.set_fill_hub_levels(levels.ptr)
        with pytest.raises(ValueError, match=ANOTHER_FILL):
            B.sinkfill_dev(od)
        for zr, name in ((od, "other"), (zd, "small")):
            filled, codes, st, counts = fill_d8(ctx, stack, zr)
            assert st["converged"] and st["rounds"] == 0
            assert_row(counts, row, name)
            assert_oracle(rasters[name], filled, codes, f"{name} behind the refusal")


def test_levels_without_a_preparation_are_refused(rasters):
    with fresh_context() as (ctx, stack):
        levels = empty(ctx, stack, D.hub_raster_shape(rasters["small"].z.shape))
        with pytest.raises(ValueError, match="no prepared hub start"):
            ctx.set_fill_hub_levels(levels.ptr)


# ---------------------------------------------------------------------------
# d. a refused call consumes the armed start
# ---------------------------------------------------------------------------
def refused_fill(ctx, zd, w, how):
    """A fill of (zd, w) the library refuses with BAD_ARG before any launch."""
    st = B.FillStats()
    if how == "nan_eps":
        rc = ctx.lib.hdem_sinkfill_f32_dev(ctx.handle, zd.ptr, zd.shape[0], zd.shape[1],
                                           float("nan"), 0, B.FILL_INIT, w.ptr, ctypes.byref(st))
    else:
        rc = ctx.lib.hdem_sinkfill_d8_f32_dev(ctx.handle, zd.ptr, zd.shape[0], zd.shape[1], 0.0, 0,
                                              B.FILL_INIT, w.ptr, None, ctypes.byref(st))
    assert rc == B.BAD_ARG, (how, rc, ctx.lib.hdem_last_error())


@pytest.mark.parametrize("how", ["nan_eps", "null_d8"])
@pytest.mark.parametrize("armed", ["coarse", "levels"])
def test_a_refused_fill_takes_the_armed_start_with_it(monkeypatch, rasters, armed, how):
    set_env(monkeypatch, {})
    raster, raised = rasters["small"], rasters["small+1000"]
    # on the CPU: the stale coarse start would leave z + 1000 as it is, and that is not its fill
    assert np.nanmax(raster.z) < np.nanmin(raised.z)
    lifted = raised.filled > raised.z
    assert lifted.mean() >= 0.01, "the fill of z + 1000 raises too few cells to tell"
    with fresh_context() as (ctx, stack):
        zd, w = up(ctx, stack, raster.z), empty(ctx, stack, raster.z.shape)
        if armed == "coarse":
            coarse = stack.enter_context(B.blockmax_dev(zd, BLOCK))
            cfill, _ = B.sinkfill_dev(coarse)
            stack.enter_context(cfill)
            ctx.set_fill_coarse_start(cfill.ptr, coarse.shape[0], coarse.shape[1], BLOCK)
        else:
            _, levels = hub_levels(ctx, stack, zd, w)
            ctx.set_fill_hub_levels(levels.ptr)
        refused_fill(ctx, zd, w, how)
        filled, codes, st, counts = fill_d8(ctx, stack, up(ctx, stack, raised.z))
        print(armed, how, counts, int((filled == raised.z)[lifted].sum()), "of", int(lifted.sum()),
              "raised cells left at z + 1000")
        assert st["converged"] and st["rounds"] == 0
        assert_row(counts, "plain", f"behind the refusal of a fill with {armed} armed")
        assert_oracle(raised, filled, codes, f"{armed} armed, then {how}")


# ---------------------------------------------------------------------------
# e. a coarse raster that does not cover the raster
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["column", "row"])
def test_a_coarse_start_that_does_not_cover_the_raster_is_refused(monkeypatch, rasters, short):
    set_env(monkeypatch, {})
    raster = rasters["coarse"]
    H, W = raster.z.shape
    with fresh_context() as (ctx, stack):
        zd, w = up(ctx, stack, raster.z), empty(ctx, stack, raster.z.shape)
        coarse = stack.enter_context(B.blockmax_dev(zd, BLOCK))
        ch, cw = coarse.shape
        assert (ch, cw) == (-(-H // BLOCK), -(-W // BLOCK)) == (13, 21)
        cfill, _ = B.sinkfill_dev(coarse)
        stack.enter_context(cfill)
        # (the same ch x cw floats under a smaller claim: whatever is read lies inside them)
        claim = (ch, cw - 1) if short == "column" else (ch - 1, cw)
        ctx.check(ctx.lib.hdem_memset_dev(ctx.handle, w.ptr, 0xA5, w.nbytes))
        ctx.set_fill_coarse_start(cfill.ptr, claim[0], claim[1], BLOCK)
        text = f"{claim[0]} x {claim[1]} blocks of {BLOCK}, does not cover the {H} x {W} raster"

        def refused():
            with pytest.raises(ValueError, match=text):
                B.sinkfill_dev(zd, out=w)
        _, counts = launches_of(ctx, refused)
        assert not any(counts.values()), counts
        assert (w.to_host().view(np.uint8) == 0xA5).all(), "the refused fill wrote to w"
        ctx.set_fill_coarse_start(cfill.ptr, ch, cw, BLOCK)
        filled, codes, st, counts = fill_d8(ctx, stack, zd, out=w)
        assert st["converged"] and counts["K_FILL_COARSE"] == 0 and counts["K_FILL_HUB"] == 0
        assert_oracle(raster, filled, codes, f"the whole coarse raster after one short of a {short}")


# ---------------------------------------------------------------------------
# f. resume across other work
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("between", ["nothing", "another_fill", "a_larger_fill", "trim"])
def test_resume_after_the_context_did_other_work(monkeypatch, rasters, between):
    set_env(monkeypatch, {"HDEM_FILL_TEST_BUDGET_US": "0"})
    raster = rasters["small"]
    with fresh_context() as (ctx, stack):
        zd, w = up(ctx, stack, raster.z), empty(ctx, stack, raster.z.shape)
        # (the queue that a cut launch leaves is only counted for a call with a time slice)
        ctx.set_fill_slice_us(1000)
        _, st = B.sinkfill_dev(zd, out=w, flags=B.FILL_INIT | B.FILL_NO_VERIFY)
        ctx.set_fill_slice_us(0)
        assert st["pending"] > 0, st
        set_env(monkeypatch, {})
        if between == "trim":
            ctx.trim()
        elif between != "nothing":
            other = rasters["other" if between == "another_fill" else "large"]
            filled, codes, _, _ = fill_d8(ctx, stack, up(ctx, stack, other.z))
            assert_oracle(other, filled, codes, between)
        _, st = B.sinkfill_dev(zd, out=w, flags=B.FILL_WARM | B.FILL_RESUME)
        print(between, st)
        assert st["converged"] and st["pending"] == 0 and st["async_timed_out"] == 0
        if between != "nothing":
            assert st["tile_visits"] >= st["tiles"] == 12
        assert_oracle(raster, w.to_host(), None, f"resumed after {between}")


# ---------------------------------------------------------------------------
# g. trim before every call of the table
# ---------------------------------------------------------------------------
def test_trim_before_every_call_of_the_device_table(clean_runs):   # noqa: F811
    steps = [(entry, shape, *S.baseline(entry, shape)) for entry, shape in D.PARAMS]
    steps += [(entry, shape, *clean_runs(entry, shape, False)) for entry, shape in MFD.POISON_PARAMS]
    ctx = B.Context()
    began = time.perf_counter()
    try:
        for entry, shape, inputs, want, want_stats in steps + steps[::-1]:
            ctx.trim()
            call = S.Call(ctx, False)
            with call.stack:
                arrays, stats = entry.run(call, inputs)
            what = f"{entry.name} {shape} behind a trim"
            S.assert_same_bytes({k: np.ascontiguousarray(v) for k, v in arrays.items()}, want, what)
            assert S.counters(stats, entry.schedule) == want_stats, what
        ctx.trim()
        assert ctx.trim() == 0
    finally:
        ctx.close()
    # (what the test takes beyond this are the runs on fresh contexts, which the files that share
    # them would make otherwise)
    print(f"\n{2 * len(steps)} calls behind a trim each: {time.perf_counter() - began:.2f} s")


# ---------------------------------------------------------------------------
# h. the partition under trim
# ---------------------------------------------------------------------------
def test_the_partition_with_a_trim_before_every_call_of_its_solver():
    import torch
    from hydrodem_amd import partition as P

    class TrimmingSolver(P.HipLocalSolver):
        trims = 0

        @contextlib.contextmanager
        def _call(self, label="call"):
            with super()._call(label):
                self.ctx.trim()
                self.trims += 1
                yield

    world, (H, W) = 2, PARTITION_SHAPE
    z, want, want_d8 = er.regime_fill("below_sea", (H, W))

    def body(rank, comm):
        g0, g1, _, _ = P.local_range(rank, world, H)
        zt = torch.from_numpy(z[g0:g1].copy()).cuda()
        d8 = torch.empty(zt.shape, dtype=torch.uint8, device=zt.device)
        solver = TrimmingSolver(0, turn=comm.gpu_turn)
        try:
            w, info = P.sinkfill_distributed(zt, rank, world, solver, comm=comm, d8_out=d8)
            torch.cuda.synchronize()
            own = P.owned_slice(rank, world)
            return w[own].cpu().numpy(), d8[own].cpu().numpy(), info, solver.trims
        finally:
            solver.ctx.close()

    got = P.ThreadWorld(world).run(body)
    assert all(g[2]["start_values"] == "hub" and g[3] >= 4 for g in got), [g[2:] for g in got]
    S.assert_same_bytes({"filled": np.concatenate([g[0] for g in got]),
                         "codes": np.concatenate([g[1] for g in got])},
                        {"filled": want, "codes": want_d8}, "the partition under trim")


# ---------------------------------------------------------------------------
# the protocol cases of the device table under poison
# ---------------------------------------------------------------------------
PROTOCOL_PARAMS = [(case, shape, own) for case in D.FILL_PROTOCOL_CASES for shape in case.shapes
                   for own in ((False, True) if case.own else (False,))]
PROTOCOL_IDS = [f"{case.name}-{shape[0]}x{shape[1]}-{'callers_out' if own else 'library_out'}"
                for case, shape, own in PROTOCOL_PARAMS]


@pytest.mark.parametrize("entry,shape,own", PROTOCOL_PARAMS, ids=PROTOCOL_IDS)
def test_the_protocol_cases_on_poisoned_memory(entry, shape, own):
    inputs, want, want_stats = S.baseline(entry, shape)
    entry.check(inputs, want)
    for byte in S.POISON:
        got, stats = S.execute(entry, inputs, byte, own)
        what = f"{entry.name} {shape} under 0x{byte:02X}, own={own}"
        S.assert_same_bytes(got, want, what)
        assert stats == want_stats, what
