"""
Every device operator on a caller's stream and beside a second context.

The other GPU tests run each operator on the context's own stream, from one thread, on inputs a
synchronous copy has put in place: there a launch, a memset, a copy or an FFT on the wrong
stream passes, because whatever it reads is complete.  Here the table of
``tests/device_cases.py`` (every ``_dev`` entry point, one shape each) is run

a.  on a caller's stream (a ``torch.cuda.Stream`` given to ``hdem_set_stream``) behind a producer
    that has not finished: one slab holds the operands and the caller's outputs, it is filled
    with 0x00, a delay is queued on the stream, the operands follow it with
    ``hdem_memcpy_h2d_async`` from page-locked memory, and the operator is called without any
    wait on the host.  Work that is queued on any stream but the caller's reads zeros -- valid
    input to every operator (code 0, label 0, word 0, elevation 0.0, weight 0), so it computes
    a wrong answer and no address from garbage.  Results and schedule-free stats are those of
    R0, the run on a fresh context's own stream (``test_gpu_scribble.baseline``), which is held
    to the CPU reference here too;
b.  as one chain a torch caller would write: the DEM made by torch arithmetic on the stream
    behind the delay, ``DemToHAND(flats="resolve")`` and ``DemToDInfWetness`` on wrapped
    tensors, a torch reduction of the results on the same stream, one synchronisation;
c.  on two contexts from two threads at once, three passes over the table from two starting
    points, a barrier before each step, with a refused call on one thread while the other's
    succeeds: each thread reads its own ``hdem_last_error``;
d.  across ``hdem_set_stream``: an operator that returns without a host wait and uses the
    context's own scratch on stream A, a change to stream B, the next such operator there.  B
    must wait for A: an event recorded on B has not completed a quarter of the delay later.

The delay is ``torch.cuda._sleep`` (a chain of element-wise operations where a torch build has
none), its cycle count calibrated and its duration measured once per module with torch events,
and every operator call is timed the same way on the idle stream: the delay must be ten times
the call.  Measured on the MI355X: 249.9 ms for the delay (598 986 229 cycles), 10.96 ms for
the longest call (fft2-complex64-forward at 141 x 155: the first complex64 transform of a
context makes its rocFFT plan); the whole file takes 53 s, the slowest test 2.7 s
(``pytest --durations=0``: the first Fourier R0 of the process; a test of (a) with both kinds of
``out=`` takes 0.55 s, two delays and three runs, (c) 0.85 s).

What was found: ``hdem_set_stream`` only stored the new stream, so in (d) stream B ran ahead of
the work still queued on A, on the same arena and the same Fourier scratch.  Against the
library before the fix (``hdem_core.hip`` of the parent commit, everything else as it is), run
once: both tests of (d) fail with "stream B did not wait for the work queued on stream A" (the
calls had taken 22 and 10 ms of host time of a 250 ms delay, so the ordering was tested), and
pass with the fix, where the new stream waits on an event recorded on the old one (the calls
queued in 0.2 and 0.3 ms).

That (a) can fail was shown once with a value-only mutant, in the manner of
tests/test_gpu_size_regimes_newer.py: ``boxmean3_kernel`` launched on ``ctx->own_stream``
instead of ``ctx->stream`` reads the zero-filled slab and computes no address from data.
Under it (a) failed for the four box-mean cases and for none of the other 80: behind the delay
the mean is 0.0 in all 20 567 cells (for 100.0 in the first), and on the idle stream of the
caller's, where the kernel races the copy, boxmean3-float32-plain differs in 10 048 cells.
The mutant is not part of the repository.
"""
import contextlib
import ctypes
import threading
import time

import numpy as np
import pytest
import torch

import device_cases as D
import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend as B
from hydrodem_amd.backend import DeviceRaster
from test_gpu_scribble import Call, assert_same_bytes, baseline, counters

pytestmark = pytest.mark.gpu

DELAY_TARGET_MS = 250.0
ALIGN = 256


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert B.device_count() >= 1, "these tests need a GPU"
    yield


# ---------------------------------------------------------------------------
# the delay
# ---------------------------------------------------------------------------
def elapsed_ms(stream, work):
    """``work()`` between two torch events on ``stream``, which is idle before and after."""
    stream.synchronize()
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first.record(stream)
    work()
    last.record(stream)
    stream.synchronize()
    return first.elapsed_time(last)


class Delay:
    """``queue(stream)`` keeps ``stream`` busy for ``ms`` milliseconds, measured here."""

    def __init__(self):
        stream = torch.cuda.Stream()
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.tensor = torch.ones(1 << 26, device="cuda")
        self.count = 1
        self.queue(stream)                                        # (first launch, not timed)
        # (the count for the target from a short probe, corrected twice: the clock the cycles are
        # counted in rises with the load.  What is relied on is ``ms``, the shortest of three.)
        self.count = 20_000_000 if self.sleep is not None else 8
        for _ in range(3):
            ms = elapsed_ms(stream, lambda: self.queue(stream))
            self.count = max(1, int(self.count * DELAY_TARGET_MS / ms))
        self.ms = min(elapsed_ms(stream, lambda: self.queue(stream)) for _ in range(3))
        print(f"\nthe delay: {self.count} {'cycles' if self.sleep else 'steps'}, {self.ms:.1f} ms")

    def queue(self, stream):
        with torch.cuda.stream(stream):
            if self.sleep is not None:
                self.sleep(self.count)
            else:
                for _ in range(self.count):
                    self.tensor.mul_(1.0)


@pytest.fixture(scope="module")
def delay():
    return Delay()


LONGEST = {"ms": 0.0, "case": None}


def note_call(ms, what, delay):
    if ms > LONGEST["ms"]:
        LONGEST.update(ms=ms, case=what)
    assert delay.ms >= 10.0 * ms, f"{what} takes {ms:.2f} ms, the delay {delay.ms:.1f} ms"


# ---------------------------------------------------------------------------
# one call on a caller's stream, out of one slab
# ---------------------------------------------------------------------------
def arrays_in(value):
    if isinstance(value, np.ndarray):
        yield value
    elif isinstance(value, dict):
        for item in value.values():
            yield from arrays_in(item)


def slab_bytes(inputs, want):
    """Room for every operand and every caller-owned output and scratch of a case, each rounded
    up to ``ALIGN``: the inputs once, the results twice (a scratch is a result's size)."""
    rounded = lambda n: -(-n // ALIGN) * ALIGN + ALIGN
    return sum(rounded(a.nbytes) for a in arrays_in(inputs)) + \
        2 * sum(rounded(a.nbytes) for a in want.values()) + (1 << 16)


class SlabCall(Call):
    """A ``Call`` whose operands and caller's outputs are carved out of one device slab, the
    operands filled by asynchronous copies from one page-locked block."""

    def __init__(self, ctx, own, nbytes):
        super().__init__(ctx, own)
        self.nbytes, self.used = nbytes, 0
        self.slab = self.stack.enter_context(DeviceRaster.empty((nbytes // ALIGN, ALIGN), np.uint8, ctx))
        pinned = ctypes.c_void_p()
        ctx.check(ctx.lib.hdem_host_alloc(ctx.handle, nbytes, ctypes.byref(pinned)))
        self.pinned = pinned.value
        self.stack.callback(ctx.lib.hdem_host_free, ctx.handle, pinned)
        ctx.check(ctx.lib.hdem_memset_dev(ctx.handle, self.slab.ptr, 0x00, nbytes))
        ctx.synchronize()

    def carve(self, shape, dtype):
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        offset = self.used
        self.used += -(-size // ALIGN) * ALIGN
        assert self.used <= self.nbytes, "the slab is too small for this case"
        return offset, DeviceRaster.wrap(self.slab.ptr + offset, shape, dtype, ctx=self.ctx,
                                         keepalive=self.slab)

    def up(self, array):
        a = np.ascontiguousarray(array)
        assert a.dtype in B._DTYPES and a.ndim == 2
        offset, raster = self.carve(a.shape, a.dtype)
        ctypes.memmove(self.pinned + offset, a.ctypes.data, a.nbytes)
        self.ctx.check(self.ctx.lib.hdem_memcpy_h2d_async(self.ctx.handle, raster.ptr,
                                                          self.pinned + offset, a.nbytes))
        return raster

    def empty(self, shape, dtype):
        return self.carve(shape, dtype)[1]


def on_a_callers_stream(entry, inputs, want, own, delay=None, timed=None):
    """``entry.run`` on a fresh context that runs on a torch stream, from a zeroed slab, behind
    ``delay`` when there is one; ``timed``: a list that takes the call's milliseconds."""
    ctx = B.Context()
    side = torch.cuda.Stream()
    try:
        ctx.set_stream(side.cuda_stream)
        call = SlabCall(ctx, own, slab_bytes(inputs, want))
        with call.stack:
            if delay is not None:
                delay.queue(side)
            if timed is None:
                arrays, stats = entry.run(call, inputs)
            else:
                made = []
                timed.append(elapsed_ms(side, lambda: made.append(entry.run(call, inputs))))
                arrays, stats = made[0]
            ctx.synchronize()
        return ({k: np.ascontiguousarray(v) for k, v in arrays.items()},
                counters(stats, entry.schedule))
    except B.BackendError as exc:
        # a HIP call failed: whatever runs on this device afterwards proves nothing
        pytest.exit(f"a HIP call failed in {entry.name} on a caller's stream: {exc}", returncode=3)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# R0 is the CPU reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry,shape", D.PARAMS, ids=D.IDS)
def test_the_run_on_the_own_stream_is_the_cpu_reference(entry, shape):
    inputs, got, _ = baseline(entry, shape)
    entry.check(inputs, got)


# ---------------------------------------------------------------------------
# a. a caller's stream, behind a producer that has not finished
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry,shape", D.PARAMS, ids=D.IDS)
def test_a_callers_stream_behind_an_unfinished_producer_changes_no_byte(entry, shape, delay):
    inputs, want, want_stats = baseline(entry, shape)
    timed = []
    got, stats = on_a_callers_stream(entry, inputs, want, False, None, timed)
    assert_same_bytes(got, want, f"{entry.name} {shape} on an idle stream of the caller's")
    note_call(timed[0], f"{entry.name} {shape}", delay)
    for own in (False, True) if entry.own else (False,):
        whose = "the caller's" if own else "the library's"
        what = f"{entry.name} {shape} behind the delay, out= {whose}"
        got, stats = on_a_callers_stream(entry, inputs, want, own, delay)
        assert_same_bytes(got, want, what)
        assert stats == want_stats, what


# ---------------------------------------------------------------------------
# b. torch interop
# ---------------------------------------------------------------------------
CHAIN_SHAPE = (300, 500)


def chains():
    return {"hand": hd.DemToHAND(threshold=50, epsilon=0.0, cellsize=30.0, flats="resolve"),
            "wetness": hd.DemToDInfWetness(cellsize=30.0)}


def test_a_torch_chain_on_one_stream_with_one_synchronisation(delay):
    z = hdem_synth.synth_dem(*CHAIN_SHAPE)
    want = {}
    ctx = B.Context()
    try:
        with DeviceRaster.from_host(z, ctx=ctx) as dz:
            for name, chain in chains().items():
                with chain.apply_device(dz) as out:
                    want[name] = out.to_host()
    finally:
        ctx.close()
    assert np.isfinite(want["hand"]).any() and np.isfinite(want["wetness"]).any()

    ctx = B.Context()
    side = torch.cuda.Stream()
    try:
        ctx.set_stream(side.cuda_stream)
        source = torch.from_numpy(z).cuda()
        dem = torch.zeros_like(source)
        torch.cuda.synchronize()
        delay.queue(side)
        results, totals, kept = {}, {}, []
        with torch.cuda.stream(side):
            torch.mul(source, 2.0, out=dem)                      # 2 z - z: z, exactly
            dem.sub_(source)
            wrapped = DeviceRaster.wrap(dem.data_ptr(), dem.shape, np.float32, ctx=ctx, keepalive=dem)
            for name, chain in chains().items():
                out = chain.apply_device(wrapped)
                kept.append(out)
                results[name] = torch.empty(CHAIN_SHAPE, dtype=torch.float32, device="cuda")
                ctx.check(ctx.lib.hdem_memcpy_d2d(ctx.handle, results[name].data_ptr(), out.ptr,
                                                  out.nbytes))
                totals[name] = torch.nansum(results[name].double())
        side.synchronize()                                       # the one synchronisation
        for out in kept:
            out.free()
        for name in want:
            got = results[name].cpu().numpy()
            assert_same_bytes({name: got}, {name: want[name]}, f"the {name} chain behind torch")
            assert totals[name].item() == torch.nansum(torch.from_numpy(want[name]).double()).item()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# c. two contexts, two threads, one GPU
# ---------------------------------------------------------------------------
PASSES = 3


def refused(ctx, raster, window, out):
    """A majority call the library refuses before any kernel; its status and its text."""
    rc = ctx.lib.hdem_majority_f32_dev(ctx.handle, raster.ptr, *raster.shape, window, out)
    return rc, ctx.lib.hdem_last_error()


def test_two_contexts_on_two_threads_walk_the_table_at_once():
    steps = [(entry, shape, *baseline(entry, shape)) for entry, shape in D.PARAMS]
    starts = (0, len(steps) // 2)
    errors, texts = [], [[], []]
    start = threading.Barrier(2)

    def run(k):
        try:
            ctx = B.Context(0)
            with DeviceRaster.from_host(np.zeros((16, 16), np.float32), ctx=ctx) as small, \
                    DeviceRaster.empty((16, 16), np.float32, ctx) as other:
                for n in range(PASSES):
                    if k == 0:
                        # this thread's own text, to be found again after the other's refusal
                        rc, mine = refused(ctx, small, 4 + 2 * n, other.ptr)
                        assert rc == B.WINDOW_EVEN and str(4 + 2 * n).encode() in mine, mine
                    for i in range(len(steps)):
                        entry, shape, inputs, want, want_stats = steps[(starts[k] + i) % len(steps)]
                        start.wait()
                        if k == 1 and i == 7 * (n + 1):
                            rc, mine = refused(ctx, small, 5, None)      # while thread 0 succeeds
                            assert rc == B.BAD_ARG and mine == b"null raster pointer", mine
                        call = Call(ctx, False)
                        with call.stack:
                            arrays, stats = entry.run(call, inputs)
                        what = f"thread {k}, pass {n}: {entry.name} {shape}"
                        assert_same_bytes({name: np.ascontiguousarray(a) for name, a in arrays.items()},
                                          want, what)
                        assert counters(stats, entry.schedule) == want_stats, what
                        if i == 7 * (n + 1):
                            start.wait()                                 # both calls are over
                            assert ctx.lib.hdem_last_error() == mine, what
                            texts[k].append(mine)
            ctx.close()
        except BaseException as exc:                        # pylint: disable=broad-except
            errors.append(exc)
            start.abort()

    threads = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(texts[0]) == len(texts[1]) == PASSES
    assert not set(texts[0]) & set(texts[1])


# ---------------------------------------------------------------------------
# d. the stream change
# ---------------------------------------------------------------------------
def entry_named(name):
    return next(e.case for e in D.ENTRIES if e.case.name == name)


def changed_streams(first, second, delay):
    """``first`` behind the delay on stream A, then ``second`` on stream B of the same context.
    Each is ``prepare(ctx, stack) -> launch`` (the uploads, waited for) and ``launch() ->
    collect`` (the operator call, no wait); both are launched once before on the context's own
    stream, so that the scratch and the block cache have their sizes and no call has to
    allocate.  Returns what the two collect, whether B was still waiting a quarter of the delay
    after the calls, and the host time the calls took."""
    ctx = B.Context()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        with contextlib.ExitStack() as warm:
            for launch in [first(ctx, warm), second(ctx, warm)]:
                launch()
            ctx.synchronize()
        with contextlib.ExitStack() as stack:
            launch_first, launch_second = first(ctx, stack), second(ctx, stack)
            ctx.synchronize()
            ctx.set_stream(a.cuda_stream)
            began = time.perf_counter()
            delay.queue(a)
            collect_first = launch_first()
            ctx.set_stream(b.cuda_stream)
            collect_second = launch_second()
            done = torch.cuda.Event()
            done.record(b)
            queued_ms = (time.perf_counter() - began) * 1e3
            time.sleep(delay.ms / 4e3)
            waiting = not done.query()
            a.synchronize()
            b.synchronize()
            return collect_first(), collect_second(), waiting, queued_ms
    finally:
        ctx.close()


def assert_b_waited(waiting, queued_ms, delay, what):
    print(f"\n{what}: queued in {queued_ms:.2f} ms of {delay.ms:.1f}")
    assert queued_ms < delay.ms / 4, "the calls waited on the host: the ordering was not tested"
    assert waiting, "stream B did not wait for the work queued on stream A"


def test_a_changed_stream_waits_for_the_arena_of_the_stream_before(delay):
    lagoons, blanks = entry_named("lagoons_detection"), entry_named("blanks_fourier")
    hs, want_lagoons, _ = baseline(lagoons, D.WINDOW_SHAPE)
    mag, want_blanks, _ = baseline(blanks, D.FFT_SHAPE)

    def first(ctx, stack):
        raster = stack.enter_context(DeviceRaster.from_host(hs["hs"], ctx=ctx))

        def launch():
            outs = [stack.enter_context(r) for r in B.lagoons_detection_dev(raster)]
            return lambda: dict(zip(("mask", "fixed", "values"), (r.to_host() for r in outs)))
        return launch

    def second(ctx, stack):
        q = stack.enter_context(DeviceRaster.from_host(mag["mag"], ctx=ctx))

        def launch():
            found = stack.enter_context(B.blanks_fourier_dev(q))
            return lambda: {"found": found.to_host(), "q": q.to_host()}
        return launch

    got_lagoons, got_blanks, waiting, queued_ms = changed_streams(first, second, delay)
    assert_b_waited(waiting, queued_ms, delay, "lagoons on A, blanks on B")
    assert_same_bytes(got_lagoons, want_lagoons, "the lagoons on stream A")
    assert_same_bytes(got_blanks, want_blanks, "the blanks on stream B")


def test_a_changed_stream_waits_for_the_fourier_scratch_of_the_stream_before(delay):
    destripe = entry_named("fourier_destripe")
    inputs, want, _ = baseline(destripe, D.DESTRIPE_SHAPES[0])

    def once(ctx, stack):
        dem = stack.enter_context(DeviceRaster.from_host(inputs["dem"], ctx=ctx))
        mask = stack.enter_context(DeviceRaster.empty(dem.shape, np.uint8, ctx))

        def launch():
            out = stack.enter_context(B.fourier_destripe_dev(dem, mask=mask))
            return lambda: {"dem": out.to_host(), "mask": mask.to_host()}
        return launch

    on_a, on_b, waiting, queued_ms = changed_streams(once, once, delay)
    assert_b_waited(waiting, queued_ms, delay, "destripe on A, then on B")
    assert_same_bytes(on_a, want, "the destripe on stream A")
    assert_same_bytes(on_b, want, "the destripe on stream B")


def test_the_delay_is_ten_times_the_longest_call(delay):
    """(runs last: the figures of the file's docstring)"""
    print(f"\nthe delay {delay.ms:.1f} ms, the longest call {LONGEST['ms']:.2f} ms "
          f"({LONGEST['case']})")
    assert LONGEST["case"] is None or delay.ms >= 10.0 * LONGEST["ms"]
