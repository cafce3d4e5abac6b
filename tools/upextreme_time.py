"""HIP-event times of the upstream D8 extreme (``hdem_upextreme_u8_dev``) and of depression
breaching (``hdem_breach_f32_dev``), phase by phase, next to ``hdem_flowacc_u8_dev`` and
``hdem_flowsum_u8_dev`` on the same codes in the same process.

Input: ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2.  The extreme runs on the D8
codes of its epsilon = 1e-3 sink fill with float32 values in [0, 100), in both modes, writing
``extreme`` alone and ``extreme`` with ``where``; ``FlowAccumulation`` and
``WeightedFlowAccumulation`` (float32 weights, ``value``) run on the same codes, and the ratios
of the medians are reported.  The breach runs on the ``ResolveFlats`` codes of the epsilon = 0
fill of the same raster: its phases (A with the pit stencil, B, C) by HIP events, and the whole
``BreachDepressions`` chain by the host clock around ``apply_device`` (every stage synchronises),
with the share of the chain that the breach call takes.  Warm-up calls, then --reps calls, every
one kept.

    python tools/upextreme_time.py [--sizes 4096,16384] [--reps 7] [--warmup 2]

``--cpu SIZE`` times the CPU route instead, on the same raster (no GPU needed): the forest from
the oracles (``--cpu-fill jacobi``: the NumPy fill of the tests; ``pflood``, the default: the C
priority flood that is bit-equal to it), then the NumPy carving of tests/test_upextreme.py.
"""
import argparse
import json
import time

import numpy as np

import d8_inputs  # noqa: F401  (puts the repository root and tests/ on sys.path)
import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, flowsum, upextreme


def timed(call, reps, warmup):
    """Every repeat of ``call() -> stats``: rows of (A, B, C, A + B + C) in ms."""
    for _ in range(warmup):
        call()
    rows = []
    for _ in range(reps):
        st = call()
        phases = [st["ms_tile"], st["ms_forest"], st["ms_final"]]
        rows.append([round(t, 4) for t in phases + [sum(phases)]])
    return rows


def summary(rows):
    cols = list(zip(*rows))
    return {"median": [round(float(np.median(c)), 4) for c in cols],
            "min": [min(c) for c in cols], "max": [max(c) for c in cols], "all": rows}


def run_extreme(dz, reps, warmup):
    ctx = dz.ctx
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    filled.free()
    shape, size = codes.shape, codes.shape[0]
    host = np.random.default_rng(size).random(shape, dtype=np.float32) * np.float32(100)
    records = []
    try:
        with backend.DeviceRaster.from_host(host, dtype=np.float32, ctx=ctx) as v, \
                backend.DeviceRaster.empty(shape, np.float32, ctx) as out, \
                backend.DeviceRaster.empty(shape, np.uint32, ctx) as out32:
            acc = summary(timed(lambda: backend.flowacc_dev(codes, out32)[1], reps, warmup))
            wsum = summary(timed(
                lambda: flowsum.flowsum_dev(codes, v, 16, "value", out={"value": out})[1],
                reps, warmup))
            for mode in ("min", "max"):
                for want in (("extreme",), ("extreme", "where")):
                    outs = {"extreme": out, "where": out32}
                    got = summary(timed(
                        lambda: upextreme.upextreme_dev(codes, v, mode, want,
                                                        out={k: outs[k] for k in want})[1],
                        reps, warmup))
                    total = got["median"][3]
                    records.append({"size": size, "mode": mode, "outputs": list(want),
                                    "ms_A_B_C_total": got,
                                    "ratio_to_flowacc": round(total / acc["median"][3], 3),
                                    "ratio_to_flowsum": round(total / wsum["median"][3], 3),
                                    "gcells_per_s": round(size * size / total / 1e6, 2)})
        for name, base in (("FlowAccumulation", acc), ("WeightedFlowAccumulation", wsum)):
            records.append({"size": size, "operator": name, "ms_A_B_C_total": base,
                            "gcells_per_s": round(size * size / base["median"][3] / 1e6, 2)})
    finally:
        codes.free()
    return records


def run_breach(dz, reps, warmup):
    """The phases with profiling on; the chain by the host clock with profiling off, so that
    no stage pays for events it does not report here."""
    ctx, size = dz.ctx, dz.shape[0]
    chain = hd.BreachDepressions()

    def once():
        chain.apply_device(dz).free()
        return chain.stats["BreachDepressions"]
    got = summary(timed(once, reps, warmup))
    st = chain.stats["BreachDepressions"]
    wall = []
    ctx.profile(False)
    try:
        for k in range(warmup + reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            once()
            if k >= warmup:
                wall.append(round((time.perf_counter() - t0) * 1e3, 3))
    finally:
        ctx.profile(True)
    return [{"size": size, "operator": "BreachDepressions", "ms_A_B_C_total": got,
             "chain_ms": {"median": round(float(np.median(wall)), 3), "min": min(wall),
                          "max": max(wall), "all": wall},
             "breach_share_of_chain": round(got["median"][3] / float(np.median(wall)), 4),
             "pits": st["pits"], "lowered": st["lowered"], "cells": size * size,
             "gcells_per_s": round(size * size / got["median"][3] / 1e6, 2)}]


def run_cpu(size, fill):
    """The CPU route: the forest from the oracles, then the NumPy carving.  ``fill``: the NumPy
    Jacobi fill of the tests, or the C priority flood that is bit-equal to it (the Jacobi sweeps
    grow with the raster's side: 10 s at 1024^2, not practical at 4096^2)."""
    from oracle import c_oracle
    from oracle.hdem_oracle_np import d8_flow_direction, sinkfill_jacobi
    from test_flats import resolve_flats_bfs
    from test_upextreme import carve_ref
    z = hdem_synth.synth_dem(size, size)
    t0 = time.perf_counter()
    filled = sinkfill_jacobi(z)[0] if fill == "jacobi" else c_oracle.sinkfill_pflood(z)
    t1 = time.perf_counter()
    codes, _ = resolve_flats_bfs(filled, d8_flow_direction(filled))
    t2 = time.perf_counter()
    _, _, pits, lowered = carve_ref(z, codes)
    t3 = time.perf_counter()
    return {"size": size, "route": "cpu", "fill": fill, "fill_s": round(t1 - t0, 2),
            "d8_and_flats_s": round(t2 - t1, 2), "carve_s": round(t3 - t2, 2),
            "total_s": round(t3 - t0, 2), "pits": pits, "lowered": lowered}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", type=int, default=0, metavar="SIZE")
    ap.add_argument("--cpu-fill", choices=("pflood", "jacobi"), default="pflood")
    a = ap.parse_args()
    if a.cpu:
        print(json.dumps(run_cpu(a.cpu, a.cpu_fill)), flush=True)
        return
    if backend.device_count() < 1:
        raise SystemExit("upextreme_time.py needs a GPU")
    ctx = backend.context()
    ctx.profile(True)
    try:
        for size in (int(s) for s in a.sizes.split(",")):
            with backend.DeviceRaster.from_host(hdem_synth.synth_dem(size, size),
                                                dtype=np.float32, ctx=ctx) as dz:
                for run in (run_extreme, run_breach):
                    for record in run(dz, a.reps, a.warmup):
                        print(json.dumps(record), flush=True)
    finally:
        ctx.profile(False)


if __name__ == "__main__":
    main()
