"""HIP-event times of the downstream D8 path sums and extremes (``hdem_flowpath_u8_dev``), phase
by phase, next to ``FlowDistance`` (``hdem_flowtrace_u8_dev``) on the same codes in the same
process.

Input: the rasters of ``tools/flowtrace_time.py`` -- the D8 codes of the epsilon = 1e-3 sink
fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2, made on the device, with the
device ``FlowAccumulation`` of those codes as the stream raster (threshold 1000 at 4096^2,
10 000 elsewhere).  Four calls: the sum to the outlet with float32 weights in [0, 100) at 16
fractional bits; the same sum to the streams; the sum per unit length with a geographic table
(1 arc second cells from 45 degrees north) and no weights, to the outlet; the minimum of the
float32 raster to the outlet.  Each writes one output (``value`` or ``extreme``) into a raster
of the caller's.  Warm-up calls, then the median of --reps calls of phase A (costs made,
in-tile pointer doubling), B (the forest of perimeter slots) and C (outputs written) and their
sum; every repeat is kept.  ``FlowDistance`` to the outlet and to the streams is timed the same
way, and each call is divided by the one with the same stops.  The call has no kernel id: its
total is the sum of its three phases (the events are back to back on the context's stream).

    python tools/flowpath_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2]
"""
import argparse
import json

import numpy as np

from d8_inputs import PER, filled_codes, tiles_of
from hydrodem_amd import backend
from hydrodem_amd import flowpath as fp

THRESHOLDS = {4096: 1000}            # 10 000 elsewhere


def timed(call, reps, warmup):
    """Every repeat of ``call() -> stats``: rows of (A, B, C, A + B + C) in ms, and the stats
    of the last one."""
    for _ in range(warmup):
        call()
    rows = []
    for _ in range(reps):
        st = call()
        phases = [st["ms_tile"], st["ms_forest"], st["ms_final"]]
        rows.append([round(t, 4) for t in phases + [sum(phases)]])
    return rows, st


def summary(rows):
    cols = list(zip(*rows))
    return {"median": [round(float(np.median(c)), 4) for c in cols],
            "min": [min(c) for c in cols], "max": [max(c) for c in cols], "all": rows}


def modelled_bytes_per_cell(size, streams, value_bytes, launches):
    """(A, B, C) bytes per cell.  A reads the codes, the stream raster and the values and
    writes 8 B per cell and a 16-byte node per slot; each of B's launches with work reads and
    writes every node; C reads 8 B per cell and the nodes and writes its 4-byte output."""
    slots = tiles_of(size, size) * PER * 16 / (size * size)
    return (1 + (4 if streams else 0) + value_bytes + 8 + slots, 2 * slots * launches,
            8 + slots + 4)


def trace(codes, streams, threshold):
    outs, st = backend.flowtrace_dev(codes, streams, threshold, None, 30.0, ("distance",))
    for raster in outs.values():
        raster.free()
    return st


def run(size, reps, warmup):
    ctx = backend.context()
    threshold = THRESHOLDS.get(size, 10000)
    codes = filled_codes(size)
    acc, _ = backend.flowacc_dev(codes)
    shape = codes.shape
    host = np.random.default_rng(size).random(shape, dtype=np.float32) * np.float32(100)
    table = fp.geographic_step_lengths(size, 45.0, 1.0 / 3600, 1.0 / 3600)
    cells = size * size
    records = []
    try:
        with backend.DeviceRaster.from_host(host, dtype=np.float32, ctx=ctx) as v, \
                backend.DeviceRaster.empty(shape, np.float32, ctx) as out:
            base = {}
            for name, streams, cut in (("outlet", None, None), ("streams", acc, threshold)):
                rows, st = timed(lambda: trace(codes, streams, cut), reps, warmup)
                base[name] = summary(rows)
                records.append({"size": size, "operator": "FlowDistance", "stops": name,
                                "ms_A_B_C_total": base[name], "unreached": int(st["unreached"]),
                                "gcells_per_s": round(cells / base[name]["median"][3] / 1e6, 2)})
            calls = (
                ("sum_outlet_f32", "outlet", dict(values=v, mode="sum", frac_bits=16,
                                                  want="value", out={"value": out})),
                ("sum_streams_f32", "streams", dict(values=v, mode="sum", streams=acc,
                                                    threshold=threshold, frac_bits=16,
                                                    want="value", out={"value": out})),
                ("length_geographic", "outlet", dict(values=None, mode="sum", per="length",
                                                     step_len=table, frac_bits=16, want="value",
                                                     out={"value": out})),
                ("min_outlet_f32", "outlet", dict(values=v, mode="min", want="extreme",
                                                  out={"extreme": out})))
            for name, stops, kw in calls:
                rows, st = timed(lambda: fp.flowpath_dev(codes, **kw)[1], reps, warmup)
                got = summary(rows)
                model = modelled_bytes_per_cell(size, stops == "streams",
                                                0 if kw["values"] is None else 4,
                                                int(st["forest_rounds"]))
                records.append({
                    "size": size, "call": name, "stops": stops, "ms_A_B_C_total": got,
                    "ratio_to_flowdistance": round(got["median"][3] / base[stops]["median"][3], 3),
                    "gcells_per_s": round(cells / got["median"][3] / 1e6, 2),
                    "forest_rounds": int(st["forest_rounds"]), "exits": int(st["exits"]),
                    "unreached": int(st["unreached"]),
                    "bytes_per_cell_model_ABC": [round(b, 2) for b in model],
                    "gbs_model_ABC": [round(b * cells / ms / 1e6, 1)
                                      for b, ms in zip(model, got["median"])]})
    finally:
        acc.free()
        codes.free()
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("flowpath_time.py needs a GPU")
    ctx = backend.context()
    ctx.profile(True)
    try:
        for size in (int(s) for s in a.sizes.split(",") if s):
            for record in run(size, a.reps, a.warmup):
                print(json.dumps(record), flush=True)
    finally:
        ctx.profile(False)


if __name__ == "__main__":
    main()
