"""HIP-event times of weighted D8 flow accumulation (``hdem_flowsum_u8_dev``), phase by phase,
next to ``hdem_flowacc_u8_dev`` on the same codes in the same process.

Input: the D8 codes of the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at
4096^2 and 16384^2, made on the device.  Per shape and per weight type (float32 weights in
[0, 100) at frac_bits 16 writing ``value``; uint8 ones writing ``sum``): warm-up calls, then
--reps calls, every one kept, of phase A (weights quantised, in-tile pass), B (exit forest),
C (in-tile pass again, writes the output) and their sum; then the same for ``FlowAccumulation``
and the ratio of the two medians.

    python tools/flowsum_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2]
"""
import argparse
import json

import numpy as np

from d8_inputs import filled_codes
from hydrodem_amd import backend, flowsum


def weights_of(kind, shape, ctx):
    if kind == "u8":
        host = np.ones(shape, np.uint8)
    else:
        host = np.random.default_rng(shape[0]).random(shape, dtype=np.float32) * np.float32(100)
    return backend.DeviceRaster.from_host(host, dtype=host.dtype, ctx=ctx)


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


def run(size, reps, warmup):
    ctx = backend.context()
    codes = filled_codes(size)
    records = []
    try:
        ctx.profile(True)
        with backend.DeviceRaster.empty(codes.shape, np.uint32, ctx) as acc:
            base = summary(timed(lambda: backend.flowacc_dev(codes, acc)[1], reps, warmup))
        for kind, want, dtype in (("f32", "value", np.float32), ("u8", "sum", np.int64)):
            with weights_of(kind, codes.shape, ctx) as w, \
                    backend.DeviceRaster.empty(codes.shape, dtype, ctx) as out:
                frac_bits = 16 if kind == "f32" else 0
                got = summary(timed(
                    lambda: flowsum.flowsum_dev(codes, w, frac_bits, want, out={want: out})[1],
                    reps, warmup))
            records.append({"size": size, "weights": kind, "output": want,
                            "ms_A_B_C_total": got,
                            "ratio_to_flowacc": round(got["median"][3] / base["median"][3], 3),
                            "gcells_per_s": round(size * size / got["median"][3] / 1e6, 2)})
        records.append({"size": size, "operator": "FlowAccumulation", "ms_A_B_C_total": base,
                        "gcells_per_s": round(size * size / base["median"][3] / 1e6, 2)})
    finally:
        ctx.profile(False)
        codes.free()
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("flowsum_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",")):
        for record in run(size, a.reps, a.warmup):
            print(json.dumps(record), flush=True)


if __name__ == "__main__":
    main()
