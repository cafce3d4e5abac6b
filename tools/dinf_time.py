"""HIP-event times of the D-infinity operators (``hdem_dinf_f32_dev``, ``hdem_dinfacc_u32_dev``)
against ``FlowAccumulation`` on the same fill.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2
and its own D8 codes, made on the device; the D-infinity words are those of the filled raster
with the codes as fallback.  Per size: warm-up calls, then --reps rounds that alternate, in one
process, one call of the direction, one of the D-infinity accumulation and one of the D8
accumulation.  Every repeat is kept: each time is printed as its median with min ... max.

  ms_direction             the direction launch (words only)
  ms_classify / relax / final   the three phases of the accumulation; relax includes the
                           host's read of one word per round
  ms_dinfacc               their sum;  wall_ms_dinfacc  host clock round the synchronising call
  ms_flowacc               the three phases of ``hdem_flowacc_u8_dev`` on the fill's codes
  dinfacc_over_flowacc     the ratio of the two medians
  rounds, visits_per_tile  the schedule: rounds that had work, tile visits over tiles
  us_per_round             ms_relax over rounds

    python tools/dinf_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
from hydrodem_amd import backend, dinf


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def run(size, variant, reps, warmup):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    words = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    try:
        ctx.profile(True)
        direction, phases, wall, d8, schedule = [], [], [], [], []
        for k in range(warmup + reps):
            _, _, st_dir = dinf.dinf_dev(filled, 1.0, codes, out=words)
            ctx.synchronize()
            t0 = time.perf_counter()
            _, st = dinf.dinfacc_dev(words, 16, "value", {"value": area})
            t1 = time.perf_counter()
            _, st_d8 = backend.flowacc_dev(codes, out=acc)
            if k >= warmup:
                direction.append(st_dir["ms_total"])
                phases.append((st["ms_classify"], st["ms_relax"], st["ms_final"]))
                wall.append((t1 - t0) * 1e3)
                d8.append(st_d8["ms_tile"] + st_d8["ms_forest"] + st_d8["ms_final"])
                schedule.append((int(st["rounds"]), int(st["tile_visits"])))
        ctx.profile(False)
        total = [sum(p) for p in phases]
        tiles = tiles_of(size, size)
        return {"size": size, "variant": variant, "reps": reps,
                "ms_direction": spread(direction),
                "ms_classify": spread([p[0] for p in phases]),
                "ms_relax": spread([p[1] for p in phases]),
                "ms_final": spread([p[2] for p in phases]),
                "ms_dinfacc": spread(total), "wall_ms_dinfacc": spread(wall),
                "ms_flowacc": spread(d8),
                "dinfacc_over_flowacc": round(float(np.median(total) / np.median(d8)), 2),
                "rounds": [r for r, _ in schedule], "tiles": tiles,
                "visits_per_tile": [round(v / tiles, 2) for _, v in schedule],
                "us_per_round": round(float(np.median([p[1] for p in phases])) * 1e3 /
                                      max(1, int(np.median([r for r, _ in schedule]))), 1),
                "split_share": round(st["split_cells"] / (size * size), 4),
                "fallback_cells": int(st_dir["fallback_cells"])}
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, words, area, acc):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("dinf_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
