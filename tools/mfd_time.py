"""HIP-event times of the MFD operators (``hdem_mfd_f32``, ``hdem_mfdacc_u64`` on device pointers)
against the D-infinity accumulation and ``FlowAccumulation`` on the same fill.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2
and its own D8 codes, made on the device; the MFD and the D-infinity words are those of the
filled raster with the codes as fallback.  Per size: warm-up calls, then --reps rounds that
alternate, in one process, one call of the MFD direction (``freeman``: the power is taken),
one of the MFD accumulation, one of the D-infinity accumulation and one of the D8 accumulation.
Every repeat is kept: each time is printed as its median with min ... max.

  ms_direction             the MFD direction launch (words only)
  ms_classify / relax / final   the three phases of the MFD accumulation; relax includes the
                           host's read of one word per round
  ms_mfdacc                their sum;  wall_ms_mfdacc  host clock round the synchronising call
  ms_dinfacc               the three phases of ``hdem_dinfacc_u32_dev`` on the D-infinity words
  ms_flowacc               the three phases of ``hdem_flowacc_u8_dev`` on the fill's codes
  mfdacc_over_dinfacc, mfdacc_over_flowacc   ratios of the medians
  rounds, visits_per_tile  the schedule of the MFD accumulation (and dinf_rounds,
                           dinf_visits_per_tile of the D-infinity one)
  split_share              cells with more than one receiver over all cells

    python tools/mfd_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
                             [--method freeman]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
from hydrodem_amd import backend, dinf, mfd


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def ratio(a, b):
    return round(float(np.median(a) / np.median(b)), 3)


def phases_of(stats):
    return stats["ms_classify"], stats["ms_relax"], stats["ms_final"]


def run(size, variant, reps, warmup, method):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    dz.free()
    words = backend.DeviceRaster.empty(codes.shape, np.uint64, ctx)
    area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    dinf_area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    dinf_words = dinf.dinf_dev(filled, 1.0, codes)[0]
    try:
        ctx.profile(True)
        direction, phases, wall, dinf_phases, d8, schedule, dinf_schedule = [], [], [], [], [], [], []
        for k in range(warmup + reps):
            _, _, st_dir = mfd.mfd_dev(filled, method, None, 1.0, codes, out=words)
            ctx.synchronize()
            t0 = time.perf_counter()
            _, st = mfd.mfdacc_dev(words, None, 16, "value", {"value": area})
            t1 = time.perf_counter()
            _, st_inf = dinf.dinfacc_dev(dinf_words, 16, "value", {"value": dinf_area})
            _, st_d8 = backend.flowacc_dev(codes, out=acc)
            if k >= warmup:
                direction.append(st_dir["ms_total"])
                phases.append(phases_of(st))
                wall.append((t1 - t0) * 1e3)
                dinf_phases.append(phases_of(st_inf))
                d8.append(st_d8["ms_tile"] + st_d8["ms_forest"] + st_d8["ms_final"])
                schedule.append((int(st["rounds"]), int(st["tile_visits"])))
                dinf_schedule.append((int(st_inf["rounds"]), int(st_inf["tile_visits"])))
        ctx.profile(False)
        total = [sum(p) for p in phases]
        dinf_total = [sum(p) for p in dinf_phases]
        tiles = tiles_of(size, size)
        return {"size": size, "variant": variant, "reps": reps, "method": method,
                "ms_direction": spread(direction),
                "ms_classify": spread([p[0] for p in phases]),
                "ms_relax": spread([p[1] for p in phases]),
                "ms_final": spread([p[2] for p in phases]),
                "ms_mfdacc": spread(total), "wall_ms_mfdacc": spread(wall),
                "ms_dinfacc": spread(dinf_total), "ms_flowacc": spread(d8),
                "mfdacc_over_dinfacc": ratio(total, dinf_total),
                "mfdacc_over_flowacc": ratio(total, d8),
                "rounds": [r for r, _ in schedule], "tiles": tiles,
                "visits_per_tile": [round(v / tiles, 2) for _, v in schedule],
                "dinf_rounds": [r for r, _ in dinf_schedule],
                "dinf_visits_per_tile": [round(v / tiles, 2) for _, v in dinf_schedule],
                "us_per_round": round(float(np.median([p[1] for p in phases])) * 1e3 /
                                      max(1, int(np.median([r for r, _ in schedule]))), 1),
                "split_share": round(st["split_cells"] / (size * size), 4),
                "dinf_split_share": round(st_inf["split_cells"] / (size * size), 4),
                "fallback_cells": int(st_dir["fallback_cells"])}
    finally:
        ctx.profile(False)
        for raster in (filled, codes, words, area, dinf_area, acc, dinf_words):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--method", default="freeman")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("mfd_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup, a.method)), flush=True)


if __name__ == "__main__":
    main()
