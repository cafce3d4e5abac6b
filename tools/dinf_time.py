"""HIP-event times of the D-infinity operators (``hdem_dinf_f32_dev``, ``hdem_dinfacc_u32_dev``,
``hdem_dinfsum_u32_dev``) against ``FlowAccumulation`` on the same fill, and of the wetness index
from their area (``hdem_terrain_area_f32_dev``) against ``hdem_terrain_f32_dev``.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2
and its own D8 codes, made on the device; the D-infinity words are those of the filled raster
with the codes as fallback.  Per size: warm-up calls, then --reps rounds that alternate, in one
process, one call of the direction, one of the D-infinity accumulation, one of the weighted one
(float32 weights in [0, 2), ``value`` out), one of the D8 accumulation and the three wetness
calls (``twi`` out) on the filled raster.  Every repeat is kept: each time is printed as its
median with min ... max.

  ms_direction             the direction launch (words only)
  ms_classify / relax / final   the three phases of the accumulation; relax includes the
                           host's read of one word per round
  ms_dinfacc               their sum;  wall_ms_dinfacc  host clock round the synchronising call
  ms_flowacc               the three phases of ``hdem_flowacc_u8_dev`` on the fill's codes
  dinfacc_over_flowacc     the ratio of the two medians
  rounds, visits_per_tile  the schedule: rounds that had work, tile visits over tiles
  us_per_round             ms_relax over rounds
  weighted                 the same phases, sum, rounds and visits of ``hdem_dinfsum_u32_dev``, and
                           weighted_over_unweighted: the ratio of the medians, per phase and in all
  ms_twi_acc               ``hdem_terrain_f32_dev`` on the uint32 D8 accumulation, Horn's slope
  ms_twi_area / _given     ``hdem_terrain_area_f32_dev`` on the float32 D-infinity area, Horn's
                           slope / the D-infinity slope as given; their ratios to ms_twi_acc
  chain                    ``DemToDInfWetness.apply_device`` on the unfilled raster (--chain-reps,
                           after one warm-up): host clock round the call, its stage times, and what
                           they leave of it (the fill + D8 call, allocations, the host)

    python tools/dinf_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
                              [--chain-reps 3]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, dinf, terrain


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def ratio(a, b):
    return round(float(np.median(a) / np.median(b)), 3)


def chain_times(dz, reps):
    """``DemToDInfWetness.apply_device``: host clock round the call and the stage times."""
    chain = hd.DemToDInfWetness()
    wall, stage = [], {}
    for k in range(1 + reps):
        dz.ctx.synchronize()
        t0 = time.perf_counter()
        with chain.apply_device(dz):
            t1 = time.perf_counter()
        if k == 0:
            continue
        wall.append((t1 - t0) * 1e3)
        acc = chain.stats["DInfFlowAccumulation"]
        times = {"direction": chain.stats["DInfFlowDirection"]["ms_total"],
                 "accumulation": acc["ms_classify"] + acc["ms_relax"] + acc["ms_final"],
                 "wetness": chain.stats["AreaWetnessIndex"]["ms_total"]}
        # the fill has no event times of its own: the fill + D8 call, the allocations and the
        # host's share are what the three stages leave of the host clock
        times["fill_and_rest"] = wall[-1] - sum(times.values())
        for name, ms in times.items():
            stage.setdefault(name, []).append(ms)
    return {"wall_ms": spread(wall), **{f"ms_{n}": spread(v) for n, v in stage.items()}}


def run(size, variant, reps, warmup, chain_reps):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    words = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    slope = None
    area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    warea = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    twi = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    weights = backend.DeviceRaster.from_host(
        np.random.default_rng(size).random(codes.shape, dtype=np.float32) * np.float32(2))
    try:
        ctx.profile(True)
        direction, phases, wall, d8, schedule = [], [], [], [], []
        wphases, wschedule, twi_acc, twi_area, twi_given = [], [], [], [], []
        for k in range(warmup + reps):
            _, _, st_dir = dinf.dinf_dev(filled, 1.0, codes, out=words)
            ctx.synchronize()
            t0 = time.perf_counter()
            _, st = dinf.dinfacc_dev(words, 16, "value", {"value": area})
            t1 = time.perf_counter()
            _, st_w = dinf.dinfsum_dev(words, weights, 16, "value", {"value": warea})
            _, st_d8 = backend.flowacc_dev(codes, out=acc)
            if k == 0:          # the D-infinity slope, once: the timed direction writes words only
                slope = dinf.dinf_dev(filled, 1.0, codes, ("slope",), out=words)[1]["slope"]
            _, st_ta = terrain.terrain_dev(filled, "twi", accumulation=acc, out={"twi": twi})
            _, st_tf = terrain.terrain_area_dev(filled, "twi", area=area, out={"twi": twi})
            _, st_tg = terrain.terrain_area_dev(filled, "twi", area=area, given_slope=slope,
                                                slope="given", out={"twi": twi})
            if k >= warmup:
                wphases.append((st_w["ms_classify"], st_w["ms_relax"], st_w["ms_final"]))
                wschedule.append((int(st_w["rounds"]), int(st_w["tile_visits"])))
                twi_acc.append(st_ta["ms_total"])
                twi_area.append(st_tf["ms_total"])
                twi_given.append(st_tg["ms_total"])
                direction.append(st_dir["ms_total"])
                phases.append((st["ms_classify"], st["ms_relax"], st["ms_final"]))
                wall.append((t1 - t0) * 1e3)
                d8.append(st_d8["ms_tile"] + st_d8["ms_forest"] + st_d8["ms_final"])
                schedule.append((int(st["rounds"]), int(st["tile_visits"])))
        chain = chain_times(dz, chain_reps) if chain_reps else None
        ctx.profile(False)
        total = [sum(p) for p in phases]
        wtotal = [sum(p) for p in wphases]
        tiles = tiles_of(size, size)
        names = ("classify", "relax", "final")
        weighted = {**{f"ms_{n}": spread([p[j] for p in wphases]) for j, n in enumerate(names)},
                    "ms_dinfsum": spread(wtotal), "rounds": [r for r, _ in wschedule],
                    "visits_per_tile": [round(v / tiles, 2) for _, v in wschedule],
                    "nan_weights": int(st_w["nan_weights"]), "total": int(st_w["total"])}
        over = {n: ratio([p[j] for p in wphases], [p[j] for p in phases])
                for j, n in enumerate(names)}
        over["all"] = ratio(wtotal, total)
        return {"size": size, "variant": variant, "reps": reps,
                "weighted": weighted, "weighted_over_unweighted": over,
                "ms_twi_acc": spread(twi_acc), "ms_twi_area": spread(twi_area),
                "ms_twi_given": spread(twi_given),
                "twi_area_over_acc": ratio(twi_area, twi_acc),
                "twi_given_over_acc": ratio(twi_given, twi_acc), "chain": chain,
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
        for raster in (dz, filled, codes, words, slope, area, warea, twi, acc, weights):
            if raster is not None:
                raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chain-reps", type=int, default=3)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("dinf_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup, a.chain_reps)), flush=True)


if __name__ == "__main__":
    main()
