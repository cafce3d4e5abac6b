"""HIP-event times of the D-infinity distance down (``hdem_dinfdist_u32`` with ``HDEM_ON_DEVICE``)
against ``DInfFlowAccumulation`` on the same words, and of ``DemToDInfHAND`` end to end next to
``DemToHAND``.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2,
its own D8 codes and their D8 accumulation, made on the device; the D-infinity words are those of
the filled raster with the codes as fallback.  Per size: warm-up calls, then --reps rounds that
alternate, in one process, one call of each timed form and one of the D-infinity accumulation.
Every repeat is kept: each time is printed as its median with min ... max.

  forms                    horizontal average to ``acc >= 100``; vertical average to ``acc >= 100``
                           (the D-infinity HAND); horizontal average to the outlet (no streams)
  ms_classify / relax / final   the three phases of a form; relax includes the host's read of one
                           word per round
  ms_total                 their sum;  over_dinfacc: the ratio of its median to ms_dinfacc's
  rounds, visits_per_tile  the schedule: rounds that had work, tile visits over tiles
  us_per_round             ms_relax over rounds
  stop_share, unreached_share   cells of the stop set and NaN results over all cells
  ms_dinfacc               the three phases of ``hdem_dinfacc_u32_dev`` on the same words, its
                           rounds and visits per tile
  chain                    ``DemToDInfHAND.apply_device`` and ``DemToHAND.apply_device`` at the same
                           threshold on the unfilled raster (--chain-reps, after one warm-up each,
                           alternating): host clock round the call, and the event time of the
                           distance stage (``DInfDistanceDown`` / ``HeightAboveDrainage``)

    python tools/dinfdist_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
                                  [--threshold 100] [--chain-reps 3]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, dinf

FORMS = (("horizontal_to_streams", "horizontal", True), ("vertical_to_streams", "vertical", True),
         ("horizontal_to_outlet", "horizontal", False))


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def phases_of(stats):
    return stats["ms_classify"], stats["ms_relax"], stats["ms_final"]


def chain_times(dz, threshold, reps):
    """The two HAND chains, alternating: host clock round the call and the distance stage."""
    chains = {"DemToDInfHAND": (hd.DemToDInfHAND(threshold=threshold), "DInfDistanceDown",
                                ("ms_classify", "ms_relax", "ms_final")),
              "DemToHAND": (hd.DemToHAND(threshold=threshold), "HeightAboveDrainage",
                            ("ms_tile", "ms_forest", "ms_final"))}
    wall = {name: [] for name in chains}
    stage = {name: [] for name in chains}
    for k in range(1 + reps):
        for name, (chain, last, keys) in chains.items():
            dz.ctx.synchronize()
            t0 = time.perf_counter()
            with chain.apply_device(dz):
                t1 = time.perf_counter()
            if k:
                wall[name].append((t1 - t0) * 1e3)
                stage[name].append(sum(chain.stats[last].get(key, 0.0) for key in keys))
    out = {name: {"wall_ms": spread(wall[name]), "ms_distance_stage": spread(stage[name])}
           for name in chains}
    out["wall_ratio"] = round(float(np.median(wall["DemToDInfHAND"]) /
                                    np.median(wall["DemToHAND"])), 3)
    return out


def run(size, variant, reps, warmup, threshold, chain_reps):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    acc, _ = backend.flowacc_dev(codes)
    words, _, _ = dinf.dinf_dev(filled, 1.0, codes)
    out = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    try:
        ctx.profile(True)
        kept = {name: {"phases": [], "schedule": []} for name, _, _ in FORMS}
        last = {}
        area_phases, area_schedule = [], []
        for k in range(warmup + reps):
            for name, kind, to_streams in FORMS:
                _, st = dinf.dinfdist_dev(words, acc if to_streams else None,
                                          threshold if to_streams else None,
                                          filled if kind != "horizontal" else None, 1.0, kind,
                                          "average", out=out)
                last[name] = st
                if k >= warmup:
                    kept[name]["phases"].append(phases_of(st))
                    kept[name]["schedule"].append((int(st["rounds"]), int(st["tile_visits"])))
            _, st = dinf.dinfacc_dev(words, 16, "value", {"value": area})
            if k >= warmup:
                area_phases.append(phases_of(st))
                area_schedule.append((int(st["rounds"]), int(st["tile_visits"])))
        chain = chain_times(dz, threshold, chain_reps) if chain_reps else None
        ctx.profile(False)
        tiles = tiles_of(size, size)
        cells = size * size
        names = ("classify", "relax", "final")
        area_total = [sum(p) for p in area_phases]
        result = {"size": size, "variant": variant, "reps": reps, "threshold": threshold,
                  "tiles": tiles, "ms_dinfacc": spread(area_total),
                  "dinfacc": {**{f"ms_{n}": spread([p[j] for p in area_phases])
                                 for j, n in enumerate(names)},
                              "rounds": [r for r, _ in area_schedule],
                              "visits_per_tile": [round(v / tiles, 2) for _, v in area_schedule]},
                  "split_share": round(st["split_cells"] / cells, 4), "chain": chain}
        for name, _, _ in FORMS:
            phases, schedule = kept[name]["phases"], kept[name]["schedule"]
            total = [sum(p) for p in phases]
            relax = float(np.median([p[1] for p in phases]))
            result[name] = {
                **{f"ms_{n}": spread([p[j] for p in phases]) for j, n in enumerate(names)},
                "ms_total": spread(total),
                "over_dinfacc": round(float(np.median(total) / np.median(area_total)), 3),
                "rounds": [r for r, _ in schedule],
                "visits_per_tile": [round(v / tiles, 2) for _, v in schedule],
                "us_per_round": round(relax * 1e3 / max(1, int(np.median([r for r, _ in
                                                                          schedule]))), 1),
                "stop_share": round(last[name]["stop_cells"] / cells, 4),
                "unreached_share": round(last[name]["unreached_cells"] / cells, 4)}
        return result
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, acc, words, out, area):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=100)
    ap.add_argument("--chain-reps", type=int, default=3)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("dinfdist_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup, a.threshold, a.chain_reps)),
              flush=True)


if __name__ == "__main__":
    main()
