"""HIP-event times of the cost distance (``hdem_costdistance_f32`` with ``HDEM_ON_DEVICE``) against
``EuclideanDistance`` on the same sources and ``DInfDistanceDown`` to the same streams.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2,
its own D8 codes and their flow accumulation, made on the device; the sources are the cells with
``acc >= 100``.  Per size: warm-up rounds, then --reps rounds that alternate, in one process, one
call of each timed form, one of the Euclidean distance and one of the D-infinity distance down.
Every repeat is kept: each time is printed as its median with min ... max.

  forms                    uniform (cost 1 everywhere) and slope (cost 1 + tangent, the tangent of
                           ``TerrainAttributes`` on the filled raster), each for ``distance`` alone
                           and for ``distance`` + ``nearest`` (the trace over the back links)
  ms_classify / relax / final / trace   the phases of a form; relax includes the host's read of one
                           word per round
  ms_total                 their sum;  over_euclidean, over_distdown: the ratio of its median to
                           ms_euclidean's and to ms_distdown's
  rounds, visits_per_tile  the schedule: rounds that had work, tile visits over tiles
  us_per_round             ms_relax over rounds
  source_share, tie_share  sources and tie cells over all cells
  ms_euclidean             the three phases of ``hdem_proximity_dev`` (distance) on the same sources
  ms_distdown              the three phases of ``hdem_dinfdist_u32``: horizontal average to the
                           same streams, with its rounds and visits per tile

    python tools/costdistance_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
"""
import argparse
import json

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
from hydrodem_amd import backend, costdistance, dinf, proximity, terrain

THRESHOLD = 100
FORMS = tuple((f"{friction}_{'+'.join(want)}", friction, want)
              for friction in ("uniform", "slope")
              for want in (("distance",), ("distance", "nearest")))
NAMES = ("classify", "relax", "final", "trace")


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def summary(phases, names):
    return {**{f"ms_{n}": spread([p[j] for p in phases]) for j, n in enumerate(names)},
            "ms_total": spread([sum(p) for p in phases])}


def run(size, variant, reps, warmup):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    acc, _ = backend.flowacc_dev(codes)
    words, _, _ = dinf.dinf_dev(filled, 1.0, codes)
    slopes, _ = terrain.terrain_dev(filled, ("tangent",))
    friction = np.minimum(slopes["tangent"].to_host(), np.float32(1000)) + np.float32(1)
    slopes["tangent"].free()
    costs = {"uniform": backend.DeviceRaster.from_host(np.ones((size, size), np.float32)),
             "slope": backend.DeviceRaster.from_host(friction)}
    del friction
    outs = {"distance": backend.DeviceRaster.empty(codes.shape, np.float32, ctx),
            "nearest": backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)}
    try:
        ctx.profile(True)
        kept = {name: [] for name in [f[0] for f in FORMS] + ["euclidean", "distdown"]}
        schedule = {name: [] for name in kept}
        last = {}
        for k in range(warmup + reps):
            for name, which, want in FORMS:
                _, st = costdistance.costdistance_dev(costs[which], acc, THRESHOLD, want,
                                                      out={n: outs[n] for n in want})
                last[name] = st
                if k >= warmup:
                    kept[name].append(tuple(st[f"ms_{n}"] for n in NAMES))
                    schedule[name].append((int(st["rounds"]), int(st["tile_visits"])))
            _, st = proximity.proximity_dev(acc, THRESHOLD, ("distance",),
                                            out={"distance": outs["distance"]})
            if k >= warmup:
                kept["euclidean"].append((st["ms_row"], st["ms_column"], st["ms_final"]))
            _, st = dinf.dinfdist_dev(words, acc, THRESHOLD, None, 1.0, "horizontal", "average",
                                      out=outs["distance"])
            if k >= warmup:
                kept["distdown"].append((st["ms_classify"], st["ms_relax"], st["ms_final"]))
                schedule["distdown"].append((int(st["rounds"]), int(st["tile_visits"])))
        ctx.profile(False)
        tiles = tiles_of(size, size)
        cells = size * size
        result = {"size": size, "variant": variant, "reps": reps, "tiles": tiles,
                  "euclidean": summary(kept["euclidean"], ("row", "column", "final")),
                  "distdown": {**summary(kept["distdown"], NAMES[:3]),
                               "rounds": [r for r, _ in schedule["distdown"]],
                               "visits_per_tile": [round(v / tiles, 2)
                                                   for _, v in schedule["distdown"]]}}
        for other in ("euclidean", "distdown"):
            result[f"ms_{other}"] = result[other]["ms_total"]
        for name, _, _ in FORMS:
            total = float(np.median([sum(p) for p in kept[name]]))
            relax = float(np.median([p[1] for p in kept[name]]))
            rounds = max(1, int(np.median([r for r, _ in schedule[name]])))
            result[name] = {
                **summary(kept[name], NAMES),
                "rounds": [r for r, _ in schedule[name]],
                "visits_per_tile": [round(v / tiles, 2) for _, v in schedule[name]],
                "over_euclidean": round(total / result["ms_euclidean"]["median"], 3),
                "over_distdown": round(total / result["ms_distdown"]["median"], 3),
                "us_per_round": round(relax * 1e3 / rounds, 1),
                "source_share": round(last[name]["sources"] / cells, 4),
                "tie_share": round(last[name]["tie_cells"] / cells, 4)}
        return result
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, acc, words, *costs.values(), *outs.values()):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("costdistance_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
