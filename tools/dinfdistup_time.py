"""HIP-event times of the D-infinity distance up (``hdem_dinfdistup_u32`` with ``HDEM_ON_DEVICE``)
against ``DInfFlowAccumulation`` and against ``DInfDistanceDown`` to the outlet on the same words.

Input: the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2
and its own D8 codes, made on the device; the D-infinity words are those of the filled raster with
the codes as fallback.  Per size: warm-up rounds, then --reps rounds that alternate, in one
process, one call of each timed form, one of the D-infinity accumulation and one of the distance
down.  Every repeat is kept: each time is printed as its median with min ... max.

  forms                    horizontal and vertical average, each at min_share 16384 (a half) and
                           1 (every link)
  ms_classify / relax / final   the three phases of a form; relax includes the host's read of one
                           word per round
  ms_total                 their sum;  over_dinfacc, over_distdown: the ratio of its median to
                           ms_dinfacc's and to ms_distdown's
  rounds, visits_per_tile  the schedule: rounds that had work, tile visits over tiles
  us_per_round             ms_relax over rounds
  ridge_share, merge_share, ignored_per_cell   ridge cells, cells with several counted donors and
                           links below min_share, over all cells
  ms_dinfacc               the three phases of ``hdem_dinfacc_u32_dev`` on the same words, its
                           rounds and visits per tile
  ms_distdown              the same of ``hdem_dinfdist_u32``: horizontal average to the outlet

    python tools/dinfdistup_time.py [--sizes 4096,16384] [--variant rough] [--reps 7] [--warmup 2]
"""
import argparse
import json

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
from hydrodem_amd import backend, dinf

FORMS = tuple((f"{kind}_{share}", kind, share)
              for kind in ("horizontal", "vertical") for share in (16384, 1))
NAMES = ("classify", "relax", "final")


def spread(values):
    """median, min and max of the kept repeats, rounded for print."""
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4),
            "max": round(float(max(values)), 4)}


def phases_of(stats):
    return stats["ms_classify"], stats["ms_relax"], stats["ms_final"]


def summary(phases, schedule, tiles):
    """The phases, their sum and the schedule of one operator's kept repeats."""
    return {**{f"ms_{n}": spread([p[j] for p in phases]) for j, n in enumerate(NAMES)},
            "ms_total": spread([sum(p) for p in phases]),
            "rounds": [r for r, _ in schedule],
            "visits_per_tile": [round(v / tiles, 2) for _, v in schedule]}


def run(size, variant, reps, warmup):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    words, _, _ = dinf.dinf_dev(filled, 1.0, codes)
    out = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    area = backend.DeviceRaster.empty(codes.shape, np.float32, ctx)
    try:
        ctx.profile(True)
        others = ("dinfacc", "distdown")
        kept = {name: {"phases": [], "schedule": []} for name in [f[0] for f in FORMS] + [*others]}
        last = {}

        def keep(name, st, k):
            last[name] = st
            if k >= warmup:
                kept[name]["phases"].append(phases_of(st))
                kept[name]["schedule"].append((int(st["rounds"]), int(st["tile_visits"])))

        for k in range(warmup + reps):
            for name, kind, share in FORMS:
                _, st = dinf.dinfdistup_dev(words, filled if kind != "horizontal" else None, 1.0,
                                            kind, "average", out=out, min_share=share)
                keep(name, st, k)
            _, st = dinf.dinfacc_dev(words, 16, "value", {"value": area})
            keep("dinfacc", st, k)
            _, st = dinf.dinfdist_dev(words, None, None, None, 1.0, "horizontal", "average",
                                      out=out)
            keep("distdown", st, k)
        ctx.profile(False)
        tiles = tiles_of(size, size)
        cells = size * size
        result = {"size": size, "variant": variant, "reps": reps, "tiles": tiles}
        for name in others:
            result[name] = summary(kept[name]["phases"], kept[name]["schedule"], tiles)
            result[f"ms_{name}"] = result[name]["ms_total"]
        for name, _, _ in FORMS:
            phases, schedule = kept[name]["phases"], kept[name]["schedule"]
            total = float(np.median([sum(p) for p in phases]))
            relax = float(np.median([p[1] for p in phases]))
            rounds = max(1, int(np.median([r for r, _ in schedule])))
            result[name] = {
                **summary(phases, schedule, tiles),
                "over_dinfacc": round(total / result["ms_dinfacc"]["median"], 3),
                "over_distdown": round(total / result["ms_distdown"]["median"], 3),
                "us_per_round": round(relax * 1e3 / rounds, 1),
                "ridge_share": round(last[name]["ridge_cells"] / cells, 4),
                "merge_share": round(last[name]["merge_cells"] / cells, 4),
                "ignored_per_cell": round(last[name]["ignored_links"] / cells, 4)}
        return result
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, words, out, area):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variant", default="rough")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("dinfdistup_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        print(json.dumps(run(size, a.variant, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
