"""HIP-event times of the D8 flat resolution (``hdem_resolve_flats_u8_dev``), phase by phase,
and the exact route against the gradient route.

Input: the epsilon = 0 sink fill of ``hdem_synth.synth_dem`` (both variants) at 4096^2,
16384^2 and 32768^2 and its own D8 codes, made on the device.  Per shape and variant: warm-up
calls, then the median of --reps calls of the three phases (classify; relax, the host's read
of one word per round included; final) and their sum, with the rounds that had work, the
tiles that hold a flat cell (the visits of the first round), the tile visits summed over the
rounds and their mean per round, the largest distance and the number of flat cells.  The
call has no kernel id: its total is the sum of its three phases (the events are back to back
on the context's stream).

``--routes`` adds the comparison the operator exists for, wall clock round synchronising
calls on device rasters, alternating in one process: fill(epsilon = 0) + D8 +
``ResolveFlats`` against fill(epsilon = 1e-3) + D8, the median of --reps after --warmup
each.

    python tools/flats_time.py [--sizes 4096,16384,32768] [--variants rough,srtm] [--reps 5]
                               [--warmup 2] [--routes]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import tiles_of
import hdem_synth
from hydrodem_amd import backend


def median_of(rows, key):
    return float(np.median([r[key] for r in rows]))


def run(size, variant, reps, warmup, routes):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    del z
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=0.0)
    out = backend.DeviceRaster.empty(codes.shape, np.uint8, ctx)
    try:
        ctx.profile(True)
        rows = []
        for k in range(warmup + reps):
            _, _, st = backend.resolve_flats_dev(codes, filled, out=out)
            if k >= warmup:
                rows.append(st)
        ctx.profile(False)
        phases = [median_of(rows, k) for k in ("ms_classify", "ms_relax", "ms_final")]
        st = rows[-1]
        row = {"size": size, "variant": variant,
               "ms_classify": round(phases[0], 4), "ms_relax": round(phases[1], 4),
               "ms_final": round(phases[2], 4), "ms_total": round(sum(phases), 4),
               "rounds": [int(r["rounds"]) for r in rows],
               "tiles": tiles_of(size, size), "active_tiles": int(st["active_tiles"]),
               "tile_visits": int(st["tile_visits"]),
               "visits_per_round": round(st["tile_visits"] / max(1, st["rounds"]), 1),
               "max_distance": int(st["max_distance"]), "flat_cells": int(st["flat_cells"]),
               "flat_share": round(st["flat_cells"] / (size * size), 4),
               "unresolved": int(st["unresolved"]), "reps": reps}
        if routes:
            exact, gradient = [], []
            for k in range(warmup + reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                backend.sinkfill_d8_dev(dz, eps=0.0, out=filled, codes=codes)
                t1 = time.perf_counter()
                backend.resolve_flats_dev(codes, filled, out=codes)
                t2 = time.perf_counter()
                backend.sinkfill_d8_dev(dz, eps=1e-3, out=filled, codes=out)
                t3 = time.perf_counter()
                if k >= warmup:
                    exact.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
                    gradient.append((t3 - t2) * 1e3)
            fill0 = float(np.median([e[0] for e in exact]))
            resolve = float(np.median([e[1] for e in exact]))
            both = float(np.median([sum(e) for e in exact]))
            grad = float(np.median(gradient))
            row.update({"wall_ms_fill0_d8": round(fill0, 3), "wall_ms_resolve": round(resolve, 3),
                        "wall_ms_exact_route": round(both, 3),
                        "wall_ms_gradient_route": round(grad, 3),
                        "exact_over_gradient": round(both / grad, 3)})
        return row
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, out):
            raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,32768")
    ap.add_argument("--variants", default="rough,srtm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", action="store_true")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("flats_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",") if s):
        for variant in (v for v in a.variants.split(",") if v):
            print(json.dumps(run(size, variant, a.reps, a.warmup, a.routes)), flush=True)


if __name__ == "__main__":
    main()
