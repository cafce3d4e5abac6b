"""HIP-event times of the longest upstream D8 flow length (``hdem_upstream_u8_dev``), phase by
phase, next to D8 flow accumulation on the same codes in the same process.

Input: the D8 codes of the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough"
and "srtm") at 4096^2 and 16384^2, made on the device.  Per shape: warm-up calls, then the
median of --reps calls of phase A (in-tile walks, perimeter paths), B (exit forest) and C
(seeded in-tile walks, writes the outputs) and their sum, with the exit-forest size, the
longest forest walk and the number of heads; then the same for ``backend.flowacc_dev`` and
the ratio of the two sums.  ``--outputs`` chooses what the upstream call writes (default: the
float32 length alone, 4 B per cell as flow accumulation writes).

    python tools/upstream_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2]
"""
import argparse
import json

import numpy as np

from d8_inputs import filled_codes
from hydrodem_amd import backend, upstream

PHASES = ("ms_tile", "ms_forest", "ms_final")


def medians(call, reps, warmup):
    """Per-phase medians of ``call() -> stats`` and the last stats dict."""
    for _ in range(warmup):
        call()
    rows = [call() for _ in range(reps)]
    return [float(np.median([r[k] for r in rows])) for k in PHASES], rows[-1]


def run(size, variant, want, reps, warmup):
    ctx = backend.context()
    codes = filled_codes(size, variant)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)

    def up_call():
        outs, st = upstream.upstream_dev(codes, 1.0, want)
        for raster in outs.values():
            raster.free()
        return st

    try:
        ctx.profile(True)
        up, st = medians(up_call, reps, warmup)
        fa, fst = medians(lambda: backend.flowacc_dev(codes, acc)[1], reps, warmup)
    finally:
        ctx.profile(False)
        acc.free()
        codes.free()
    cells = size * size
    return {"size": size, "variant": variant, "outputs": list(want),
            "ms_A_tile": round(up[0], 4), "ms_B_forest": round(up[1], 4),
            "ms_C_final": round(up[2], 4), "ms_ABC": round(sum(up), 4),
            "gcells_per_s": round(cells / sum(up) / 1e6, 2),
            "exits": int(st["exits"]), "max_hops": int(st["max_hops"]),
            "heads": int(st["heads"]),
            "flowacc_ms_A_tile": round(fa[0], 4), "flowacc_ms_B_forest": round(fa[1], 4),
            "flowacc_ms_C_final": round(fa[2], 4), "flowacc_ms_ABC": round(sum(fa), 4),
            "flowacc_max_hops": int(fst["max_hops"]),
            "ratio_to_flowacc": round(sum(up) / sum(fa), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variants", default="rough,srtm")
    ap.add_argument("--outputs", default="length")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("upstream_time.py needs a GPU")
    for variant in a.variants.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            print(json.dumps(run(size, variant, tuple(a.outputs.split(",")), a.reps, a.warmup)),
                  flush=True)


if __name__ == "__main__":
    main()
