"""HIP-event times of D8 watershed labelling (``hdem_watershed_u8_dev``), phase by phase.

Input: the rasters of ``tools/flowacc_time.py`` -- the D8 codes of the epsilon = 1e-3 sink
fill of ``hdem_synth.synth_dem`` ("rough" and "srtm") at 4096^2, 16384^2 and 32768^2, made
on the device.  Per shape and mode (outlet, compact, pour points at one seed per 10^4
cells): warm-up calls, then the median of --reps calls of phase A (in-tile pointer
doubling), B (the forest of perimeter slots), C (labels written) and their sum, with the
basin and exit counts, the forest rounds that had work and a byte model.  The call has no
kernel id: its total is the sum of its three phases (the events are back to back on the
context's stream).  ``FlowAccumulation`` is timed on the same codes in the same process as
the yardstick.  For context, the NumPy pointer-doubling reference of tests/test_watersheds.py
is timed once at 4096^2 on the host.

    python tools/watershed_time.py [--sizes 4096,16384,32768] [--reps 5] [--warmup 2]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import PER, filled_codes, pour_seeds, tiles_of
from hydrodem_amd import backend


def modelled_bytes_per_cell(h, w, pour):
    """A reads the codes (and the seeds), writes 2 B per cell and 8 B per slot; B reads and
    writes the slot words about three times; C reads 2 B per cell and the slot words and
    writes the labels."""
    return 1 + 2 + 2 + 4 + (4 if pour else 0) + tiles_of(h, w) * PER * 8 * 5 / (h * w)


def time_mode(codes, out, seeds, compact, reps, warmup):
    rows = []
    for k in range(warmup + reps):
        _, _, st = backend.watershed_dev(codes, seeds, compact, out=out)
        if k >= warmup:
            rows.append(st)
    med = [float(np.median([r[k] for r in rows])) for k in ("ms_tile", "ms_forest", "ms_final")]
    return med, rows[-1]


def run(size, variant, reps, warmup):
    ctx = backend.context()
    codes = filled_codes(size, variant)
    out = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    cells = size * size
    seeds = pour_seeds(size)
    results = []
    try:
        ctx.profile(True)
        flow = []
        for k in range(warmup + reps):
            ctx.profile_reset()
            backend.flowacc_dev(codes, out)
            if k >= warmup:
                flow.append(ctx.profile_get(backend.K_FLOWACC)["ms"])
        for mode, s, compact in (("outlet", None, False), ("compact", None, True),
                                 ("pour", seeds, False)):
            med, st = time_mode(codes, out, s, compact, reps, warmup)
            total = sum(med)
            results.append({
                "size": size, "variant": variant, "mode": mode, "ms_A_tile": round(med[0], 4),
                "ms_B_forest": round(med[1], 4), "ms_C_final": round(med[2], 4),
                "ms_total": round(total, 4), "gcells_per_s": round(cells / total / 1e6, 2),
                "basins": int(st["basins"]), "exits": int(st["exits"]),
                "forest_rounds": int(st["forest_rounds"]),
                "bytes_per_cell_model": round(modelled_bytes_per_cell(size, size, s is not None),
                                              2),
                "flowacc_ms_same_codes": round(float(np.median(flow)), 4), "reps": reps})
    finally:
        ctx.profile(False)
        seeds.free()
        out.free()
        codes.free()
    return results


def host_reference(size=4096):
    from test_watersheds import labels_doubling
    with filled_codes(size) as codes:
        host_codes = codes.to_host()
    t = time.perf_counter()
    labels_doubling(host_codes)
    ms = (time.perf_counter() - t) * 1e3
    return {"size": size, "variant": "rough", "host_numpy_doubling_ms": round(ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,32768")
    ap.add_argument("--variants", default="rough,srtm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("watershed_time.py needs a GPU")
    for variant in a.variants.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            for row in run(size, variant, a.reps, a.warmup):
                print(json.dumps(row), flush=True)
    if not a.no_host:
        print(json.dumps(host_reference()), flush=True)


if __name__ == "__main__":
    main()
