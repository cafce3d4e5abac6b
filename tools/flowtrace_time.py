"""HIP-event times of the D8 flow trace (``hdem_flowtrace_u8_dev``), phase by phase.

Input: the rasters of ``tools/watershed_time.py`` -- the D8 codes of the epsilon = 1e-3 sink
fill of ``hdem_synth.synth_dem`` at 4096^2, 16384^2 and 32768^2, made on the device, with
the device ``FlowAccumulation`` of those codes as the stream raster.  Per shape and mode
(distance to the outlet; distance to the streams ``acc >= threshold``; HAND with all five
outputs): warm-up calls, then the median of --reps calls of phase A (in-tile pointer
doubling with counts), B (the forest of perimeter slots) and C (outputs written) and their
sum, with the stop, unreached and exit counts, the forest rounds that had work and a byte
model.  The call has no kernel id: its total is the sum of its three phases (the events are
back to back on the context's stream).  ``Watersheds`` in pour-point mode (one seed per 10^4
cells) is timed on the same codes in the same process as the yardstick: the same scheme
without the payload.  The device copy rate is measured in the same process.

``--alternative SIZE`` times what the HAND call replaces, wall clock on host arrays: seeds
``1 + flat index`` on the stream cells built with NumPy, ``Watersheds(pour_points=seeds)``,
and the NumPy gather ``z - z.ravel()[label - 1]``; next to it ``HeightAboveDrainage.apply``
on the same host arrays.

    python tools/flowtrace_time.py [--sizes 4096,16384,32768] [--reps 5] [--warmup 2]
                                   [--alternative 16384]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import PER, filled_dem_and_codes, pour_seeds, tiles_of
import hydrodem_amd as hd
from hydrodem_amd import backend

THRESHOLDS = {4096: 1000}            # 10 000 elsewhere
ALL = ("stop", "ncard", "ndiag", "distance", "hand")


def modelled_bytes_per_cell(h, w, streams, outputs, hand, launches):
    """(A, B, C) bytes per cell.  A reads the codes (and the 4-byte stream raster) and writes
    6 B per cell and a 16-byte node per slot; each of B's launches with work reads and writes
    every node (the jumps on top hit the cache or do not happen); C reads 6 B per cell and
    the nodes and writes 4 B per output, and HAND reads the cell's own elevation (the
    gathered one is counted as a cache hit: neighbours share their stream cell)."""
    slots = tiles_of(h, w) * PER * 16 / (h * w)
    return (1 + (4 if streams else 0) + 6 + slots, 2 * slots * launches, 6 + slots + 4 * outputs
            + (4 if hand else 0))


def median_phases(rows):
    return [float(np.median([r[k] for r in rows])) for k in ("ms_tile", "ms_forest", "ms_final")]


def run(size, reps, warmup, copy_gbs):
    ctx = backend.context()
    threshold = THRESHOLDS.get(size, 10000)
    filled, codes = filled_dem_and_codes(size)
    acc, _ = backend.flowacc_dev(codes)
    cut = {False: None, True: threshold}
    cells = size * size
    seeds = pour_seeds(size)
    results = []
    try:
        ctx.profile(True)
        rows = []
        with backend.DeviceRaster.empty(codes.shape, np.uint32, ctx) as labels:
            for k in range(warmup + reps):
                _, _, st = backend.watershed_dev(codes, seeds, False, out=labels)
                if k >= warmup:
                    rows.append(st)
        pour = median_phases(rows)
        for mode, streams, dem, want in (("outlet_distance", None, None, ("distance",)),
                                         ("stream_distance", acc, None, ("distance",)),
                                         ("hand_all_outputs", acc, filled, ALL)):
            rows = []
            for k in range(warmup + reps):
                outs, st = backend.flowtrace_dev(codes, streams, cut[streams is not None],
                                                 dem, 30.0, want)
                for raster in outs.values():
                    raster.free()
                if k >= warmup:
                    rows.append(st)
            med, st = median_phases(rows), rows[-1]
            total = sum(med)
            model = modelled_bytes_per_cell(size, size, streams is not None, len(want),
                                            "hand" in want, int(st["forest_rounds"]))
            results.append({
                "size": size, "mode": mode, "threshold": cut[streams is not None],
                "ms_A_tile": round(med[0], 4), "ms_B_forest": round(med[1], 4),
                "ms_C_final": round(med[2], 4), "ms_total": round(total, 4),
                "gcells_per_s": round(cells / total / 1e6, 2),
                "stops": int(st["stops"]), "unreached": int(st["unreached"]),
                "exits": int(st["exits"]), "forest_rounds": int(st["forest_rounds"]),
                "bytes_per_cell_model_ABC": [round(b, 2) for b in model],
                "gbs_model_ABC": [round(b * cells / ms / 1e6, 1) for b, ms in zip(model, med)],
                "copy_rate_gbs": round(copy_gbs, 1),
                "watershed_pour_ms_ABC": [round(v, 4) for v in pour],
                "watershed_pour_ms_total": round(sum(pour), 4), "reps": reps})
    finally:
        ctx.profile(False)
        for raster in (seeds, acc, filled, codes):
            raster.free()
    return results


def alternative(size):
    """Wall time of the host route to HAND through ``Watersheds`` and of the new operator."""
    threshold = THRESHOLDS.get(size, 10000)
    filled, codes = filled_dem_and_codes(size)
    with filled, codes:
        acc_dev, _ = backend.flowacc_dev(codes)
        with acc_dev:
            z, d8, acc = filled.to_host(), codes.to_host(), acc_dev.to_host()
    hd.Watersheds().apply(d8[:256, :256].copy())         # the library and the context are up
    t0 = time.perf_counter()
    seeds = np.where(acc >= threshold,
                     np.arange(1, acc.size + 1, dtype=np.uint32).reshape(acc.shape),
                     np.uint32(0))
    t1 = time.perf_counter()
    label = hd.Watersheds(pour_points=seeds).apply(d8)
    t2 = time.perf_counter()
    hand = z - z.ravel()[np.maximum(label.astype(np.int64) - 1, 0)]
    hand[label == 0] = np.nan
    t3 = time.perf_counter()
    op = hd.HeightAboveDrainage(dem=z, streams=acc, threshold=threshold)
    op.apply(d8)                                         # warm: page-locked result blocks
    t4 = time.perf_counter()
    got = op.apply(d8)
    t5 = time.perf_counter()
    return {"size": size, "threshold": threshold,
            "host_seeds_s": round(t1 - t0, 3), "watersheds_apply_s": round(t2 - t1, 3),
            "numpy_gather_s": round(t3 - t2, 3), "alternative_total_s": round(t3 - t0, 3),
            "height_above_drainage_apply_s": round(t5 - t4, 3),
            "identical": bool(np.array_equal(got, hand, equal_nan=True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternative", type=int, default=0)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("flowtrace_time.py needs a GPU")
    copy_gbs = backend.copy_rate()
    for size in (int(s) for s in a.sizes.split(",") if s):
        for row in run(size, a.reps, a.warmup, copy_gbs):
            print(json.dumps(row), flush=True)
    if a.alternative:
        print(json.dumps(alternative(a.alternative)), flush=True)


if __name__ == "__main__":
    main()
