"""HIP-event times of the stream network table (``hdem_streamlinks_u8_dev``), step by step, with
and without ``catchment``, next to the stream order, to ``Watersheds`` with the links as pour
points and to the host route the operator replaces, on the same inputs in the same process.

Input: the D8 codes of the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at
4096^2 and 16384^2, made on the device, their flow accumulation and, per stream set (every
cell, ``acc >= 100``, ``acc >= 1000``), the three rasters of the stream order.  Warm-up calls,
then the median of --reps calls of the four steps (ends and ranks, first stream cell, tile
pass, end pass) and their sum; the same for ``streamorder.streamorder_dev`` (all three
outputs) and ``backend.watershed_dev`` (the link raster as seeds) and the ratios of the sums.
The host route, up to --host-size only: download of the link, order and magnitude rasters
(9 B per cell), ``np.unique(links, return_inverse=True)`` and one ``np.bincount`` per count
column, wall clock, once.

    python tools/streamnet_time.py [--sizes 4096,16384] [--thresholds 0,100,1000]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import filled_dem_and_codes
from hydrodem_amd import backend, streamnet, streamorder

STEPS = ("ms_rank", "ms_trace", "ms_tile", "ms_final")
COUNTS = ("links", "stream_cells", "catchment_cells")
NO_CATCHMENT = tuple(n for n, _ in streamnet.STREAMNET_COLUMNS if n != "catchment")


def medians(call, phases, reps, warmup):
    """Per-phase medians of ``call() -> stats`` and the last stats dict."""
    for _ in range(warmup):
        call()
    rows = [call() for _ in range(reps)]
    return [float(np.median([r[k] for r in rows])) for k in phases], rows[-1]


def freed(outs, st):
    for raster in outs.values() if isinstance(outs, dict) else (outs,):
        raster.free()
    return st


def host_route(link, order, magnitude):
    """What a user does today: the rasters down, the cells grouped by link id on the host."""
    t0 = time.perf_counter()
    links, orders, magnitudes = link.to_host().ravel(), order.to_host(), magnitude.to_host()
    t1 = time.perf_counter()
    on = links > 0
    ids, inverse = np.unique(links[on], return_inverse=True)
    t2 = time.perf_counter()
    cells = np.bincount(inverse, minlength=ids.size)
    end = ids - 1
    table = cells, orders.ravel()[end], magnitudes.ravel()[end]
    t3 = time.perf_counter()
    return {"host_download_ms": round((t1 - t0) * 1e3, 1),
            "host_unique_ms": round((t2 - t1) * 1e3, 1),
            "host_bincount_ms": round((t3 - t2) * 1e3, 1),
            "host_links": int(table[0].size)}


def run(size, variant, thresholds, reps, warmup, host_size):
    ctx = backend.context()
    filled, codes = filled_dem_and_codes(size, variant)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    try:
        ctx.profile(True)
        backend.flowacc_dev(codes, acc)
        for threshold in thresholds:
            streams = (acc, threshold) if threshold else (None, None)
            wanted = ("order", "magnitude", "link")
            so, _ = medians(lambda: freed(*streamorder.streamorder_dev(codes, *streams, wanted)),
                            ("ms_nodes", "ms_walk", "ms_gather"), reps, warmup)
            outs, order_stats = streamorder.streamorder_dev(codes, *streams, wanted)
            count = order_stats["links"]

            def table(columns):
                _, raster, st = streamnet.streamlinks_dev(
                    codes, outs["link"], count, *streams, outs["order"], outs["magnitude"],
                    filled, 30.0, columns, True)
                return freed(raster, st)
            full, st = medians(lambda: table(None), STEPS, reps, warmup)
            lean, _ = medians(lambda: table(NO_CATCHMENT), STEPS, reps, warmup)
            ws, _ = medians(lambda: (lambda r: freed(r[0], r[2]))(
                backend.watershed_dev(codes, outs["link"])),
                ("ms_tile", "ms_forest", "ms_final"), reps, warmup)
            row = {"size": size, "variant": variant, "threshold": threshold or None}
            row.update({k: int(st[k]) for k in COUNTS})
            row.update({k: round(v, 4) for k, v in zip(STEPS, full)})
            row.update({"ms_sum": round(sum(full), 4),
                        "no_catchment": {k: round(v, 4) for k, v in zip(STEPS, lean)},
                        "no_catchment_ms_sum": round(sum(lean), 4),
                        "streamorder_ms": round(sum(so), 4), "watersheds_ms": round(sum(ws), 4),
                        "ratio_to_streamorder": round(sum(full) / sum(so), 3),
                        "no_catchment_ratio_to_streamorder": round(sum(lean) / sum(so), 3),
                        "ratio_to_watersheds": round(sum(full) / sum(ws), 3), "reps": reps})
            if size <= host_size:
                row.update(host_route(outs["link"], outs["order"], outs["magnitude"]))
            print(json.dumps(row), flush=True)
            freed(outs, None)
    finally:
        ctx.profile(False)
        acc.free()
        codes.free()
        filled.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variants", default="rough")
    ap.add_argument("--thresholds", default="100,1000,0", help="0: every cell is a stream cell")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-size", type=int, default=4096,
                    help="largest size at which the host route is timed")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("streamnet_time.py needs a GPU")
    for variant in a.variants.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            run(size, variant, [int(t) for t in a.thresholds.split(",")], a.reps, a.warmup,
                a.host_size)


if __name__ == "__main__":
    main()
