"""HIP-event times of the zonal statistics (``hdem_zonal_count_u32_dev``,
``hdem_zonal_table_u32_dev``), step by step, with and without values, next to the specialised
depression table and to the host route the operator replaces, on the same inputs in the same
process.

Input: ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2, its epsilon = 1e-3 sink fill
and D8 codes, made on the device, and three label rasters of that fill: compact ``Watersheds``
labels, the ``row`` raster of the stream network at ``acc >= 100`` and compact ``Depressions``
labels.  Per label raster, with the DEM as values and without values: warm-up calls, then the
median of --reps calls of the count call and of the three steps of the table call (ranks, tile
pass, final) and the wall clock of the binding's whole call (count + table + download of the
columns).  On the depression labels also the wall clock of ``hdem_depression_table_f32_dev``
on device columns.  The host route, up to --host-size only, wall clock, once: download of the
labels and the values, ``np.unique(return_inverse=True)``, ``np.bincount`` and
``ndimage.minimum`` / ``maximum`` / ``sum``.

``--lib PATH`` times another build of the library, e.g. the comparison build of the tile pass
(``make FLAGS='... -DHDEM_ZONAL_PLAIN'`` into a directory of its own); the rows name it.

    python tools/zonal_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2] [--host-size 4096]
                               [--lib PATH]
"""
import argparse
import json
import os
import time

import numpy as np

import d8_inputs  # noqa: F401  (puts the repository root on sys.path)
import hdem_synth
from hydrodem_amd import backend, streamnet, streamorder, zonal

STEPS = ("ms_rank", "ms_tile", "ms_final")


def timed(call, reps, warmup):
    """Medians of the steps of ``call() -> stats`` (count call first), of its wall clock in ms,
    and the last stats."""
    rows, walls = [], []
    ctx = backend.context()
    for k in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        st = call()
        if k >= warmup:
            walls.append((time.perf_counter() - t0) * 1e3)
            rows.append(st)
    steps = {k: round(float(np.median([r[k] for r in rows])), 4) for k in ("ms_count",) + STEPS}
    steps["ms_sum"] = round(sum(steps.values()), 4)
    steps["wall_ms"] = round(float(np.median(walls)), 3)
    return steps, rows[-1]


def host_route(labels, values):
    """What a user does today: the rasters down, the cells grouped by id on the host."""
    from scipy import ndimage
    t0 = time.perf_counter()
    zones, v = labels.to_host(), values.to_host()
    t1 = time.perf_counter()
    flat = zones.ravel()
    on = flat > 0
    ids, inverse = np.unique(flat[on], return_inverse=True)
    t2 = time.perf_counter()
    np.bincount(inverse.ravel(), minlength=ids.size)
    t3 = time.perf_counter()
    ndimage.minimum(v, zones, ids)
    ndimage.maximum(v, zones, ids)
    ndimage.sum(v, zones, ids)
    t4 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 1)  # noqa: E731
    return {"host_download_ms": ms(t0, t1), "host_unique_ms": ms(t1, t2),
            "host_bincount_ms": ms(t2, t3), "host_ndimage_ms": ms(t3, t4),
            "host_ms": ms(t0, t4), "host_zones": int(ids.size)}


def depression_table_ms(dem, filled, labels, count, reps, warmup):
    ctx = backend.context()
    walls = []
    with backend.DeviceRaster.empty((max(count, 1), 24), np.uint8, ctx) as block:
        at = [block.ptr + count * k for k in (8, 12, 16, 20, 0)]
        for k in range(warmup + reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.check(ctx.lib.hdem_depression_table_f32_dev(
                ctx.handle, dem.ptr, filled.ptr, labels.ptr, *dem.shape, count, *at))
            if k >= warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(walls)), 3)


def run(size, reps, warmup, host_size, lib):
    ctx = backend.context()
    with backend.DeviceRaster.from_host(hdem_synth.synth_dem(size, size, variant="rough")) as dem:
        filled, codes, _ = backend.sinkfill_d8_dev(dem, eps=1e-3)
        with filled, codes:
            acc, _ = backend.flowacc_dev(codes)
            with acc:
                outs, order_stats = streamorder.streamorder_dev(codes, acc, 100,
                                                                ("order", "magnitude", "link"))
                _, row, _ = streamnet.streamlinks_dev(codes, outs["link"], order_stats["links"],
                                                      acc, 100, columns=("cells",), want_row=True)
                for raster in outs.values():
                    raster.free()
            basins, _, _ = backend.watershed_dev(codes, None, True)
            lakes, lake_stats = backend.depressions_dev(dem, filled, compact=True)
            rasters = {"watersheds": basins, "links": row, "depressions": lakes}
            try:
                ctx.profile(True)
                for name, labels in rasters.items():
                    out = {"size": size, "labels": name, "lib": lib or "default", "reps": reps}
                    full, st = timed(lambda z=labels: zonal.zonal_dev(z, dem)[1], reps, warmup)
                    lean, _ = timed(lambda z=labels: zonal.zonal_dev(z)[1], reps, warmup)
                    out.update({"zones": int(st["zones"]), "unzoned": int(st["unzoned"]),
                                "overflow_cells": int(st["overflow"]), "with_values": full,
                                "without_values": lean})
                    if name == "depressions":
                        ms = depression_table_ms(dem, filled, labels, lake_stats["depressions"],
                                                 reps, warmup)
                        # (that call leaves its columns on the device: the steps are its like)
                        out.update({"depression_table_call_ms": ms,
                                    "steps_to_depression_table": round(full["ms_sum"] / ms, 3),
                                    "wall_to_depression_table": round(full["wall_ms"] / ms, 3)})
                    if size <= host_size:
                        out.update(host_route(labels, dem))
                        out["host_over_device"] = round(out["host_ms"] / full["wall_ms"], 1)
                    print(json.dumps(out), flush=True)
            finally:
                ctx.profile(False)
                for raster in rasters.values():
                    raster.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-size", type=int, default=4096,
                    help="largest size at which the host route is timed")
    ap.add_argument("--lib", default=None, help="another build of libhydrodem_hip.so")
    a = ap.parse_args()
    if a.lib:
        os.environ["HYDRODEM_HIP_LIB"] = os.path.abspath(a.lib)
    if backend.device_count() < 1:
        raise SystemExit("zonal_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",")):
        run(size, a.reps, a.warmup, a.host_size, a.lib)


if __name__ == "__main__":
    main()
