"""HIP-event times of the proximity operator (``hdem_proximity_dev``), phase by phase (row pass
with the source bits and carries, column pass, final launch), with ``d2`` only and with all six
outputs, next to the host route the operator replaces, in the same process.

Input: ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2, its epsilon = 1e-3 sink fill,
D8 codes and flow accumulation, made on the device.  Source sets: the streams at ``acc >= 100``
and ``acc >= 1000`` (the accumulation with a threshold), one source in the corner (0, 0) and a
random mask of density 0.5; for the six outputs the sources go in as a label raster.  Per set:
--warmup calls, then every one of --reps calls is kept: the median and min ... max of each
phase, of their sum and of the wall clock of the binding's call.  ``corner_over_acc100`` is the
ratio of the medians of the single-corner-source case and the ``acc >= 100`` case: how much the
column pass still depends on its input.  ``copy_gbs`` is ``hdem_copy_rate_dev`` in the same
process, and ``fraction_of_copy`` the modelled traffic of the call over its time, over that
rate.  The host route, up to --host-size only, wall clock, once:
``scipy.ndimage.distance_transform_edt(return_indices=True)`` on the ``acc >= 100`` streams.

    python tools/proximity_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2]
                                   [--host-size 4096]
"""
import argparse
import json
import time

import numpy as np

import d8_inputs  # noqa: F401  (puts the repository root on sys.path)
import hdem_synth
from hydrodem_amd import backend, proximity

PHASES = ("ms_row", "ms_column", "ms_final")
ALL = tuple(n for n, _ in proximity.PROXIMITY_OUTPUTS)
SCRATCH_BYTES = 4 + 12 / 64             # per cell: see the header comment of hdem_proximity.hip


def modelled_bytes(source_bytes, want, with_dem):
    """Bytes per cell the call moves at least: sources once, the scratch written and read once
    each (the row pass's columns are read twice: by the column pass and by the final launch),
    the dem once plus a gather, the outputs once."""
    return (source_bytes + 2 * SCRATCH_BYTES + 2 + (8 if with_dem else 0)
            + (4 if "label" in want else 0) + 4 * len(want))


def timed(call, reps, warmup):
    rows, walls = [], []
    ctx = backend.context()
    for k in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        st = call()
        if k >= warmup:
            walls.append((time.perf_counter() - t0) * 1e3)
            rows.append(dict(st, ms_sum=sum(st[p] for p in PHASES), wall_ms=walls[-1]))
    out = {}
    for key in PHASES + ("ms_sum", "wall_ms"):
        values = [r[key] for r in rows]
        out[key] = {"median": round(float(np.median(values)), 4),
                    "min": round(float(min(values)), 4), "max": round(float(max(values)), 4),
                    "all": [round(float(v), 4) for v in values]}
    return out, rows[-1]


def host_route(mask):
    from scipy import ndimage
    t0 = time.perf_counter()
    ndimage.distance_transform_edt(~mask, return_indices=True)
    return round((time.perf_counter() - t0) * 1e3, 1)


def run(size, reps, warmup, host_size):
    ctx = backend.context()
    copy_gbs = backend.copy_rate(ctx)
    rng = np.random.default_rng(size)
    with backend.DeviceRaster.from_host(hdem_synth.synth_dem(size, size, variant="rough")) as dem:
        filled, codes, _ = backend.sinkfill_d8_dev(dem, eps=1e-3)
        with filled, codes:
            acc, _ = backend.flowacc_dev(codes)
        corner = np.zeros((size, size), np.uint8)
        corner[0, 0] = 1
        with acc, backend.DeviceRaster.from_host(corner) as corner_d, \
                backend.DeviceRaster.from_host(
                    (rng.random((size, size)) < 0.5).astype(np.uint8)) as random_d:
            del corner
            sets = {"acc100": (acc, 100), "acc1000": (acc, 1000), "corner": (corner_d, None),
                    "random0.5": (random_d, None)}
            medians = {}
            try:
                ctx.profile(True)
                for name, (sources, threshold) in sets.items():
                    for want in (("d2",), ALL):
                        src, thr = sources, threshold
                        labels = None
                        if "label" in want:       # the six outputs take the set as labels
                            host = sources.to_host()
                            host = (host >= threshold) if threshold else (host != 0)
                            labels = backend.DeviceRaster.from_host(host.astype(np.uint32))
                            src, thr = labels, None
                        try:
                            def call(s=src, t=thr, w=want):
                                outs, st = proximity.proximity_dev(
                                    s, t, w, dem if len(w) > 1 else None, 30.0, None, 8.0, 5.0, 1.0)
                                for raster in outs.values():
                                    raster.free()
                                return st
                            times, st = timed(call, reps, warmup)
                        finally:
                            if labels is not None:
                                labels.free()
                        per_cell = modelled_bytes(src.dtype.itemsize, want, len(want) > 1)
                        gbs = per_cell * size * size / (times["ms_sum"]["median"] * 1e6)
                        medians[(name, len(want))] = times["ms_sum"]["median"]
                        row = {"size": size, "sources": name, "outputs": len(want), "reps": reps,
                               "source_cells": int(st["sources"]), "times": times,
                               "modelled_bytes_per_cell": round(per_cell, 2),
                               "copy_gbs": round(copy_gbs, 1),
                               "fraction_of_copy": round(gbs / copy_gbs, 3)}
                        if name == "acc100" and len(want) == 1 and size <= host_size:
                            row["host_edt_ms"] = host_route(acc.to_host() >= 100)
                        print(json.dumps(row), flush=True)
            finally:
                ctx.profile(False)
            for outputs in (1, len(ALL)):
                print(json.dumps({"size": size, "outputs": outputs, "corner_over_acc100": round(
                    medians[("corner", outputs)] / medians[("acc100", outputs)], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-size", type=int, default=4096,
                    help="largest size at which the host route is timed")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("proximity_time.py needs a GPU")
    for size in (int(s) for s in a.sizes.split(",")):
        run(size, a.reps, a.warmup, a.host_size)


if __name__ == "__main__":
    main()
