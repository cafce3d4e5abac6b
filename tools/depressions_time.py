"""HIP-event times of the depression labelling (``hdem_depressions_f32_dev``), phase by phase,
of the depression table, and the host route they replace.

Input: ``hdem_synth.synth_dem`` (both variants) at 4096^2 and 16384^2 and its epsilon = 0
sink fill, made on the device.  Per shape and variant: warm-up calls, then the median of
--reps calls of the three phases of the compact labelling (tile: components inside a tile;
seam: unions across the seams; final: roots flattened, labels written, numbered) and their
sum, the same for ``labels="first"``, and the wall clock of the table: of the binding's call
(block allocated, K rows downloaded) and of the C call alone on device columns.
The streaming phases are quoted against the measured copy rate (``hdem_copy_rate_dev``) for
the bytes they must move: tile reads dem and filled and writes the labels (12 B per cell),
final reads and writes the labels twice in compact mode (16 B per cell), the table reads the
three rasters (12 B per cell).  ``Watersheds`` (outlet mode) on the D8 codes of the same fill
is the sibling to compare with.  ``--host`` adds ``scipy.ndimage.label`` plus the five
``ndimage`` statistics on the downloaded arrays, in the same run.  ``--spiral`` times the
tile phase on the 2 047-cell spiral corridor, the shape that makes a naive propagation slow.

    python tools/depressions_time.py [--sizes 4096,16384] [--variants rough,srtm] [--reps 5]
                                     [--warmup 2] [--host] [--spiral]
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


def phases_of(dem, filled, out, compact, reps, warmup):
    rows = []
    for k in range(warmup + reps):
        _, st = backend.depressions_dev(dem, filled, compact=compact, out=out)
        if k >= warmup:
            rows.append(st)
    return [median_of(rows, k) for k in ("ms_tile", "ms_seam", "ms_final")], rows[-1]


def host_route(z, w):
    """``ndimage.label`` and the five statistics of the table, seconds each."""
    from scipy import ndimage
    t0 = time.perf_counter()
    raised = w > z
    lab, count = ndimage.label(raised, structure=np.ones((3, 3)))
    t1 = time.perf_counter()
    index = np.arange(1, count + 1)
    depth = w - z
    flat = np.arange(z.size, dtype=np.int64).reshape(z.shape)
    ndimage.minimum(flat, lab, index)
    ndimage.sum(raised, lab, index)
    ndimage.minimum(w, lab, index)
    ndimage.maximum(depth, lab, index)
    ndimage.sum(depth, lab, index)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, count


def run(size, variant, reps, warmup, host, copy_gbs):
    ctx = backend.context()
    z = hdem_synth.synth_dem(size, size, variant=variant)
    dz = backend.DeviceRaster.from_host(z)
    filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=0.0)
    out = backend.DeviceRaster.empty(dz.shape, np.uint32, ctx)
    try:
        ctx.profile(True)
        compact, st = phases_of(dz, filled, out, True, reps, warmup)
        first, _ = phases_of(dz, filled, out, False, reps, warmup)
        sheds = []
        for k in range(warmup + reps):
            _, _, ws = backend.watershed_dev(codes, out=out)
            if k >= warmup:
                sheds.append(ws["ms_tile"] + ws["ms_forest"] + ws["ms_final"])
        ctx.profile(False)
        backend.depressions_dev(dz, filled, compact=True, out=out)
        count = int(st["depressions"])
        table_ms = []
        for k in range(warmup + reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            table = backend.depression_table_dev(dz, filled, out, count)
            if k >= warmup:
                table_ms.append((time.perf_counter() - t0) * 1e3)
        # ... and of the C call alone, on device columns that stay: it ends in its own synchronise
        call_ms = []
        with backend.DeviceRaster.empty((count, 24), np.uint8, ctx) as block:
            at = [block.ptr + count * k for k in (8, 12, 16, 20, 0)]
            for k in range(warmup + reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.check(ctx.lib.hdem_depression_table_f32_dev(
                    ctx.handle, dz.ptr, filled.ptr, out.ptr, size, size, count, *at))
                if k >= warmup:
                    call_ms.append((time.perf_counter() - t0) * 1e3)
        cells = size * size
        roof = lambda nbytes, ms: round(nbytes * cells / (ms * 1e6) / copy_gbs, 3)  # noqa: E731
        row = {"size": size, "variant": variant, "reps": reps,
               "ms_tile": round(compact[0], 4), "ms_seam": round(compact[1], 4),
               "ms_final": round(compact[2], 4), "ms_total": round(sum(compact), 4),
               "first_ms_final": round(first[2], 4), "first_ms_total": round(sum(first), 4),
               "table_wall_ms": round(float(np.median(table_ms)), 4),
               "table_call_ms": round(float(np.median(call_ms)), 4),
               "watersheds_ms": round(float(np.median(sheds)), 4),
               "tile_of_copy_rate": roof(12, compact[0]),
               "final_of_copy_rate": roof(16, compact[2]),
               "first_final_of_copy_rate": roof(8, first[2]),
               "table_of_copy_rate": roof(12, float(np.median(call_ms))),
               "copy_gbs": round(copy_gbs, 1), "tiles": tiles_of(size, size),
               "depressions": count, "raised_share": round(st["raised_cells"] / cells, 4),
               "tile_components": int(st["tile_components"]),
               "single_cell": int((table["area"] == 1).sum()),
               "largest_cells": int(table["area"].max()) if count else 0}
        if host:
            label_s, stats_s, host_count = host_route(z, filled.to_host())
            assert host_count == count
            row.update({"host_label_s": round(label_s, 3), "host_statistics_s": round(stats_s, 3)})
        return row
    finally:
        ctx.profile(False)
        for raster in (dz, filled, codes, out):
            raster.free()


def spiral(reps, warmup):
    """The tile phase on a 2 047-cell spiral corridor inside one tile."""
    def walk(n):                     # ring by ring inwards: consecutive cells are neighbours
        cells, top, left, bottom, right = [], 0, 0, n - 1, n - 1
        while top <= bottom and left <= right:
            cells += [(top, x) for x in range(left, right + 1)]
            cells += [(y, right) for y in range(top + 1, bottom + 1)]
            if top < bottom:
                cells += [(bottom, x) for x in range(right - 1, left - 1, -1)]
            if left < right:
                cells += [(y, left) for y in range(bottom - 1, top, -1)]
            top, left, bottom, right = top + 1, left + 1, bottom - 1, right - 1
        return cells
    coarse = walk(32)
    mask = np.zeros((66, 66), np.float32)
    for (ay, ax), (by, bx) in zip(coarse[:-1], coarse[1:]):
        mask[1 + 2 * ay, 1 + 2 * ax] = mask[1 + ay + by, 1 + ax + bx] = 1
    mask[1 + 2 * coarse[-1][0], 1 + 2 * coarse[-1][1]] = 1
    assert int(mask.sum()) == 2047
    ctx = backend.context()
    with backend.DeviceRaster.from_host(np.zeros_like(mask)) as dem, \
            backend.DeviceRaster.from_host(mask) as filled, \
            backend.DeviceRaster.empty(mask.shape, np.uint32, ctx) as out:
        ctx.profile(True)
        try:
            phases, st = phases_of(dem, filled, out, True, reps, warmup)
        finally:
            ctx.profile(False)
        blank = np.zeros_like(mask)
        blank[0:64, 0:64] = 1
        with backend.DeviceRaster.from_host(blank) as full:
            ctx.profile(True)
            try:
                plain, _ = phases_of(dem, full, out, True, reps, warmup)
            finally:
                ctx.profile(False)
    return {"spiral_cells": 2047, "depressions": int(st["depressions"]),
            "spiral_ms_tile": round(phases[0], 4), "full_square_ms_tile": round(plain[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variants", default="rough,srtm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--spiral", action="store_true")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("depressions_time.py needs a GPU")
    if a.spiral:
        print(json.dumps(spiral(a.reps, a.warmup)), flush=True)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    if not sizes:
        return
    try:
        copy_gbs = backend.copy_rate()
    finally:
        backend.context().profile(False)
    for size in sizes:
        for variant in (v for v in a.variants.split(",") if v):
            print(json.dumps(run(size, variant, a.reps, a.warmup, a.host, copy_gbs)),
                  flush=True)


if __name__ == "__main__":
    main()
