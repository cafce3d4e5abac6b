"""HIP-event times of the stream order (``hdem_streamorder_u8_dev``), phase by phase, next to
D8 flow accumulation and the flow distance to the same streams on the same codes in the same
process.

Input: the D8 codes of the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough") at
4096^2 and 16384^2, made on the device, and their flow accumulation.  Per shape and stream
set (every cell, ``acc >= 100``, ``acc >= 1000``): warm-up calls, then the median of --reps
calls of the three phases (node pass + first stop, walk over the link graph, gather) and their
sum, with the stream cells, heads, junctions, links, greatest order and the longest walk; then
the same for ``backend.flowacc_dev`` and ``backend.flowtrace_dev`` (distance to those
streams) and the ratios of the sums.

    python tools/streamorder_time.py [--sizes 4096,16384] [--thresholds 0,100,1000]
"""
import argparse
import json

import numpy as np

from d8_inputs import filled_codes
from hydrodem_amd import backend, streamorder

COUNTS = ("stream_cells", "heads", "junctions", "links", "max_order", "max_hops")


def medians(call, phases, reps, warmup):
    """Per-phase medians of ``call() -> stats`` and the last stats dict."""
    for _ in range(warmup):
        call()
    rows = [call() for _ in range(reps)]
    return [float(np.median([r[k] for r in rows])) for k in phases], rows[-1]


def freed(result):
    outs, st = result
    for raster in outs.values():
        raster.free()
    return st


def run(size, variant, thresholds, want, reps, warmup):
    ctx = backend.context()
    codes = filled_codes(size, variant)
    acc = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    d8_phases = ("ms_tile", "ms_forest", "ms_final")
    try:
        ctx.profile(True)
        fa, _ = medians(lambda: backend.flowacc_dev(codes, acc)[1], d8_phases, reps, warmup)
        for threshold in thresholds:
            streams = (acc, threshold) if threshold else (None, None)
            so, st = medians(lambda: freed(streamorder.streamorder_dev(codes, *streams, want)),
                             ("ms_nodes", "ms_walk", "ms_gather"), reps, warmup)
            fd, _ = medians(lambda: freed(backend.flowtrace_dev(codes, *streams)), d8_phases,
                            reps, warmup)
            row = {"size": size, "variant": variant, "threshold": threshold or None,
                   "outputs": list(want), "ms_nodes": round(so[0], 4), "ms_walk": round(so[1], 4),
                   "ms_gather": round(so[2], 4), "ms_sum": round(sum(so), 4)}
            row.update({k: int(st[k]) for k in COUNTS})
            row.update({"flowacc_ms": round(sum(fa), 4), "flowdistance_ms": round(sum(fd), 4),
                        "ratio_to_flowacc": round(sum(so) / sum(fa), 3),
                        "ratio_to_flowdistance": round(sum(so) / sum(fd), 3), "reps": reps})
            print(json.dumps(row), flush=True)
    finally:
        ctx.profile(False)
        acc.free()
        codes.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--variants", default="rough")
    ap.add_argument("--thresholds", default="0,100,1000", help="0: every cell is a stream cell")
    ap.add_argument("--outputs", default="order")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("streamorder_time.py needs a GPU")
    for variant in a.variants.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            run(size, variant, [int(t) for t in a.thresholds.split(",")],
                tuple(a.outputs.split(",")), a.reps, a.warmup)


if __name__ == "__main__":
    main()
