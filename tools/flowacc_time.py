"""HIP-event times of D8 flow accumulation (``hdem_flowacc_u8_dev``), phase by phase.

Input: the D8 codes of the epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` ("rough"
and "srtm") at 4096^2, 16384^2 and 32768^2, made on the device.  Per shape: warm-up calls,
then the median of --reps calls of phase A (in-tile pass), B (exit forest), C (in-tile
pass again, writes acc) and the whole call (HDEM_K_FLOWACC), with the exit-forest size,
the longest forest walk and a byte model.  For context, the NumPy Kahn reference of
tests/test_flowacc.py is timed once at 4096^2 on the host.

    python tools/flowacc_time.py [--sizes 4096,16384,32768] [--reps 5] [--warmup 2]
"""
import argparse
import json
import time

import numpy as np

from d8_inputs import TILE, PER, filled_codes, tiles_of
from hydrodem_amd import backend


def modelled_bytes_per_cell(h, w):
    """Codes read twice with their halo, acc written once, and the perimeter slots
    (A writes 20 B, B1 ~16, B2 ~12, C ~16 per slot: 64 B)."""
    halo = (TILE + 2) ** 2 / TILE ** 2
    return 2 * halo + 4 + tiles_of(h, w) * PER * 64 / (h * w)


def run(size, variant, reps, warmup):
    ctx = backend.context()
    codes = filled_codes(size, variant)
    out = backend.DeviceRaster.empty(codes.shape, np.uint32, ctx)
    rows = []
    try:
        ctx.profile(True)
        for _ in range(warmup):
            backend.flowacc_dev(codes, out)
        for _ in range(reps):
            ctx.profile_reset()
            _, st = backend.flowacc_dev(codes, out)
            total = ctx.profile_get(backend.K_FLOWACC)["ms"]
            rows.append((st["ms_tile"], st["ms_forest"], st["ms_final"], total, st))
    finally:
        ctx.profile(False)
        out.free()
        codes.free()
    med = [float(np.median([r[k] for r in rows])) for k in range(4)]
    st = rows[-1][4]
    cells = size * size
    return {"size": size, "variant": variant, "ms_A_tile": round(med[0], 4),
            "ms_B_forest": round(med[1], 4), "ms_C_final": round(med[2], 4),
            "ms_total": round(med[3], 4), "gcells_per_s": round(cells / med[3] / 1e6, 2),
            "exits": int(st["exits"]), "max_hops": int(st["max_hops"]),
            "bytes_per_cell_model": round(modelled_bytes_per_cell(size, size), 2),
            "reps": reps}


def host_reference(size=4096):
    from test_flowacc import acc_kahn
    with filled_codes(size) as codes:
        host_codes = codes.to_host()
    t = time.perf_counter()
    acc_kahn(host_codes)
    ms = (time.perf_counter() - t) * 1e3
    return {"size": size, "variant": "rough", "host_numpy_kahn_ms": round(ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,32768")
    ap.add_argument("--variants", default="rough,srtm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("flowacc_time.py needs a GPU")
    for variant in a.variants.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            print(json.dumps(run(size, variant, a.reps, a.warmup)), flush=True)
    if not a.no_host:
        print(json.dumps(host_reference()), flush=True)


if __name__ == "__main__":
    main()
