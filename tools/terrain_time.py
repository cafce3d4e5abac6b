"""HIP-event times of the terrain-attribute launch (``hdem_terrain_f32_dev``) for several sets
of outputs, next to the two radius-1 kernels of the same shape (``d8_kernel``,
``boxmean3_kernel<float>``), to the measured copy rate and to the host route the operator
replaces, on the same raster in the same process.

Input: ``hdem_synth.synth_dem`` ("rough") at 4096^2 and 16384^2; for the wetness index its
epsilon = 1e-3 sink fill, D8 codes and accumulation, made on the device.  Per configuration:
warm-up calls, then the median of --reps calls of the launch's own time (``ms_total``, HIP
events), Gcells/s, the modelled HBM bytes per cell (4 B per raster touched, 1 B for the codes,
the DEM x 1.07 for the halo) and that traffic as a fraction of the 8 TB/s peak and of the copy
rate ``hdem_copy_rate_dev`` reaches in this run.  ``DemToWetness`` end to end: wall clock of its
stages, each ended by a synchronise.  The host route, up to --host-size only, wall clock, once:
download of the DEM (and the accumulation), ``np.gradient`` / ``np.arctan`` / ``np.arctan2`` /
``np.log``.

    python tools/terrain_time.py [--sizes 4096,16384] [--reps 5] [--warmup 2] [--host-size 4096]
"""
import argparse
import json
import time

import numpy as np

import d8_inputs  # noqa: F401  (puts the repository root on sys.path)
import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, terrain

PEAK_GBS = 8000.0
CONFIGS = (("tangent", ("tangent",), "horn"),
           ("degrees+aspect", ("degrees", "aspect"), "horn"),
           ("all eight", terrain.TERRAIN_OUTPUTS, "horn"),
           ("twi", ("twi",), "horn"),
           ("twi along d8", ("twi",), "d8"))


def bytes_per_cell(want, slope):
    reads = 4 * 1.07
    if "twi" in want or "spi" in want:
        reads += 4
    if "d8_slope" in want or (slope == "d8" and ("twi" in want or "spi" in want)):
        reads += 1
    return reads + 4 * len(want)


def rates(ms, cells, per_cell, copy_gbs):
    gbs = cells * per_cell / ms / 1e6
    return {"ms": round(ms, 4), "gcells_s": round(cells / ms / 1e6, 2),
            "bytes_per_cell": round(per_cell, 2), "model_gb_s": round(gbs, 1),
            "of_peak": round(gbs / PEAK_GBS, 3), "of_copy_rate": round(gbs / copy_gbs, 3)}


def launch_ms(call, reps, warmup):
    """Median ``ms_total`` of ``call() -> (outs, stats)``; the outputs are freed."""
    seen = []
    for k in range(warmup + reps):
        outs, stats = call()
        for raster in outs.values():
            raster.free()
        if k >= warmup:
            seen.append(stats["ms_total"])
    return float(np.median(seen))


def kernel_ms(ctx, kernel_id, call, reps, warmup):
    """Median time of the launches ``call()`` makes under ``kernel_id`` (the context's timers)."""
    seen = []
    for k in range(warmup + reps):
        was = ctx.profile_get(kernel_id)["ms"]
        call().free()
        if k >= warmup:
            seen.append(ctx.profile_get(kernel_id)["ms"] - was)
    return float(np.median(seen))


def host_route(dem, acc, cell):
    t0 = time.perf_counter()
    z, a = dem.to_host(), acc.to_host()
    t1 = time.perf_counter()
    gy, gx = np.gradient(z, cell)
    tangent = np.sqrt(gx * gx + gy * gy)
    degrees = np.degrees(np.arctan(tangent))
    aspect = np.degrees(np.arctan2(-gx, gy))
    aspect[aspect < 0] += 360
    t2 = time.perf_counter()
    with np.errstate(divide="ignore"):
        np.log(a.astype(np.float32) * np.float32(cell) / np.maximum(tangent, np.float32(1e-3)))
    t3 = time.perf_counter()
    del degrees
    ms = lambda p, q: round((q - p) * 1e3, 1)  # noqa: E731
    return {"host_download_ms": ms(t0, t1), "host_slope_aspect_ms": ms(t1, t2),
            "host_twi_ms": ms(t2, t3), "host_ms": ms(t0, t3)}


def chain_stages(dem, cell):
    """Wall clock of the stages of ``DemToWetness`` (each ended by a synchronise), and of the
    chain as the class runs it."""
    ctx = dem.ctx
    ms = {}

    def stage(name, call):
        ctx.synchronize()
        t0 = time.perf_counter()
        result = call()
        ctx.synchronize()
        ms[name] = round((time.perf_counter() - t0) * 1e3, 2)
        return result
    filled, codes, _ = stage("fill_d8_ms", lambda: backend.sinkfill_d8_dev(dem, eps=1e-3))
    with filled, codes:
        acc, _ = stage("flowacc_ms", lambda: backend.flowacc_dev(codes))
        with acc:
            outs, _ = stage("wetness_ms", lambda: terrain.terrain_dev(
                filled, "twi", cell, codes=codes, accumulation=acc))
            outs["twi"].free()
    stage("chain_ms", lambda: hd.DemToWetness(cellsize=cell).apply_device(dem)).free()
    return ms


def run(size, reps, warmup, host_size, copy_gbs):
    ctx = backend.context()
    cell, cells = 30.0, size * size
    with backend.DeviceRaster.from_host(hdem_synth.synth_dem(size, size, variant="rough")) as dem:
        filled, codes, _ = backend.sinkfill_d8_dev(dem, eps=1e-3)
        with filled, codes:
            acc, _ = backend.flowacc_dev(codes)
            with acc:
                ctx.profile(True)
                try:
                    for name, want, slope in CONFIGS:
                        ms = launch_ms(lambda w=want, s=slope: terrain.terrain_dev(
                            dem, w, cell, codes=codes, accumulation=acc, slope=s), reps, warmup)
                        print(json.dumps({"size": size, "config": name, "reps": reps,
                                          **rates(ms, cells, bytes_per_cell(want, slope),
                                                  copy_gbs)}), flush=True)
                    for name, kernel_id, call, per_cell in (
                            ("d8_kernel", backend.K_D8, lambda: backend.d8_dev(dem), 4 * 1.07 + 1),
                            ("boxmean3_kernel<float>", backend.K_BOXMEAN,
                             lambda: backend.boxmean3_dev(dem, False), 4 * 1.07 + 4)):
                        ms = kernel_ms(ctx, kernel_id, call, reps, warmup)
                        print(json.dumps({"size": size, "config": name, "reps": reps,
                                          **rates(ms, cells, per_cell, copy_gbs)}), flush=True)
                finally:
                    ctx.profile(False)
                if size <= host_size:
                    print(json.dumps({"size": size, "config": "host route",
                                      **host_route(dem, acc, cell)}), flush=True)
        print(json.dumps({"size": size, "config": "DemToWetness", **chain_stages(dem, cell)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-size", type=int, default=4096,
                    help="largest size at which the host route is timed")
    a = ap.parse_args()
    if backend.device_count() < 1:
        raise SystemExit("terrain_time.py needs a GPU")
    ctx = backend.context()
    copy_gbs = backend.copy_rate(ctx)
    ctx.profile(False)
    print(json.dumps({"copy_rate_gb_s": round(copy_gbs, 1)}), flush=True)
    for size in (int(s) for s in a.sizes.split(",")):
        run(size, a.reps, a.warmup, a.host_size, copy_gbs)


if __name__ == "__main__":
    main()
