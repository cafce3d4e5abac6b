"""
bench.py's plain run: the headline line only, --steps timed steps, and --dump-outputs
writes what the last step computed (here the whole raster: it is below the sampling size).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle import c_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(built, tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--size", "1024", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == "Mcells/s sink-fill+D8 on 1024^2 float32 DEM"
    assert rec["unit"] == "Mcells/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(1024 * 1024 / rec["ms_per_step"] / 1e3, rel=1e-9)
    # the extras are --full's
    for key in ("roofline", "kernels", "filters", "config2", "cpu_baseline"):
        assert key not in rec
    z = oracle.synth_dem(1024, 1024)
    want = c_oracle.sinkfill_pflood(z)
    filled, codes = np.load(dump / "filled.npy"), np.load(dump / "d8.npy")
    assert filled.dtype == np.float32 and codes.dtype == np.float32
    assert np.array_equal(filled, want)
    assert np.array_equal(codes, c_oracle.d8(want).astype(np.float32))
