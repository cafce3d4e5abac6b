"""What ``flowacc_time.py``, ``watershed_time.py`` and ``flowtrace_time.py`` share: the tile
geometry of the D8 operators for their byte models, and their inputs, made on the device.
Importing it puts the repository root and ``tests/`` on ``sys.path``."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hdem_synth  # noqa: E402
from hydrodem_amd import backend  # noqa: E402

TILE, PER = 64, 252


def tiles_of(h, w):
    return -(-h // TILE) * -(-w // TILE)


def filled_dem_and_codes(size, variant="rough"):
    """The epsilon = 1e-3 sink fill of ``hdem_synth.synth_dem`` at size^2 and its D8 codes,
    both device rasters that the caller frees."""
    z = hdem_synth.synth_dem(size, size, variant=variant)
    with backend.DeviceRaster.from_host(z) as dz:
        del z
        filled, codes, _ = backend.sinkfill_d8_dev(dz, eps=1e-3)
    return filled, codes


def filled_codes(size, variant="rough"):
    filled, codes = filled_dem_and_codes(size, variant)
    filled.free()
    return codes


def pour_seeds(size):
    """A device raster of pour points: one seed per 10^4 cells, labels 1, 2, ..."""
    cells = size * size
    rng = np.random.default_rng(size)
    host_seeds = np.zeros(cells, np.uint32)
    where = rng.choice(cells, size=cells // 10000, replace=False)
    host_seeds[where] = np.arange(1, where.size + 1, dtype=np.uint32)
    return backend.DeviceRaster.from_host(host_seeds.reshape(size, size), dtype=np.uint32)
