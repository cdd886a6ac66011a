"""Randomised differential soak of OccupancyMap::calcRange on the device where its rays run long (soak_rays.py draws
maps below 400 cells a side, which every ray leaves after a few hundred steps): sparse open maps of 1000 ... 2500 cells
a side, the two sides drawn independently, 1500 rays per map with max ranges of 600 ... 3000 cells -- the integer form
of the walk up to its last ray length and the fp64 form beyond -- against the oracle's cell-by-cell Bresenham walk.
Exact.
usage: python tools/soak_long_rays.py [maps] [seed]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import badger_amcl_amd as bpf
from oracle import pyoracle as orc
import long_rays as lr

def run(maps=6, seed=1, e=None, quiet=False):
    """Returns the number of mismatching cases."""
    rng = np.random.default_rng(seed)
    own = e is None
    if own:
        e = bpf.Engine(0)
    t0 = time.time()
    bad = 0
    rays = 0
    far = 0
    for case in range(maps):
        sx, sy = int(rng.integers(1000, 2501)), int(rng.integers(1000, 2501))
        res = float(rng.choice([0.05, 0.1]))
        cells = lr.open_map(sx, sy, int(rng.integers(1 << 30)))
        if rng.random() < 0.3:     # no border walls: the rays leave the map instead
            cells[0, :] = cells[-1, :] = -1
            cells[:, 0] = cells[:, -1] = -1
        origin = (float(np.float32(rng.uniform(-50, 50))), float(np.float32(rng.uniform(-50, 50))))
        om = orc.OccupancyMap(cells, res, origin)
        m = bpf.OccupancyMap(e, res)
        m.setCells(cells)
        m.setOrigin(origin)
        n = 1500
        ox, oy, oa, _ = lr.fan(om, n, int(rng.integers(1 << 30)))
        k = rng.uniform(600.0, 3000.0, n)
        k[: n // 3] = rng.choice([999.0, 1000.0, 1000.5, 1001.0], n // 3)   # at the switch between the two forms
        mr = k * res * rng.choice([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0], n)
        got = m.calcRange(ox, oy, oa, mr)
        want, visited = lr.oracle_walk(orc, om, ox, oy, oa, mr)
        rays += n
        far += int((visited > 600).sum())
        if not np.array_equal(got, want):
            bad += 1
            i = int(np.flatnonzero(got != want)[0])
            print("MISMATCH map %d (%dx%d res %g): ray %d from (%.3f, %.3f) angle %.9f max %.4f: %r vs %r (%d cells)" %
                  (case, sx, sy, res, i, ox[i], oy[i], oa[i], mr[i], got[i], want[i], visited[i]), flush=True)
    if not quiet:
        print("%d maps, %d rays (%d beyond 600 cells), %d maps mismatching, %.0f s" %
              (maps, rays, far, bad, time.time() - t0))
    if own:
        e.close()
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 6,
                      int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
