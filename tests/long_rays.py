"""Maps and ray sets on which OccupancyMap::calcRange walks far: the inputs of test_long_rays_cpu.py (which holds them
to what they are for, from the oracle alone), test_gpu_long_rays.py, test_gpu_long_beams.py and tools/soak_long_rays.py.

The engine's walk (calc_range_skip) has an integer minor-axis form for rays of at most 1000 cells and an fp64 form
from there to 32 760 cells; the other maps of this suite are walled, so their rays end after a few hundred cells
whatever max_range says.  Here the maps are open (a few single obstacles), long and narrow, or three cells wide.

An ordinary module, like map_geometry.py."""
import ctypes as C
import math

import numpy as np

from map_geometry import bounds

RES = 0.05
ORIGIN = (np.float32(-7.3), np.float32(11.9))
INT_FORM_CELLS = 1000      # fabs(max_range) / resolution <= this: the engine's integer form (kIntDivRayCells)
MAX_RAY_CELLS = 32760      # fabs(max_range) / resolution must stay below this (kMaxRayCells)
FAN_CELLS = (700, 999, 1000, 1000.5, 1001, 1002, 1300, 1800)
WIDEST = (1 << 21) - 4     # the widest map the ray walk's guard admits (size_x + 3 < 2^21)


def open_map(size_x, size_y, seed):
    """cells[int32, size_y x size_x]: free, single occupied cells at density 2e-5, unknown cells at 5e-6, border
    walls."""
    rng = np.random.default_rng(seed)
    u = rng.random((int(size_y), int(size_x)))
    cells = np.full(u.shape, -1, dtype=np.int32)
    cells[u < 2e-5] = 1
    cells[(u >= 2e-5) & (u < 2.5e-5)] = 0
    cells[0, :] = cells[-1, :] = 1
    cells[:, 0] = cells[:, -1] = 1
    return cells


def strip_map(size_x, size_y, seed):
    """open_map of a long narrow map with the five middle lines of the long axis free from wall to wall: the corridor
    of strip_rays' fixed group."""
    cells = open_map(size_x, size_y, seed)
    if size_x >= size_y:
        c = size_y // 2
        cells[c - 2:c + 3, 1:-1] = -1
    else:
        c = size_x // 2
        cells[1:-1, c - 2:c + 3] = -1
    return cells


def three_cell_map(size_x, size_y, seed, density=1e-4):
    """No border walls (there is no room for them): free cells with occupied ones at `density`."""
    rng = np.random.default_rng(seed)
    cells = np.full((int(size_y), int(size_x)), -1, dtype=np.int32)
    cells[rng.random(cells.shape) < density] = 1
    return cells


def _origins(rng, omap, n, grow=0.03):
    x0, x1, y0, y1 = bounds(omap.size_x, omap.size_y, omap.origin, omap.resolution)
    gx, gy = grow * (x1 - x0), grow * (y1 - y0)
    return rng.uniform(x0 - gx, x1 + gx, n), rng.uniform(y0 - gy, y1 + gy, n)


def fan(omap, n, seed):
    """(ox, oy, oa, max_range) of n rays on an open map: origins uniform over the map's world rectangle grown by 3 %
    on each side, angles uniform in (-pi, pi] but for the first 400 (40 repeats of the eight multiples of pi / 4 and
    of +-1e-9), max_range = k cells with k from FAN_CELLS -- both sides of the engine's switch between its two forms
    -- and 5 % of the ranges negated (the reference then walks backwards)."""
    rng = np.random.default_rng(seed)
    ox, oy = _origins(rng, omap, n)
    oa = -rng.uniform(-math.pi, math.pi, n)   # uniform() draws from [-pi, pi)
    special = np.array([k * (math.pi / 4) for k in range(-3, 5)] + [1e-9, -1e-9])
    oa[:400] = np.tile(special, 40)
    mr = rng.choice(np.array(FAN_CELLS), n) * omap.resolution
    mr[rng.random(n) < 0.05] *= -1.0
    return ox, oy, oa, mr


def strip_rays(omap, n, seed):
    """n rays on a strip_map.  60 % point along the long axis, either way, +- uniform(-3e-4, 3e-4); 30 % have uniform
    angles; both start anywhere (as fan's do) with max_range uniform in [20 000, 32 759] cells.  The last 10 % are a
    fixed group: they start in the first 2 % of the long axis inside the middle cell of the short one, deviate at most
    5e-5 rad from the long axis and have a max_range of 32 759 cells, so they stay in the free corridor (1.64 cells of
    drift) and reach the far wall."""
    rng = np.random.default_rng(seed)
    res = omap.resolution
    wide = omap.size_x >= omap.size_y
    along = 0.0 if wide else math.pi / 2
    ox, oy = _origins(rng, omap, n)
    oa = rng.uniform(-math.pi, math.pi, n)
    n_axis, n_fixed = int(0.6 * n), n // 10
    oa[:n_axis] = along + rng.choice([0.0, math.pi], n_axis) + rng.uniform(-3e-4, 3e-4, n_axis)
    mr = rng.uniform(20000, MAX_RAY_CELLS - 1, n) * res
    x0, x1, y0, y1 = bounds(omap.size_x, omap.size_y, omap.origin, res)
    f = slice(n - n_fixed, n)
    lo, hi = (x0, x1) if wide else (y0, y1)
    s0 = (y0 if wide else x0) + ((omap.size_y if wide else omap.size_x) // 2 + 0.5) * res  # middle of the middle cell
    longs = rng.uniform(lo + 2 * res, lo + 0.02 * (hi - lo), n_fixed)
    shorts = s0 + rng.uniform(-0.4, 0.4, n_fixed) * res
    ox[f], oy[f] = (longs, shorts) if wide else (shorts, longs)
    oa[f] = along + rng.uniform(-5e-5, 5e-5, n_fixed)
    mr[f] = (MAX_RAY_CELLS - 1) * res
    return ox, oy, oa, mr


def three_cell_rays(omap, n, seed, along_share=0.8):
    """n rays of 1 ... 3000 cells on a map three cells wide, starting anywhere.  A fifth have uniform angles: on
    such a map nearly all of them are steep (their major step is one whole line of the grid, either way) and leave
    after a step or two.  Uniform angles alone would leave no ray that walks far, so the other four fifths point
    along the long axis, either way, +- uniform(-3e-4, 3e-4) (0.9 cells of drift at 3000 cells)."""
    rng = np.random.default_rng(seed)
    along = 0.0 if omap.size_x >= omap.size_y else math.pi / 2
    ox, oy = _origins(rng, omap, n)
    oa = rng.uniform(-math.pi, math.pi, n)
    k = int(along_share * n)
    oa[:k] = along + rng.choice([0.0, math.pi], k) + rng.uniform(-3e-4, 3e-4, k)
    mr = rng.uniform(1.0, 3000.0, n) * omap.resolution
    return ox, oy, oa, mr


def oracle_walk(orc, omap, ox, oy, oa, mr):
    """Per ray: the oracle's calcRange and the number of cells its walk visited."""
    lib = orc.lib()
    m = omap.struct()
    mp = C.byref(m)
    n = len(ox)
    dist = np.zeros(n, dtype=np.float64)
    cells = np.zeros(n, dtype=np.int64)
    visited = C.c_long(0)
    vp = C.byref(visited)
    f = lib.orc_map2d_calc_range
    for i in range(n):
        visited.value = 0
        dist[i] = f(mp, float(ox[i]), float(oy[i]), float(oa[i]), float(mr[i]), vp)
        cells[i] = visited.value
    return dist, cells


def int_form(omap, mr):
    """The engine's own test for the integer form of the walk (k_calc_range)."""
    return np.abs(mr) / omap.resolution <= float(INT_FORM_CELLS)


# name -> (map builder, size_x, size_y, map seed, ray generator, rays, ray seed)
CASES = {
    "fan_wide": (open_map, 1400, 1050, 1, fan, 20000, 11),
    "fan_tall": (open_map, 1050, 1400, 2, fan, 20000, 12),
    "strip_wide": (strip_map, 33000, 17, 3, strip_rays, 4000, 13),
    "strip_tall": (strip_map, 17, 33000, 4, strip_rays, 4000, 14),
    "three_widest": (three_cell_map, WIDEST, 3, 5, three_cell_rays, 4000, 15),
    "three_tall": (three_cell_map, 3, 60000, 6, three_cell_rays, 4000, 16),
    "three_tallest": (three_cell_map, 3, WIDEST, 7, three_cell_rays, 4000, 17),
}
_CASES = {}


class RayCase:
    """A map, its rays and the oracle's answers, computed once per process and left unchanged."""

    def __init__(self, orc, name):
        build, sx, sy, map_seed, rays, n, ray_seed = CASES[name]
        self.name = name
        self.cells = build(sx, sy, map_seed)
        self.omap = orc.OccupancyMap(self.cells, RES, ORIGIN)
        self.ox, self.oy, self.oa, self.mr = rays(self.omap, n, ray_seed)
        self.want, self.visited = oracle_walk(orc, self.omap, self.ox, self.oy, self.oa, self.mr)
        self.int_form = int_form(self.omap, self.mr)
        for a in (self.cells, self.ox, self.oy, self.oa, self.mr, self.want, self.visited):
            a.setflags(write=False)

    def gpu_map(self, engine):
        import badger_amcl_amd as bpf
        m = bpf.OccupancyMap(engine, RES)
        m.setCells(self.cells)
        m.setOrigin(ORIGIN)
        return m


def ray_case(orc, name):
    if name not in _CASES:
        _CASES[name] = RayCase(orc, name)
    return _CASES[name]


# ------------------------------------------------------------------------------------------------ beam-model scene
BEAM_SHAPES = {"wide": (1400, 1050), "tall": (1050, 1400)}
BEAM_RANGE_CELLS = (999, 1001, 1600)   # one launch in the integer form, two in the fp64 form
BEAM_N, BEAM_BEAMS = 257, 128          # 128 beams: two trips of a wave
BEAM_SCANNER_POSE = (0.1, -0.05, 0.2)
BEAM_MAX_DIST = 2.0


class BeamScene:
    """The beam model on an open map: the true pose in the cell (120, 90), off its middle, heading 0.6; 128 beams cast
    at range_max (3 % of them then set to range_max itself, the z_max term); 257 particles within sigma (0.05, 0.05,
    0.002) of the pose, so that z = obs - map_range stays within a few sigma_hit on the long beams too; non-uniform prior weights, as scenario.Scenario has them."""

    def __init__(self, orc, shape, range_cells, seed=5):
        from badger_amcl_amd import synth
        self.orc = orc
        self.size_x, self.size_y = BEAM_SHAPES[shape]
        self.res, self.origin = RES, ORIGIN
        self.cells = open_map(self.size_x, self.size_y, seed)
        self.omap = orc.OccupancyMap(self.cells, self.res, self.origin)
        self.max_dist = BEAM_MAX_DIST
        self.lut = self.omap.update_distances_lut(self.max_dist)
        ci, cj = 120, 90
        assert np.all(self.cells[cj - 1:cj + 2, ci - 1:ci + 2] == -1)
        self.pose = np.array([float(self.origin[0]) + (ci - self.size_x // 2 + 0.3) * self.res,
                              float(self.origin[1]) + (cj - self.size_y // 2 - 0.2) * self.res, 0.6])
        self.range_max = range_cells * self.res
        self.ranges, self.angles = synth.cast_scan(self.cells, self.origin, self.res, self.pose, BEAM_BEAMS,
                                                   range_max=self.range_max, seed=seed, frac_max=0.03, frac_nan=0.0)
        self.samples = synth.converged_cloud(BEAM_N, self.pose, seed=seed + 10, sigma=(0.05, 0.05, 0.002))
        self.samples[:, 3] *= np.random.default_rng(seed + 20).uniform(0.5, 1.5, BEAM_N)
        self.params = dict(synth.BEAM_DEFAULTS)
        self.map_factors = synth.MAP_FACTORS

    def planar(self):
        mf = self.map_factors
        return self.orc.planar(self.orc.MODEL_BEAM, BEAM_BEAMS, scanner_pose=BEAM_SCANNER_POSE, off_map_factor=mf[0],
                               non_free_space_factor=mf[1], non_free_space_radius=mf[2], **self.params)

    def oracle_weights(self, omap=None):
        """(samples with the oracle's weights, total), on this scene's map or on another one handed in."""
        want = self.samples.copy()
        total = self.orc.planar_apply(self.planar(), omap if omap is not None else self.omap, want, self.ranges,
                                      self.angles, self.range_max, 0)
        return want, total

    def far_walls_thickened(self):
        """The same map and LUT with the two far walls one cell thicker."""
        cells = self.cells.copy()
        cells[-2, :] = 1
        cells[:, -2] = 1
        return self.orc.OccupancyMap(cells, self.res, self.origin, self.max_dist, lut=self.lut)

    def gpu_objects(self, engine):
        import badger_amcl_amd as bpf
        m = bpf.OccupancyMap(engine, self.res)
        m.setCells(self.cells)
        m.setOrigin(self.origin)
        m.setDistancesLUT(self.lut, self.max_dist)
        sc = bpf.PlanarScanner(engine)
        sc.init(BEAM_BEAMS, m)
        p = self.params
        sc.setModelBeam(p["z_hit"], p["z_short"], p["z_max"], p["z_rand"], p["sigma_hit"], p["lambda_short"])
        sc.setMapFactors(*self.map_factors)
        sc.setPlanarScannerPose(BEAM_SCANNER_POSE)
        pf = bpf.ParticleFilter(engine, 100, BEAM_N, 0.0, 0.0, 85.0)
        pf.srand48(42)
        pf.initWithSamples(self.samples)
        return m, sc, pf, bpf.PlanarData(self.ranges, self.angles, self.range_max)


_SCENES = {}


def beam_scene(orc, shape, range_cells):
    key = (shape, range_cells)
    if key not in _SCENES:
        _SCENES[key] = BeamScene(orc, shape, range_cells)
    return _SCENES[key]
