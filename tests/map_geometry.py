"""Rectangular, off-centre 2-D maps for the parity tests.  scenario.Scenario builds square maps whose origin follows
the node's centre formula; on those a swapped x / y pair anywhere in the engine (a size, a half size, a tile stride, a
clamp) gives the same results.  The maps here have size_x != size_y, wall lattices with different periods on the two
axes, origins that are negative or no multiple of the cell, and other resolutions; the clouds reach past every edge.

An ordinary module that tests and the soaks under tools/ import, like scenario.py."""
import math

import numpy as np

from badger_amcl_amd import synth
from scenario import Scenario

# name -> (size_x, size_y, resolution, origin); origin None = the node's formula per axis (node_2d.cpp:275-277)
GEOMETRIES = {
    "G1": (333, 150, 0.05, None),                 # wide, odd x; (size + 2) mod 8 = 7 / 0
    "G2": (93, 211, 0.1, (-3.0, 1.5)),            # tall, both odd, negative origin; (size + 2) mod 8 = 7 / 5
    "G3": (151, 62, 0.025, (12.3456, -7.891)),    # (size + 2) mod 8 = 1 / 0, origin no multiple of the cell
    "G4": (5, 12, 0.05, (0.0, 0.0)),              # narrower than one LUT tile (scoring only: no cell far from a wall)
    "L1": (1701, 1003, 0.05, (-7.3, 11.9)),       # tiled LUT image of 3 451 392 B: the tile-sorted form engages
    "L2": (1003, 1701, 0.05, (-7.3, 11.9)),       # ... and its transpose, 3 462 528 B
}


def node_origin(size_x, size_y, res):
    return (np.float32((size_x // 2) * res), np.float32((size_y // 2) * res))


def rect_map(size_x, size_y):
    """cells[int32, size_y x size_x]: border walls, wall segments on a lattice of period 37 in x and 29 in y (so that
    no part of the map is its own transpose), a small unknown strip, and a free neighbourhood of the centre cell
    (size_x // 2, size_y // 2)."""
    sx, sy = int(size_x), int(size_y)
    ys, xs = np.mgrid[0:sy, 0:sx]
    cells = np.full((sy, sx), -1, dtype=np.int32)
    wall = ((xs % 37 == 0) & (ys % 29 < 19)) | ((ys % 29 == 0) & (xs % 37 < 23))
    wall |= (xs == 0) | (ys == 0) | (xs == sx - 1) | (ys == sy - 1)
    cx, cy = sx // 2, sy // 2
    r = min(6, min(sx, sy) // 4)
    centre = np.zeros((sy, sx), dtype=bool)
    centre[max(cy - r, 1):min(cy + r + 1, sy - 1), max(cx - r, 1):min(cx + r + 1, sx - 1)] = True
    wall &= ~centre
    cells[wall] = 1
    strip = (xs >= sx // 3) & (xs < sx // 3 + 3) & (ys > sy // 8) & (ys < sy // 8 + max(sy // 5, 2)) & ~wall & ~centre
    cells[strip] = 0
    return cells


def world_to_cell(x, y, size_x, size_y, origin, res):
    """OccupancyMap::convertWorldToMap (occupancy_map.cpp:90-103) on arrays."""
    i = np.floor((np.asarray(x) - float(origin[0])) / res + 0.5).astype(np.int64) + size_x // 2
    j = np.floor((np.asarray(y) - float(origin[1])) / res + 0.5).astype(np.int64) + size_y // 2
    return i, j


def bounds(size_x, size_y, origin, res):
    """World rectangle [x0, x1) x [y0, y1) that converts to cells inside the map."""
    x0 = float(origin[0]) - (size_x // 2 + 0.5) * res
    y0 = float(origin[1]) - (size_y // 2 + 0.5) * res
    return x0, x0 + size_x * res, y0, y0 + size_y * res


def rect_cloud(n, size_x, size_y, origin, res, margin, seed):
    """Uniform over the map's rectangle grown by `margin` metres on all four sides."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = bounds(size_x, size_y, origin, res)
    s = np.zeros((n, 4), dtype=np.float64)
    s[:, 0] = rng.uniform(x0 - margin, x1 + margin, n)
    s[:, 1] = rng.uniform(y0 - margin, y1 + margin, n)
    s[:, 2] = rng.uniform(-math.pi, math.pi, n)
    s[:, 3] = 1.0 / n
    return s


class GeoScenario(Scenario):
    """Scenario on a rect_map: the same gpu_objects / oracle_planar / oracle_apply interface."""

    def __init__(self, orc, size_x, size_y, res, origin, beams=61, n=257, cloud="spread", max_dist=2.0, seed=3,
                 frac_max=0.03, frac_nan=0.02, scanner_pose=(0.1, -0.05, 0.2), map_factors=synth.MAP_FACTORS,
                 range_max=30.0, margin=None, pose_cell=None):
        self.orc = orc
        self.size_x, self.size_y, self.res = int(size_x), int(size_y), float(res)
        self.cells = rect_map(size_x, size_y)
        if origin is None:
            origin = node_origin(size_x, size_y, res)
        self.origin = (np.float32(origin[0]), np.float32(origin[1]))  # narrowed to float32 as the node does
        self.omap = orc.OccupancyMap(self.cells, self.res, self.origin)
        self.lut = self.omap.update_distances_lut(max_dist)
        self.max_dist = max_dist
        # inside the centre cell (or the free cell asked for), off its middle
        ci, cj = pose_cell if pose_cell is not None else (self.size_x // 2, self.size_y // 2)
        assert self.cells[cj, ci] == -1
        self.pose = np.array([float(self.origin[0]) + (ci - self.size_x // 2 + 0.3) * self.res,
                              float(self.origin[1]) + (cj - self.size_y // 2 - 0.2) * self.res, 0.3])
        self.range_max = range_max
        self.ranges, self.angles = synth.cast_scan(self.cells, self.origin, self.res, self.pose, beams,
                                                   range_max=range_max, seed=seed, frac_max=frac_max,
                                                   frac_nan=frac_nan)
        # a margin past every edge: about a tenth of the shorter side, so that some particles and many beam end points
        # are off the map on all four sides
        self.margin = margin if margin is not None else max(0.1 * min(size_x, size_y) * self.res, 2.5 * self.res)
        sigma = min(0.3, 0.1 * min(size_x, size_y) * self.res)
        if cloud == "converged":
            self.samples = synth.converged_cloud(n, self.pose, seed=seed + 10, sigma=(sigma, sigma, 0.1))
        elif cloud == "spread":
            self.samples = rect_cloud(n, size_x, size_y, self.origin, self.res, self.margin, seed + 11)
        elif cloud == "mixture":
            a = synth.converged_cloud(n - n // 2, self.pose, seed=seed + 10, sigma=(sigma, sigma, 0.1))
            b = rect_cloud(n // 2, size_x, size_y, self.origin, self.res, self.margin, seed + 11)
            self.samples = np.ascontiguousarray(np.concatenate([a, b]))
            self.samples[:, 3] = 1.0 / n
        else:
            raise ValueError(cloud)
        rng = np.random.default_rng(seed + 20)
        self.samples[:, 3] *= rng.uniform(0.5, 1.5, n)  # non-uniform prior weights
        self.scanner_pose = scanner_pose
        self.map_factors = map_factors

    @classmethod
    def named(cls, orc, name, **kw):
        sx, sy, res, origin = GEOMETRIES[name]
        return cls(orc, sx, sy, res, origin, **kw)

    def cells_of(self, samples=None):
        s = self.samples if samples is None else samples
        return world_to_cell(s[:, 0], s[:, 1], self.size_x, self.size_y, self.origin, self.res)

    def in_map(self, samples=None):
        i, j = self.cells_of(samples)
        return (i >= 0) & (i < self.size_x) & (j >= 0) & (j < self.size_y)

    def transposed_blind_fraction(self, samples=None):
        """Of the particles inside the map, the share in cells with i >= size_y (wide map) or j >= size_x (tall map):
        the region an engine that swapped the two sizes would treat as off the map."""
        i, j = self.cells_of(samples)
        inside = self.in_map(samples)
        if self.size_x > self.size_y:
            blind = i >= self.size_y
        elif self.size_y > self.size_x:
            blind = j >= self.size_x
        else:
            raise ValueError("a square map has no such region")
        return float((blind & inside).sum()) / max(int(inside.sum()), 1)

    def off_map_sides(self, samples=None):
        """Number of particles past the -x, +x, -y, +y edge."""
        i, j = self.cells_of(samples)
        return int((i < 0).sum()), int((i >= self.size_x).sum()), int((j < 0).sum()), int((j >= self.size_y).sum())

    def assert_geometry_is_seen(self, samples=None, sides=True):
        """What every test on a wide or tall map asserts about its own input first."""
        assert self.transposed_blind_fraction(samples) >= 0.2
        if sides:
            assert min(self.off_map_sides(samples)) > 0

    def free_space(self, ref):
        """pose_check_ref.FreeSpace of this map (Node2D::updateFreeSpaceIndices + convertMapToWorld)."""
        return ref.FreeSpace.planar(self.free_cells(), self.size_x, self.size_y, self.origin, self.res)

    def free_cells(self):
        """pose_check_ref.free_cells_2d as array operations (i outer, j inner; the comparison in double, as there)."""
        mask = (self.cells == -1) & (self.lut.astype(np.float64) > self.map_factors[2])
        return [(int(i), int(j)) for i, j in np.argwhere(mask.T)]
