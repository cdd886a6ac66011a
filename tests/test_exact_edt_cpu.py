"""exact_edt_ref.py on the CPU: the direct transform against a cell-by-cell restatement and against itself walked the
other way, what the seam maps promise, and the brushfire bound that test_gpu_exact_edt.py keeps beside its equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exact_edt_ref import direct_edt, radius_cells, seam_map  # noqa: E402
from map_geometry import rect_map  # noqa: E402

MAX_DISTS = [0.04, 0.07, 0.5, 2.0, 0.33]   # those of test_gpu_exact_edt.py


def test_radii_are_what_the_cases_say():
    assert [radius_cells(d, 0.05) for d in MAX_DISTS] == [0, 1, 10, 40, 6]
    assert [radius_cells(d, 0.025) for d in MAX_DISTS] == [1, 2, 20, 80, 13]
    assert [radius_cells(d, 0.1) for d in MAX_DISTS] == [0, 0, 5, 20, 3]


@pytest.mark.parametrize("max_dist", [0.04, 0.07, 0.33])
def test_direct_transform_cell_by_cell(max_dist):
    rng = np.random.default_rng(2)
    cells = rng.choice(np.array([-1, -1, -1, -1, -1, -1, 0, 1], dtype=np.int32), (13, 21))
    cells[:6, :9] = -1
    res = 0.05
    r = radius_cells(max_dist, res)
    want = np.zeros(cells.shape, dtype=np.float32)
    for y in range(13):
        for x in range(21):
            best = None
            for b in range(-r, r + 1):
                for a in range(-r, r + 1):
                    if 0 <= y + b < 13 and 0 <= x + a < 21 and cells[y + b, x + a] == 1:
                        best = a * a + b * b if best is None else min(best, a * a + b * b)
            want[y, x] = np.float32(np.sqrt(float(best)) * res) if best is not None and best <= r * r \
                else np.float32(max_dist)
    for walk in ("occupied", "offsets"):
        assert np.array_equal(direct_edt(cells, res, max_dist, walk), want), walk


@pytest.mark.parametrize("shape", [(600, 70), (70, 600)])
def test_seam_maps_straddle_the_block_seams(shape):
    sx, sy = shape
    cells = seam_map(sx, sy)
    assert cells.shape == (sy, sx) and cells.dtype == np.int32 and cells.flags.c_contiguous
    assert np.array_equal(seam_map(sy, sx), cells.T)
    line = (cells == 1).any(axis=0) if sx > sy else (cells == 1).any(axis=1)
    assert line.size == 600 and line[[253, 255, 256, 258, 509, 511, 512, 514]].all()
    assert 0.005 < (cells == 0).mean() < 0.015 and 0.002 < (cells == 1).mean() < 0.006
    a = direct_edt(cells, 0.05, 0.5, "occupied")
    assert np.array_equal(a, direct_edt(cells, 0.05, 0.5, "offsets"))
    # near cells in each of the three block columns, at every radius; capped ones at the small radii
    for max_dist in MAX_DISTS:
        lut = direct_edt(cells, 0.05, max_dist)
        near = lut < np.float32(max_dist)
        along = near.any(axis=0) if sx > sy else near.any(axis=1)
        assert all(along[k:k + 256].any() for k in (0, 256, 512)), max_dist
        if radius_cells(max_dist, 0.05) <= 10:
            assert (~near).mean() > 0.2, max_dist


@pytest.mark.parametrize("res", [0.025, 0.05, 0.1])
@pytest.mark.parametrize("shape", [(333, 150), (93, 211)])
def test_direct_transform_is_never_above_the_brushfire(orc, shape, res):
    cells = rect_map(*shape)
    for max_dist in MAX_DISTS:
        brushfire = orc.OccupancyMap(cells, res, (-3.0, 1.5)).update_distances_lut(max_dist)
        lut = direct_edt(cells, res, max_dist)
        assert np.all(lut <= brushfire), (max_dist, int((lut > brushfire).sum()))
        assert np.mean(lut == brushfire) > 0.9, max_dist
