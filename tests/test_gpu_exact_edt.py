"""updateDistancesLUTExact (k_edt_rows / k_edt_cols behind bpf_map2d_build_distances_lut) against the transform written
out directly (exact_edt_ref.direct_edt), exactly: on rectangles, on maps three 256-thread blocks wide with obstacles
whose windows straddle the block seams, at three resolutions and at radii of 0, 1, a few and 80 cells.  The other
tests of this builder on maps wider than one block assert only that it stays below the brushfire."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exact_edt_ref import direct_edt, radius_cells, seam_map  # noqa: E402
from map_geometry import rect_map  # noqa: E402

pytestmark = pytest.mark.gpu

MAPS = {"rect_wide": (333, 150), "rect_tall": (93, 211), "seam_wide": (600, 70), "seam_tall": (70, 600)}
RESOLUTIONS = [0.025, 0.05, 0.1]
# r = 0 and r = 1 at 0.05 m, two everyday values, and one that is no multiple of any of the three cells
MAX_DISTS = [0.04, 0.07, 0.5, 2.0, 0.33]
ORIGIN = (-3.0, 1.5)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


_CELLS = {}


def cells_of(name):
    if name not in _CELLS:
        sx, sy = MAPS[name]
        _CELLS[name] = rect_map(sx, sy) if name.startswith("rect") else seam_map(sx, sy)
        _CELLS[name].setflags(write=False)
    return _CELLS[name]


def gpu_map(engine, cells, res):
    import badger_amcl_amd as bpf
    m = bpf.OccupancyMap(engine, res)
    m.setCells(cells)
    m.setOrigin(ORIGIN)
    return m


def exact_lut(engine, cells, res, max_dist):
    m = gpu_map(engine, cells, res)
    m.updateDistancesLUTExact(max_dist)
    lut = m.getDistancesLUT()
    assert lut.shape == cells.shape and lut.dtype == np.float32
    return lut


def assert_same(got, want, what):
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (what, len(bad), [(int(y), int(x), float(got[y, x]), float(want[y, x]))
                                                        for y, x in bad[:8]])


@pytest.mark.parametrize("max_dist", MAX_DISTS)
@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("name", sorted(MAPS))
def test_exact_lut_is_the_direct_transform(engine, orc, name, res, max_dist):
    cells = cells_of(name)
    got = exact_lut(engine, cells, res, max_dist)
    want = direct_edt(cells, res, max_dist)
    assert_same(got, want, (name, res, max_dist, radius_cells(max_dist, res)))
    if name.startswith("rect"):
        brushfire = orc.OccupancyMap(cells, res, ORIGIN).update_distances_lut(max_dist)
        assert np.all(got <= brushfire)


@pytest.mark.parametrize("name", ["seam_wide", "seam_tall"])
@pytest.mark.parametrize("max_dist", [0.5, 2.0])
def test_reference_builder_is_still_the_brushfire(engine, orc, name, max_dist):
    """updateDistancesLUT, the reference-named builder, on the maps three blocks wide: the oracle's brushfire byte for
    byte."""
    cells = cells_of(name)
    m = gpu_map(engine, cells, 0.05)
    m.updateDistancesLUT(max_dist)
    want = orc.OccupancyMap(cells, 0.05, ORIGIN).update_distances_lut(max_dist)
    assert m.getDistancesLUT().tobytes() == want.tobytes()


@pytest.mark.parametrize("shape", [(300, 40), (40, 300)])
def test_maps_without_and_of_nothing_but_obstacles(engine, shape):
    sx, sy = shape
    free = np.full((sy, sx), -1, dtype=np.int32)
    free[3, 5:9] = 0                                   # unknown is not occupied
    got = exact_lut(engine, free, 0.05, 0.5)
    assert np.all(got == np.float32(0.5))
    full = np.ones((sy, sx), dtype=np.int32)
    got = exact_lut(engine, full, 0.05, 0.5)
    assert np.all(got == 0.0)
    assert_same(got, direct_edt(full, 0.05, 0.5), shape)


@pytest.mark.parametrize("shape", [(300, 40), (40, 300)])
def test_unknown_cells_are_no_obstacles(engine, shape):
    """A map that is half unknown: the LUT of the same map with the unknown cells free, and the direct transform."""
    sx, sy = shape
    rng = np.random.default_rng(4)
    cells = np.full((sy, sx), -1, dtype=np.int32)
    u = rng.random(cells.shape)
    cells[u < 0.5] = 0
    cells[u < 0.004] = 1
    got = exact_lut(engine, cells, 0.05, 0.5)
    assert_same(got, direct_edt(cells, 0.05, 0.5), shape)
    as_free = np.where(cells == 0, -1, cells).astype(np.int32)
    assert_same(got, exact_lut(engine, as_free, 0.05, 0.5), shape)
    assert (got < np.float32(0.5)).mean() > 0.3 and (got == np.float32(0.5)).mean() > 0.05


def test_max_dist_zero_leaves_the_lut_untouched(engine):
    cells = cells_of("seam_wide")
    m = gpu_map(engine, cells, 0.05)
    m.updateDistancesLUTExact(0.5)
    before = m.getDistancesLUT()
    m.updateDistancesLUTExact(0.0)
    assert np.array_equal(m.getDistancesLUT(), before)
    assert_same(before, direct_edt(cells, 0.05, 0.5), "before")
