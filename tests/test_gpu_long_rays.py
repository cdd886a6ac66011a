"""OccupancyMap::calcRange on the device (calc_range_skip behind bpf_map2d_calc_range) against the oracle's cell-by-cell
walk, at the sizes its exactness arguments speak of: the integer minor-axis form up to its last ray length (1000
cells, with the end cell one further), the fp64 form up to 32 759 cells, and the widest line of the grid the 24-bit
multiply-adds may see (size_x = 2^21 - 4).  The inputs are those of tests/long_rays.py, which test_long_rays_cpu.py
holds to what they are for; every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_rays as lr  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_CAPACITY = 8


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _check(c, got, what=None):
    bad = np.flatnonzero(got != c.want)
    assert np.array_equal(got, c.want), (what or c.name, bad.size, [
        (int(k), c.ox[k], c.oy[k], c.oa[k], c.mr[k], got[k], c.want[k], int(c.visited[k])) for k in bad[:5]])


def _walk_case(engine, orc, name):
    c = lr.ray_case(orc, name)
    m = c.gpu_map(engine)
    got = m.calcRange(c.ox, c.oy, c.oa, c.mr)
    _check(c, got)
    return c, m


def _valid_batch(engine, orc, m=None, c=None):
    """A batch the engine has to answer correctly after it refused another: on the map that is set, or on the fan's."""
    if m is None:
        c = lr.ray_case(orc, "fan_wide")
        m = c.gpu_map(engine)
    k = slice(0, 1000)
    got = m.calcRange(c.ox[k], c.oy[k], c.oa[k], c.mr[k])
    assert np.array_equal(got, c.want[k]), (c.name, np.flatnonzero(got != c.want[k])[:10])


@pytest.mark.parametrize("name", ["fan_wide", "fan_tall"])
def test_fan_on_an_open_map_matches_the_oracle(engine, orc, name):
    """20 000 rays of 700 ... 1800 cells on 1400 x 1050 and 1050 x 1400: both forms, a third of each class beyond 600
    cells, the integer form up to rays whose end cell is 1001 cells away."""
    c, _ = _walk_case(engine, orc, name)
    assert (c.visited[c.int_form] > 900).sum() > 300 and (c.visited[~c.int_form] > 1000).sum() > 300


@pytest.mark.parametrize("name", ["strip_wide", "strip_tall"])
def test_strips_match_the_oracle(engine, orc, name):
    """33 000 x 17 and 17 x 33 000: the fp64 form with step indices up to 32 761."""
    c, _ = _walk_case(engine, orc, name)
    assert (c.visited > 30000).mean() >= 0.08 and c.visited.max() >= 32760


@pytest.mark.parametrize("name", ["three_widest", "three_tall", "three_tallest"])
def test_three_cell_maps_match_the_oracle(engine, orc, name):
    """size_x = 2^21 - 4 with size_y = 3: four times the grid's line is at the top of the signed 24-bit range, and the
    rays across the map step by one whole line, either way; 40 % of the rays walk more than 1000 cells along it.  The
    transposed kind of map at 3 x 60 000 and at 3 x (2^21 - 4)."""
    c, _ = _walk_case(engine, orc, name)
    assert (c.visited > 1000).mean() >= 0.40


def test_a_map_one_cell_too_wide_is_refused(engine, orc):
    """size_x = 2^21 - 3: BPF_ERR_CAPACITY, and the engine goes on answering."""
    import badger_amcl_amd as bpf
    m = bpf.OccupancyMap(engine, lr.RES)
    m.setCells(np.full((3, lr.WIDEST + 1), -1, dtype=np.int32))
    m.setOrigin(lr.ORIGIN)
    one = np.array([float(lr.ORIGIN[0])]), np.array([float(lr.ORIGIN[1])])
    with pytest.raises(bpf.BpfError) as ei:
        m.calcRange(one[0], one[1], np.array([0.1]), np.array([5.0]))
    assert ei.value.code == ERR_CAPACITY
    _valid_batch(engine, orc)


def test_ray_length_guard_sits_at_32760_cells(engine, orc):
    """max_range of exactly 32 760 cells, either sign, NaN and inf are refused with BPF_ERR_CAPACITY; the next double
    below 32 760 cells is walked, to the cell the oracle finds.  After every refusal the engine answers the strip's
    own first rays."""
    import badger_amcl_amd as bpf
    c = lr.ray_case(orc, "strip_wide")
    m = c.gpu_map(engine)
    res = c.omap.resolution
    edge = lr.MAX_RAY_CELLS * res
    while edge / res < lr.MAX_RAY_CELLS:       # the smallest max_range the guard refuses
        edge = np.nextafter(edge, np.inf)
    while np.nextafter(edge, 0.0) / res >= lr.MAX_RAY_CELLS:
        edge = np.nextafter(edge, 0.0)
    below = np.nextafter(edge, 0.0)
    assert edge / res >= lr.MAX_RAY_CELLS > below / res and abs(edge / res - lr.MAX_RAY_CELLS) < 1e-6
    # along the corridor from its first cells, straight and at a slope, forwards; backwards from its last cells; and
    # across the strip
    x0, x1, y0, y1 = lr.bounds(c.omap.size_x, c.omap.size_y, c.omap.origin, res)
    yc = y0 + (c.omap.size_y // 2 + 0.5) * res
    ox = np.array([x0 + 3.3 * res, x0 + 40.2 * res, x0 + 150.7 * res, x1 - 3.3 * res, x1 - 120.4 * res, x0 + 900 * res])
    oy = np.full(ox.shape, yc)
    oa = np.array([0.0, 3e-5, -4e-5, np.pi, np.pi - 2e-5, 1.0])
    n = ox.shape[0]
    for bad in (edge, -edge, float("nan"), float("inf"), -float("inf")):
        for k in (0, n - 1):
            mr = np.full(n, below)
            mr[k] = bad
            with pytest.raises(bpf.BpfError) as ei:
                m.calcRange(ox, oy, oa, mr)
            assert ei.value.code == ERR_CAPACITY, bad
        _valid_batch(engine, orc, m, c)
    for sign in (1.0, -1.0):
        mr = np.full(n, sign * below)
        oa_s = oa if sign > 0 else oa + np.pi     # a negated range walks the other way
        got = m.calcRange(ox, oy, oa_s, mr)
        want, visited = lr.oracle_walk(orc, c.omap, ox, oy, oa_s, mr)
        assert np.array_equal(got, want), (sign, got, want)
        assert visited.max() > 32700, visited
