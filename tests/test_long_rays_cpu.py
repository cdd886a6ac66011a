"""The inputs of the long-ray GPU tests (tests/long_rays.py), held from the oracle alone to what they are there for:
rays that the reference walks for more than 600, 900, 1000, 10 000 and 30 000 cells, on both sides of the engine's
switch between the integer and the fp64 form of its walk, with far hits, full-length misses and starts off the map;
and a beam-model scene whose weights depend on where its long walks end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_rays as lr  # noqa: E402


def test_open_map_is_sparse_and_walled():
    cells = lr.open_map(1400, 1050, 1)
    assert cells.shape == (1050, 1400) and cells.dtype == np.int32
    assert np.all(cells[0, :] == 1) and np.all(cells[-1, :] == 1) and np.all(cells[:, 0] == 1) and np.all(cells[:, -1] == 1)
    inner = cells[1:-1, 1:-1]
    assert 10 <= (inner == 1).sum() <= 60 and 1 <= (inner == 0).sum() <= 25     # 2e-5 and 5e-6 of 1.47 M cells
    assert not np.array_equal(lr.open_map(1400, 1050, 2), cells)


@pytest.mark.parametrize("name", ["fan_wide", "fan_tall"])
def test_fan_walks_far_in_both_forms(orc, name):
    c = lr.ray_case(orc, name)
    assert (c.omap.size_x, c.omap.size_y) in ((1400, 1050), (1050, 1400)) and c.mr.shape == (20000,)
    assert c.omap.origin == lr.ORIGIN and c.omap.resolution == 0.05
    assert np.all((c.oa > -np.pi) & (c.oa <= np.pi))
    assert c.oa[3] == 0.0 and c.oa[7] == np.pi and c.oa[8] == 1e-9 and c.oa[9] == -1e-9
    assert np.array_equal(c.oa[:10], c.oa[390:400])
    k = np.abs(c.mr) / 0.05
    assert set(np.round(k, 1)) == set(lr.FAN_CELLS) and 0.03 < (c.mr < 0).mean() < 0.07
    # 1000 cells is on the integer side of the switch, 1000.5 on the other
    assert c.int_form[np.round(k, 1) == 1000.0].all() and not c.int_form[np.round(k, 1) == 1000.5].any()
    v, w, mr = c.visited, c.want, c.mr
    hit = (w != mr) & (w != 0.0)
    # (share of rays beyond 600 cells, beyond `far` cells, of hits after 600 cells, at max_range, at 0)
    for cls, far, need in ((c.int_form, 900, (0.25, 0.05, 0.10, 0.05, 0.05)),
                           (~c.int_form, 1000, (0.25, 0.03, 0.15, 0.05, 0.05))):
        got = ((v[cls] > 600).mean(), (v[cls] > far).mean(), (hit[cls] & (v[cls] > 600)).mean(),
               (w[cls] == mr[cls]).mean(), (w[cls] == 0.0).mean())
        print(name, "int" if far == 900 else "fp64", int(cls.sum()), ["%.3f" % g for g in got])
        assert cls.sum() > 5000
        assert all(g >= n for g, n in zip(got, need)), (name, far, got)
    # the negated ranges are walked too, and come back negative where nothing is hit
    assert (v[mr < 0] > 600).mean() > 0.2 and (w[mr < 0] == mr[mr < 0]).any()


@pytest.mark.parametrize("name", ["strip_wide", "strip_tall"])
def test_strips_walk_tens_of_thousands_of_cells(orc, name):
    c = lr.ray_case(orc, name)
    assert (c.omap.size_x, c.omap.size_y) in ((33000, 17), (17, 33000))
    k = np.abs(c.mr) / 0.05
    assert k.min() >= 20000 and k.max() < lr.MAX_RAY_CELLS and not c.int_form.any()
    n = c.mr.shape[0]
    fixed = slice(n - n // 10, n)
    assert np.all(k[fixed] == k.max()) and abs(k.max() - 32759) < 1e-6
    got = (c.visited > 10000).mean(), (c.visited > 30000).mean()
    print(name, ["%.3f" % g for g in got], "fixed group beyond 30 000: %.3f" % (c.visited[fixed] > 30000).mean())
    assert got[0] >= 0.30 and got[1] >= 0.08, got
    # both directions of the long axis are walked far, and far walks end in hits as well as at max_range
    ahead = np.cos(c.oa) > 0 if c.omap.size_x > c.omap.size_y else np.sin(c.oa) > 0
    assert (c.visited[ahead] > 10000).sum() > 200 and (c.visited[~ahead] > 10000).sum() > 200
    far = c.visited > 10000
    assert (c.want[far] != c.mr[far]).sum() > 200 and (c.want[far] == c.mr[far]).sum() > 20


@pytest.mark.parametrize("name", ["three_widest", "three_tall", "three_tallest"])
def test_three_cell_maps_have_long_walks_and_whole_line_steps(orc, name):
    c = lr.ray_case(orc, name)
    sx, sy = c.omap.size_x, c.omap.size_y
    assert min(sx, sy) == 3 and max(sx, sy) in (lr.WIDEST, 60000)
    assert lr.WIDEST + 3 < (1 << 21) <= lr.WIDEST + 4 and 4 * (lr.WIDEST + 2) < (1 << 23) <= 4 * (lr.WIDEST + 2) + 8
    k = np.abs(c.mr) / 0.05
    assert 1.0 <= k.min() and k.max() <= 3000.0
    ca, sa = np.abs(np.cos(c.oa)), np.abs(np.sin(c.oa))
    across = (sa > ca) if sx > sy else (ca > sa)          # the major axis is the short one
    inside = c.want != 0.0
    print(name, "beyond 1000 cells %.3f, across %d (inside the map %d)" %
          ((c.visited > 1000).mean(), across.sum(), (across & inside).sum()))
    assert (c.visited > 1000).mean() >= 0.40
    assert (across & inside).sum() >= 300
    assert (c.int_form & (c.visited > 600)).sum() > 100 and (~c.int_form & (c.visited > 1000)).sum() > 1000


@pytest.mark.parametrize("shape", sorted(lr.BEAM_SHAPES))
@pytest.mark.parametrize("cells", lr.BEAM_RANGE_CELLS)
def test_beam_scene_depends_on_the_far_end_of_its_walks(orc, shape, cells):
    s = lr.beam_scene(orc, shape, cells)
    assert s.ranges.shape == (lr.BEAM_BEAMS,) and s.samples.shape == (lr.BEAM_N, 4) and np.isfinite(s.ranges).all()
    assert s.omap.world_to_map(float(s.pose[0]), float(s.pose[1])) == (120, 90)
    assert (s.ranges > 30.0).mean() >= 0.30
    assert (s.ranges == s.range_max).sum() >= 1 and (s.ranges < s.range_max).mean() > 0.5
    assert (s.range_max / s.res <= lr.INT_FORM_CELLS) == (cells == 999)
    want, total = s.oracle_weights()
    assert np.isfinite(total) and total > 0.0 and want[:, 3].std() > 0.01 * want[:, 3].mean()
    other, _ = s.oracle_weights(s.far_walls_thickened())
    changed = np.abs(other[:, 3] - want[:, 3]) > 1e-6 * want[:, 3]
    print(shape, cells, "beyond 30 m %.3f, weights changed %.3f" % ((s.ranges > 30.0).mean(), changed.mean()))
    assert changed.mean() > 0.90
