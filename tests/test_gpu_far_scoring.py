"""Planar scoring, ray casting and pose generation on maps whose origin is far from the world origin: 151 x 62 cells
at 0.05 m with origin (41 234.5678, -1 003 456.789) and 93 x 211 at 0.1 m with origin (-3.2e6, 2.9e6), narrowed to
float32 as the node does (map_geometry.GeoScenario).

field_prep_of forms (sp.x - origin) / res once and adds the rotated beam to it; the reference rounds
x + r cos(theta + b) at the magnitude of x first.  The two differ by about ulp(|x|) / res cells, so an end point
within that distance of a cell border may land in the neighbour cell: about 2 ulp(|x|) / res per evaluation and axis
 -- 5e-9 (nearly all of it from y, a million metres out) and 1.9e-8 over both axes here, against
~1e-12 near the origin.  With 4097 x 61 = 2.5e5 evaluations per case that is 1.2e-3 and 4.7e-3 expected knife-edge
weights, and the existing budget (weights 1e-9 relative, at most one knife-edge weight) holds as it stands."""
import math

import numpy as np
import pytest

from map_geometry import GeoScenario, bounds
from test_gpu_map_geometry import MODELS, _score_all_forms

pytestmark = pytest.mark.gpu

FAR = {
    "F1": (151, 62, 0.05, (41234.5678, -1003456.789)),
    "F2": (93, 211, 0.1, (-3.2e6, 2.9e6)),
}


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


_CACHE = {}


def scenario(orc, name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        sx, sy, res, origin = FAR[name]
        sc = GeoScenario(orc, sx, sy, res, origin, **kw)
        assert sc.origin == (np.float32(origin[0]), np.float32(origin[1]))
        _CACHE[key] = sc
    return _CACHE[key]


def test_knife_edge_rate_at_these_origins():
    """2 ulp(|x|) / res per evaluation and axis, as the docstring and DESIGN.md section 2 state it."""
    for name, rate in (("F1", 5.0e-9), ("F2", 1.9e-8)):
        sx, sy, res, origin = FAR[name]
        got = sum(2 * np.spacing(abs(float(np.float32(o)))) / res for o in origin)
        assert 0.9 * rate < got < 1.1 * rate, (name, got)
        assert 1 + int(4097 * 61 * got) == 1  # the existing budget of one knife-edge weight is the expected one


@pytest.mark.parametrize("cloud", ["spread", "mixture"])
@pytest.mark.parametrize("model_name", list(MODELS))
@pytest.mark.parametrize("name", list(FAR))
def test_scoring_on_far_maps_matches_oracle(engine, orc, name, model_name, cloud):
    """The four planar models, beam skipping off and armed, the resident set and both host-buffer forms; the clouds
    reach past every edge and into the walls, so recalcWeight's off-map and non-free-space factors are in the weights."""
    n = 1000 if model_name == "beam" else 4097
    kw = dict(n=n, beams=61, cloud=cloud)
    if model_name == "beam":
        kw["frac_nan"] = 0.0
    sc_ = scenario(orc, name, **kw)
    assert min(sc_.off_map_sides()) > 0
    i, j = sc_.cells_of()
    inside = sc_.in_map()
    assert (sc_.cells[j[inside], i[inside]] != -1).any()  # particles in walls / unknown space
    _score_all_forms(engine, orc, sc_, model_name, 61, (name, model_name, cloud))


@pytest.mark.parametrize("name", list(FAR))
def test_calc_range_on_far_maps_is_exact(engine, orc, name):
    """occupancy_map.cpp:257-364: 2 000 rays from on and off the map, all octants and the exact axis and diagonal
    directions."""
    sc_ = scenario(orc, name, n=257, beams=61, cloud="spread")
    m, sc, pf, data = sc_.gpu_objects(engine, 61, "beam")
    rng = np.random.default_rng(12)
    n = 2000
    x0, x1, y0, y1 = bounds(sc_.size_x, sc_.size_y, sc_.origin, sc_.res)
    ox, oy = rng.uniform(x0 - 1.0, x1 + 1.0, n), rng.uniform(y0 - 1.0, y1 + 1.0, n)
    oa = rng.uniform(-math.pi, math.pi, n)
    oa[:64] = np.repeat(np.arange(-4, 4) * (math.pi / 4), 8)
    mr = rng.choice([0.3, 8.0, 30.0], n)
    got = m.calcRange(ox, oy, oa, mr)
    want = np.array([sc_.omap.calc_range(float(a), float(b), float(c), float(d))
                     for a, b, c, d in zip(ox, oy, oa, mr)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want < mr).mean() > 0.3 and (want == mr).mean() > 0.02


@pytest.mark.parametrize("name", list(FAR))
def test_uniform_pose_generator_on_far_maps_is_exact(engine, orc, name):
    """initWithRandomPoses with the 2-D free-space generator: 5 000 poses, the leaf count and the RNG state, exactly."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = 5000
    sc_ = scenario(orc, name, n=257, beams=61, cloud="spread")
    m, sc, _, data = sc_.gpu_objects(engine, 61, "lf")
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
    pf.srand48(17)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    rng0 = pf.getRngState()
    pf.initWithRandomPoses()
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0)
    opf.pf.rng = rng0
    assert opf.set_random_pose_source(sc_.omap, sc_.map_factors[2]) == len(sc_.free_cells()) > 200
    opf.init_with_free_space_poses()
    got = pf.getCurrentSet().samples
    st = pf.getState()
    assert sc_.in_map(opf.samples[:n]).all()
    assert st.sample_count == n
    assert np.array_equal(got[:, :3], opf.samples[:n, :3])
    assert np.all(got[:, 3] == 1.0 / n)
    assert pf.getRngState() == opf.pf.rng
    assert st.leaf_count == opf.leaf_count
