"""The scan's end points formed by the scoring's prep launch (default) against the host's (BPF_OPT_STAGE_ON_HOST = 1):
the same weights and the same total, bit for bit, after updateSensor -- for scans that take the device path, for scans
that fall back to the host's staging, and across changes of the bearings (the device copy of their cosines and sines
follows the host's cache)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
SIZE = 400
BEAMS = 181
RANGE_MAX = 30.0
MAX_DIST = 2.0


@pytest.fixture(scope="module")
def world():
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    e = bpf.Engine(0)
    cells, origin = synth.make_map(SIZE, 0.05)
    m = bpf.OccupancyMap(e, 0.05)
    m.setCells(cells)
    m.setOrigin(origin)
    m.updateDistancesLUT(MAX_DIST)
    pose = synth.true_pose(SIZE, 0.05)
    ranges, angles = synth.cast_scan(cells, origin, 0.05, pose, BEAMS, range_max=RANGE_MAX, seed=5, frac_max=0.0,
                                     frac_nan=0.0)
    samples = synth.converged_cloud(N, pose, seed=17)
    samples[:, 3] *= np.random.default_rng(4).uniform(0.5, 1.5, N)
    yield dict(engine=e, map=m, ranges=np.minimum(ranges, 25.0), angles=angles, samples=samples)
    e.close()


def _scans(w):
    """(name, ranges, angles, range_max) in the order they are run on ONE engine.  Every planted beam sits at a multiple
    of 6, the decimation step of 181 beams at max_beams = 30, so that both decimations keep it."""
    base, ang_a = w["ranges"].copy(), w["angles"].copy()
    # one beam at each of the four cardinal bearings
    for i, a in ((6, 0.0), (12, np.pi / 2), (18, np.pi), (24, -np.pi / 2)):
        ang_a[i] = a
    usual = base.copy()
    for i, r in ((36, 0.0), (48, -0.0), (60, -1.5), (72, 5e-324), (84, 1e-300), (96, np.nextafter(RANGE_MAX, 0.0))):
        usual[i] = r
    assert (usual < RANGE_MAX).all()                                  # the device path takes it
    with_nan = usual.copy()
    with_nan[108] = np.nan
    at_max = usual.copy()
    at_max[120] = RANGE_MAX
    huge = usual.copy()
    huge[132] = 1e12                                                  # < range_max = 1e13, but 2e13 cells long
    assert huge[132] / 0.05 >= 268435456.0
    ang_b = ang_a * 0.75 + 0.1                                        # other bearings, same count
    return [("usual", usual, ang_a, RANGE_MAX),
            ("nan", with_nan, ang_a, RANGE_MAX),
            ("range_max", at_max, ang_a, RANGE_MAX),
            ("huge", huge, ang_a, 1e13),
            ("usual again", usual, ang_a, RANGE_MAX),
            ("other bearings", usual, ang_b, RANGE_MAX),
            ("first bearings, fresh buffer", usual, ang_a.copy(), RANGE_MAX)]


def _run(w, model, max_beams, on_host):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd import synth
    e = w["engine"]
    e.set_option(hpf.OPT_STAGE_ON_HOST, on_host)
    try:
        sc = bpf.PlanarScanner(e)
        sc.init(max_beams, w["map"])
        if model == "lf":
            p = synth.LF_DEFAULTS
            sc.setModelLikelihoodField(p["z_hit"], p["z_rand"], p["sigma_hit"], MAX_DIST)
        else:
            p = synth.GOMPERTZ_LAUNCH
            sc.setModelLikelihoodFieldGompertz(p["z_hit"], p["z_rand"], p["sigma_hit"], MAX_DIST, p["gompertz_a"],
                                               p["gompertz_b"], p["gompertz_c"], p["input_shift"], p["input_scale"],
                                               p["output_shift"])
        sc.setMapFactors(*synth.MAP_FACTORS)
        sc.setPlanarScannerPose((0.1, -0.05, 0.2))
        pf = bpf.ParticleFilter(e, 10, N, 0.001, 0.1, 85.0)
        out = []
        for name, ranges, angles, range_max in _scans(w):
            pf.initWithSamples(w["samples"])
            assert sc.updateSensor(pf, bpf.PlanarData(ranges, angles, range_max))
            st = pf.getState()
            out.append((name, pf.getCurrentSet().samples[:, 3].copy(), st.total, st.evals))
        return out
    finally:
        e.set_option(hpf.OPT_STAGE_ON_HOST, 0)


@pytest.mark.parametrize("max_beams", [BEAMS, 30])   # decimation step 1 and step 6
@pytest.mark.parametrize("model", ["lf", "gompertz"])
def test_device_staging_equals_host_staging(world, model, max_beams):
    dev = _run(world, model, max_beams, 0)
    host = _run(world, model, max_beams, 1)
    for (name, w_dev, t_dev, ev_dev), (_, w_host, t_host, ev_host) in zip(dev, host):
        assert np.isfinite(w_host).all() and w_host.max() > 0.0, name
        assert np.array_equal(w_dev, w_host), name
        assert t_dev == t_host, name
        assert ev_dev == ev_host, name
    by = {name: (w, t) for name, w, t, _ in dev}
    # the scans differ where they should: a stale table of cosines would make "other bearings" a repeat of "usual"
    assert not np.array_equal(by["other bearings"][0], by["usual"][0])
    assert np.array_equal(by["first bearings, fresh buffer"][0], by["usual"][0])
    assert np.array_equal(by["usual again"][0], by["usual"][0])
    assert by["first bearings, fresh buffer"][1] == by["usual"][1]
