"""Planar scoring and pose generation on rectangular, off-centre maps (tests/map_geometry.py) against the oracle.
Every other 2-D map of this suite is square with its origin at the node's centre formula; there a swapped x / y pair
in the engine -- size_x for size_y in a bounds test or a clamp, tx for ty in the tile addressing, half_x for half_y in
a conversion -- gives the same results.  Here it does not: the maps are 333 x 150, 93 x 211, 151 x 62 and 5 x 12
cells (and 1701 x 1003 with its transpose for the tile-sorted form), the wall lattice has another period on each
axis, origins are negative or no multiple of the cell, and the clouds reach past all four edges.  Each test on a wide
or tall map first asserts that at least a fifth of its in-map particles lie where a transposed engine would see
nothing.

Weights: 1e-9 relative with the knife-edge budget of test_gpu_parity.py; poses, counts and RNG state exact; totals
1e-9 relative."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_check_ref as ref  # noqa: E402
from map_geometry import GeoScenario  # noqa: E402
from scenario import rel_err  # noqa: E402
from test_gpu_parity import W_TOL, _knife_edge_budget  # noqa: E402

pytestmark = pytest.mark.gpu

BEAMSKIP = dict(do_beamskip=1, beam_skip_distance=0.5, beam_skip_threshold=0.3, beam_skip_error_threshold=0.9)
# name -> (model, model parameters, set_converged of the host-buffer forms)
MODELS = {
    "lf": ("lf", None, 0),
    "gompertz": ("gompertz", None, 0),
    "prob": ("prob", None, 0),
    "prob_skip": ("prob", BEAMSKIP, 1),   # beam skipping armed: the COUNT_ONLY pass runs first
    "beam": ("beam", None, 0),
}
IN_PLACE = -1  # seam_last_plan: one launch read and wrote the registered records (HOST_MODE 2 of k_score_field)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


_CACHE = {}


def scenario(orc, name, **kw):
    """One GeoScenario per argument set for the whole module; the tests copy what they change."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = GeoScenario.named(orc, name, **kw)
    return _CACHE[key]


def check_weights(got, want, n_evals, what):
    bad = rel_err(got, want) > W_TOL
    assert bad.sum() <= _knife_edge_budget(n_evals), (what, int(bad.sum()), np.flatnonzero(bad)[:10])


def check_total(total, want_total, what):
    assert abs(total - want_total) <= 1e-9 * abs(want_total), (what, total, want_total)


# ---------------------------------------------------------------------------------------------- a. scoring matrix
def _armed_beamskip(sc_, max_beams):
    """Beam-skip parameters under which skipping changes this scenario's weights.  Which beams are skipped depends on
    the share of particles that agree with each beam, so one threshold does not serve every map and cloud: below it
    no beam is skipped, above it too many are and the reference falls back to all beams (or to weight zero); either way
    the counts of the COUNT_ONLY pass would not show in the result.  The first threshold of a fixed ladder at which the
    oracle's weights with skipping armed differ from those without, with a positive total, is taken."""
    plain = sc_.samples.copy()
    sc_.oracle_apply(sc_.oracle_planar(max_beams, "prob", dict(BEAMSKIP)), plain, 0)
    for thr in (0.3, 0.4, 0.5, 0.6, 0.7, 0.8):
        kw = dict(BEAMSKIP, beam_skip_threshold=thr)
        w = sc_.samples.copy()
        total = sc_.oracle_apply(sc_.oracle_planar(max_beams, "prob", kw), w, 1)
        if total > 0.0 and not np.array_equal(w[:, 3], plain[:, 3]):
            return kw
    raise AssertionError("no threshold of the ladder arms beam skipping on this scenario")


def _score_all_forms(engine, orc, sc_, model_name, beams, what):
    """The oracle once, then the three forms: the resident set (updateSensor), applyModelToSampleSet on a pageable
    buffer and on a registered one.  Returns the forms the engine reported."""
    model, kw, conv = MODELS[model_name]
    n = sc_.samples.shape[0]
    max_beams = beams
    if kw is not None:
        kw = _armed_beamskip(sc_, max_beams)
    p = sc_.oracle_planar(max_beams, model, kw)
    want = sc_.samples.copy()
    want_total = sc_.oracle_apply(p, want, conv)
    assert np.isfinite(want_total) and want_total > 0.0 and want[:, 3].std() > 0.0
    m, sc, pf, data = sc_.gpu_objects(engine, max_beams, model, model_kw=kw)
    forms = {}
    # resident: the set's own flag decides whether beam skipping is armed (a set that was just adopted is not
    # converged); the host-buffer forms below are told
    res_conv = pf.getState().converged
    assert sc.updateSensor(pf, data) is True
    st = pf.getState()
    if res_conv == conv:
        res_want, res_total = want, want_total
    else:
        res_want = sc_.samples.copy()
        res_total = sc_.oracle_apply(p, res_want, res_conv)
    cur = pf.getCurrentSet().samples
    assert np.array_equal(cur[:, :3], sc_.samples[:, :3])
    check_weights(cur[:, 3], res_want[:, 3] / res_total, n * max_beams, what + ("resident",))
    check_total(st.total, res_total, what + ("resident",))
    forms["resident"] = engine.score_last_form()
    # pageable
    got = sc_.samples.copy()
    total = sc.applyModelToSampleSet(data, got, conv)
    forms["pageable"] = engine.seam_last_plan()
    assert forms["pageable"][1] is False
    assert np.array_equal(got[:, :3], want[:, :3])
    check_weights(got[:, 3], want[:, 3], n * max_beams, what + ("pageable",))
    check_total(total, want_total, what + ("pageable",))
    # registered
    got = sc_.samples.copy()
    engine.registerHostBuffer(got)
    try:
        total = sc.applyModelToSampleSet(data, got, conv)
        forms["registered"] = engine.seam_last_plan()
    finally:
        engine.unregisterHostBuffer(got)
    assert forms["registered"][1] is True
    if n >= 4096 and model != "beam" and conv == 0:
        assert forms["registered"][0] == IN_PLACE
    assert np.array_equal(got[:, :3], want[:, :3])
    check_weights(got[:, 3], want[:, 3], n * max_beams, what + ("registered",))
    check_total(total, want_total, what + ("registered",))
    return forms


@pytest.mark.parametrize("cloud", ["spread", "mixture"])
@pytest.mark.parametrize("model_name", list(MODELS))
@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G4"])
def test_scoring_on_rectangular_maps_matches_oracle(engine, orc, name, model_name, cloud):
    """4097 particles (1000 for the beam model) x 61 beams, every model, the resident set and both host-buffer forms."""
    n = 1000 if model_name == "beam" else 4097   # 4097: past the 4096 from which a registered buffer is scored in place
    kw = dict(n=n, beams=61, cloud=cloud)
    if model_name == "beam":
        kw["frac_nan"] = 0.0                      # the beam model does not skip NaN ranges: NaN in, NaN out
    sc_ = scenario(orc, name, **kw)
    sc_.assert_geometry_is_seen()
    forms = _score_all_forms(engine, orc, sc_, model_name, 61, (name, model_name, cloud))
    print("forms on %s %s %s: %s" % (name, model_name, cloud, forms))


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_scoring_a_long_scan_on_rectangular_maps_matches_oracle(engine, orc, name):
    """193 beams: three chunks of 64 and one beam over."""
    sc_ = scenario(orc, name, n=4097, beams=193, cloud="spread")
    sc_.assert_geometry_is_seen()
    _score_all_forms(engine, orc, sc_, "lf", 193, (name, "lf", 193))


# ---------------------------------------------------------------------------------------------- b. the engine's LUT
@pytest.mark.parametrize("builder", ["reference", "exact"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_lut_built_by_the_engine_on_a_rectangle_then_scored(engine, orc, name, builder):
    """updateDistancesLUT (the reference's brushfire order) and updateDistancesLUTExact leave the tiled image that
    scoring reads; the float LUT read back and handed to the oracle must give the weights that image gives."""
    import badger_amcl_amd as bpf
    n, beams = 4097, 61
    sc_ = scenario(orc, name, n=n, beams=beams, cloud="spread")
    sc_.assert_geometry_is_seen()
    m = bpf.OccupancyMap(engine, sc_.res)
    m.setCells(sc_.cells)
    m.setOrigin(sc_.origin)
    if builder == "reference":
        m.updateDistancesLUT(sc_.max_dist)
    else:
        m.updateDistancesLUTExact(sc_.max_dist)
    lut = m.getDistancesLUT()
    assert lut.shape == (sc_.size_y, sc_.size_x)
    if builder == "reference":
        assert np.array_equal(lut, sc_.lut)
    else:
        # the exact transform is never above the brushfire and differs from it in few cells (pf.py)
        assert np.all(lut <= sc_.lut) and np.mean(lut == sc_.lut) > 0.9
    sc = bpf.PlanarScanner(engine)
    sc.init(beams, m)
    sc_.configure_gpu_model(sc, "lf")
    sc.setMapFactors(*sc_.map_factors)
    sc.setPlanarScannerPose(sc_.scanner_pose)
    data = bpf.PlanarData(sc_.ranges, sc_.angles, sc_.range_max)
    got = sc_.samples.copy()
    total = sc.applyModelToSampleSet(data, got, 0)
    omap = orc.OccupancyMap(sc_.cells, sc_.res, sc_.origin, sc_.max_dist, lut=lut)
    want = sc_.samples.copy()
    want_total = orc.planar_apply(sc_.oracle_planar(beams, "lf"), omap, want, sc_.ranges, sc_.angles, sc_.range_max, 0)
    check_weights(got[:, 3], want[:, 3], n * beams, (name, builder))
    check_total(total, want_total, (name, builder))


# ---------------------------------------------------------------------------------------------- c. tile-sorted form
N_TILE = 100000


def _tile_world(orc, name):
    """The scenario of a geometry, built once (spread cloud with a 0.5 m margin)."""
    key = ("tile", name)
    if key not in _CACHE:
        sc_ = GeoScenario.named(orc, name, n=N_TILE, beams=61, cloud="spread", margin=0.5)
        _CACHE[key] = sc_
    return _CACHE[key]


def _oracle_normalised(orc, sc_, samples, beams=61):
    """The oracle's updateSensor of the likelihood-field model: (normalised weights, total)."""
    n = samples.shape[0]
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0)
    opf.set_samples(samples, leaf_count=1)
    p = sc_.oracle_planar(beams, "lf")
    total = opf.update_sensor(lambda s, conv: sc_.oracle_apply(p, s, conv))
    return opf.samples[:n, 3].copy(), total


@pytest.mark.parametrize("name,entry", [("L1", "resample"), ("L1", "init"), ("L2", "resample"), ("L2", "init")])
def test_tile_sorted_scoring_on_rectangular_maps_matches_oracle(engine, orc, name, entry):
    """HOST_MODE 3 of k_score_field (the particles walked in map-tile order) on a 1701 x 1003 map and then, on the
    same engine, on its transpose: the tile histogram the engine keeps between updates sees txc / tyc change.  The
    form is entered once by a resample that ran to the end followed by a re-initialisation (as
    test_tile_sorted_scoring_of_a_spread_cloud_gives_the_same_weights enters it) and once by initWithRandomPoses with
    the 2-D free-space generator, whose 100 000 poses and RNG state are compared with the oracle's exactly.  The
    normalised weights against the oracle, and against OPT_TILE_SORT = 0 within 1e-14."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = N_TILE
    sc_ = _tile_world(orc, name)
    sx, sy = sc_.size_x, sc_.size_y
    assert ((sx + 2 + 7) // 8) * ((sy + 2 + 7) // 8) * 128 > (3 << 20)  # the image does not fit an XCD's L2
    m, sc, _, data = sc_.gpu_objects(engine, 61, "lf")
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)  # a new filter: nothing says "spread" yet
    pf.srand48(5)
    if entry == "resample":
        samples = sc_.samples
        sc_.assert_geometry_is_seen(samples)
        pf.initWithSamples(samples)
        sc.updateSensor(pf, data)
        assert engine.score_last_form() == 0
        pf.updateResample()                  # runs to the end: no KLD stop for a spread cloud
        assert pf.getState().sample_count == n
        pf.srand48(5)
        pf.initWithSamples(samples)
    else:
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        rng0 = pf.getRngState()
        pf.initWithRandomPoses()
        opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0)
        opf.pf.rng = rng0
        n_free = opf.set_random_pose_source(sc_.omap, sc_.map_factors[2])
        assert n_free > 100000
        opf.init_with_free_space_poses()
        cur = pf.getCurrentSet().samples
        st = pf.getState()
        assert np.array_equal(cur[:, :3], opf.samples[:n, :3])
        assert np.all(cur[:, 3] == 1.0 / n)
        assert pf.getRngState() == opf.pf.rng
        assert st.leaf_count == opf.leaf_count
        samples = cur.copy()
        sc_.assert_geometry_is_seen(samples, sides=False)  # free-space poses: all of them inside the map
        assert sc_.in_map(samples).all()
    sc.updateSensor(pf, data)
    assert engine.score_last_form() == 3
    w = pf.getCurrentSet().samples[:, 3].copy()
    total = pf.getState().total
    want, want_total = _oracle_normalised(orc, sc_, samples)
    check_weights(w, want, n * 61, (name, entry))
    check_total(total, want_total, (name, entry))
    assert abs(w.sum() - 1.0) < 1e-12
    engine.set_option(hpf.OPT_TILE_SORT, 0)
    try:
        pf.initWithSamples(samples)
        sc.updateSensor(pf, data)
        assert engine.score_last_form() == 0
        w0 = pf.getCurrentSet().samples[:, 3].copy()
        total0 = pf.getState().total
    finally:
        engine.set_option(hpf.OPT_TILE_SORT, 1)
    assert abs(total - total0) <= 1e-13 * abs(total0)
    assert np.max(np.abs(w - w0) / w0) <= 1e-14


# ---------------------------------------------------------------------------------------------- d. window path
# (size_x, size_y, pose cell): the cloud next to the +x edge of the wide map, next to the +y edge of the tall one
WINDOW_CASES = {"wide": (413, 251, (409, 125)), "tall": (251, 413, (125, 409))}


@pytest.mark.parametrize("shape", ["wide", "tall"])
def test_lds_window_path_at_the_edge_of_a_rectangular_map(engine, orc, shape):
    """BPF_OPT_WINDOW_PATH on a 413 x 251 map and on a 251 x 413 one, the cloud three cells (its own 3 sigma) inside
    the +x / +y border: the windows are clipped at the padded image's last row or column (max_u / max_v of
    k_field_windows) and hold the border cells and the spare tile column.  Cloud and scan as in
    test_lds_window_scoring_path_matches_oracle: 16 384 particles, sigma 0.05 / 0.05 / 0.01, 1081 beams, range_max 8.
    The device-side switch took the windows at these positions as first tried; nothing was moved inward."""
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd import synth
    sx, sy, cell = WINDOW_CASES[shape]
    n, beams = 16384, 1081
    key = ("window", shape)
    if key not in _CACHE:
        _CACHE[key] = GeoScenario(orc, sx, sy, 0.05, (-7.3, 11.9), beams=beams, n=n, cloud="converged", frac_nan=0.0,
                                  range_max=8.0, pose_cell=cell)
    sc_ = _CACHE[key]
    samples = synth.converged_cloud(n, sc_.pose, seed=77, sigma=(0.05, 0.05, 0.01))
    samples[:, 3] *= np.random.default_rng(78).uniform(0.5, 1.5, n)
    sc_.samples = samples
    # the input is what the test is about: all of it beyond the other axis' size, and it reaches the last cells
    i, j = sc_.cells_of(samples)
    assert sc_.transposed_blind_fraction(samples) >= 0.2
    edge = (i >= sx - 2) if shape == "wide" else (j >= sy - 2)
    assert 0.001 < edge.mean() < 0.5
    engine.set_option(hpf.OPT_WINDOW_PATH, 1)
    try:
        m, sc, pf, data = sc_.gpu_objects(engine, beams, "lf")
        sc.updateSensor(pf, data)
        got = pf.getCurrentSet().samples
        plan = engine.window_plan()
    finally:
        engine.set_option(hpf.OPT_WINDOW_PATH, 0)
    want, _ = _oracle_normalised(orc, sc_, samples, beams)
    check_weights(got[:, 3], want, n * beams, shape)
    assert plan["chunks_total"] == 17 and plan["used_window"], plan


# ---------------------------------------------------------------------------------------------- e. random poses
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_random_free_space_poses_on_rectangular_maps_match_oracle(engine, orc, name):
    """initWithRandomPoses with the 2-D free-space generator (the list i outer, j inner; size_x / 2 and size_y / 2 in
    the conversion back to the world): 5000 poses, the leaf count and the RNG state, exactly."""
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
    assert opf.set_random_pose_source(sc_.omap, sc_.map_factors[2]) == len(sc_.free_cells()) > 500
    opf.init_with_free_space_poses()
    got = pf.getCurrentSet().samples
    st = pf.getState()
    assert sc_.transposed_blind_fraction(opf.samples[:n]) >= 0.2 and sc_.in_map(opf.samples[:n]).all()
    assert st.sample_count == n
    assert np.array_equal(got[:, :3], opf.samples[:n, :3])
    assert np.all(got[:, 3] == 1.0 / n)
    assert pf.getRngState() == opf.pf.rng
    assert st.leaf_count == opf.leaf_count


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("n,device_kld", [(2500, False), (6000, True)])
def test_recovery_random_poses_on_a_rectangular_map_match_oracle(engine, orc, resampler, n, device_kld):
    """test_gpu_parity.py::test_recovery_random_poses_match_oracle on G1 (333 x 150): w_diff > 0, the random poses
    from the rectangle's free-space list interleaved with the CDF draws, with the host's ordered replay and with the
    device-side histogram tree."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    sc_ = scenario(orc, "G1", n=n, beams=61, cloud="mixture")
    sc_.assert_geometry_is_seen()
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 1 if device_kld else 8192)
    try:
        # alpha_fast 0.5: with 0.1 the second scan moves w_fast by less than a hundredth of w_slow on this map
        m, sc, pf, data = sc_.gpu_objects(engine, 61, "lf", min_samples=100, seed=31, alpha=(0.001, 0.5))
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        opf = orc.ParticleFilter(100, n, 0.001, 0.5, 85.0, seed=31)
        opf.set_resample_model(resampler)
        opf.set_samples(sc_.samples)
        assert opf.set_random_pose_source(sc_.omap, sc_.map_factors[2]) > 1000
        scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0)]
        w_diffs, forms, n_random = [], [], 0
        for cycle, ranges in enumerate(scans):
            sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
            cur = pf.getCurrentSet()
            st0 = pf.getState()
            opf.set_samples(cur.samples, leaf_count=st0.leaf_count)
            opf.pf.w_slow, opf.pf.w_fast = st0.w_slow, st0.w_fast
            opf.pf.rng = pf.getRngState()
            pf.updateResample()
            out = opf.update_resample()
            st1 = pf.getState()
            w_diffs.append(out.w_diff)
            forms.append(st1.kld_on_device)
            assert out.status == 0, cycle
            assert abs(st1.w_diff - out.w_diff) <= 1e-12
            assert st1.sample_count == out.sample_count, (cycle, out.w_diff)
            assert st1.leaf_count == out.leaf_count and st1.bin_count == out.node_count
            M = out.sample_count
            after = pf.getCurrentSet().samples
            assert np.array_equal(after[:, :3], opf.samples[:M, :3])
            assert np.all(after[:, 3] == 1.0 / M)
            assert pf.getRngState() == opf.pf.rng
            if out.w_diff > 0:
                assert st1.w_slow == 0.0 and st1.w_fast == 0.0
                rnd = opf.last_idx < 0
                n_random += int(rnd.sum())
                # the random poses themselves lie where a transposed free-space list has nothing
                assert sc_.transposed_blind_fraction(opf.samples[:M][rnd]) >= 0.2
        assert max(w_diffs) > 0.01 and n_random > 0
        print("kld_on_device per cycle (n %d, device tree %s, resampler %d): %s" % (n, device_kld, resampler, forms))
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
        engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 8192)


# ---------------------------------------------------------------------------------------------- f. score-guided check
def test_score_guided_pose_check_on_a_tall_map(engine, orc):
    """BPF_POSE_CHECK_SENSOR_MODEL on G2 (93 x 211, origin (-3, 1.5), 0.1 m cells), as
    test_gpu_pose_check.py::test_sensor_model_matches_oracle_scores: the trial poses come from the rectangle's
    free-space list and are scored against the last scan; init, then recovery resamples."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_pose_check import ALPHA, _OracleScore, _check_resample, _no_knife_edges, _sensor_gen
    n, beams, resampler = 256, 61, 0
    sc_ = scenario(orc, "G2", n=n, beams=beams, cloud="mixture", frac_nan=0.0)
    sc_.assert_geometry_is_seen()
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    try:
        m_, sc, pf, data = sc_.gpu_objects(engine, beams, "lf", min_samples=100, seed=29, alpha=ALPHA)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        fs = sc_.free_space(ref)
        scorer = _OracleScore(orc, sc_, "lf", beams)
        probe = ref.Rng(12345)
        scorer.ranges = sc_.ranges
        sample = sorted(scorer(fs.pose(probe)) for _ in range(200))
        g0, mult = max(sample[180], 1e-300), 0.5
        assert np.isfinite(g0)
        pf.setUniformPoseCheck(g0, mult, hpf.POSE_CHECK_SENSOR_MODEL)
        sc.updateSensor(pf, data)  # the scan scorePose uses
        rng0 = pf.getRngState()
        pf.initWithRandomPoses()
        r = ref.Rng(rng0)
        want = np.array(ref.init_with_pose_fn(r, n, _sensor_gen(fs, g0, mult, scorer)))
        assert np.array_equal(pf.getCurrentSet().samples[:, :3], want)
        assert pf.getRngState() == r.s
        assert len(scorer.seen) > n  # some trials were rejected
        want4 = np.concatenate([want, np.ones((n, 1))], axis=1)
        assert sc_.transposed_blind_fraction(want4) >= 0.2
        pf.initWithSamples(sc_.samples)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=29)
        scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(beams, 1.0)]
        w_diffs = []
        for ranges in scans:
            sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
            scorer.ranges = ranges
            w_diffs.append(_check_resample(orc, pf, opf, fs, g0, mult, resampler,
                                           gen=_sensor_gen(fs, g0, mult, scorer)))
        assert max(w_diffs) > 0.0
        _no_knife_edges(scorer.seen)
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
