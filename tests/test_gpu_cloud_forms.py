"""Every instance of the 3-D scoring kernel (k_cloud_score: EXACT_RINV x PLANAR x DENSE, and BORDER in both reciprocal
forms) against the oracle on the worlds of tests/cloud_geometry.py: resolutions whose reciprocal is not exact, dense
volumes of whole tiles, sides narrower than a tile, one z plane and more than 255, positive lower bounds, a map
kilometres from the origin, a plane too large for the dense volume; points and robots placed on voxel faces on
purpose.  Engine.cloud_last_form() says after every launch which instance ran."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cloud_geometry as cg  # noqa: E402
import pose_check_ref as ref  # noqa: E402
from cloud_geometry import F_BORDER, F_DENSE, F_EXACT, F_PLANAR, F_RAN  # noqa: E402
from scenario import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

W_TOL = 1e-9
NAMES = sorted(cg.GEOMETRIES)

# form -> (pitched mounting, BPF_OPT_CLOUD_DENSE, LUT without a free ratio, the instance's bits but EXACT_RINV)
FORMS = {
    "border": (False, 1, False, F_PLANAR | F_DENSE | F_BORDER),
    "planar_dense": (False, 1, True, F_PLANAR | F_DENSE),
    "planar_two_level": (False, 0, False, F_PLANAR),
    "general_dense": (True, 1, False, F_DENSE),
    "general_two_level": (True, 0, False, 0),
}
IDENTITY = {False: (0.0, 0.0, 0.0, 1.0), True: (1e-30, 0.0, 0.0, 1.0)}   # the second selects the general kernel
NO_SHIFT = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def expected_form(s, form):
    return F_RAN | FORMS[form][3] | (F_EXACT if s.exact else 0)


def score(engine, s, form, model, samples, pts, identity=False):
    """One applyModelToSampleSet through `form`: (samples with the new weights, total, the form the engine reports)."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    pitched, dense, full, _ = FORMS[form]
    engine.set_option(hpf.OPT_CLOUD_DENSE, dense)
    try:
        mount = dict(tf_xyz=NO_SHIFT, tf_quat=IDENTITY[pitched]) if identity else {}
        _, sc = s.gpu_scanner(engine, model, pitched, ratios=s.full_ratios() if full else None, **mount)
        got = samples.copy()
        total = sc.applyModelToSampleSet(bpf.PointCloudData(pts), got)
        return got, total, engine.cloud_last_form()
    finally:
        engine.set_option(hpf.OPT_CLOUD_DENSE, 1)


_WANT = {}


def oracle(orc, s, model, pitched):
    """The oracle's weights and total for the scenario's own set and cloud: computed once, left unchanged."""
    key = (s.name, model, pitched)
    if key not in _WANT:
        want = s.samples.copy()
        total = orc.cloud_apply(s.oracle_cloud(model, pitched), s.lut, want, s.pts[pitched])
        want.setflags(write=False)
        _WANT[key] = (want, total)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ a. every form
@pytest.mark.parametrize("model", ["plain", "gompertz"])
@pytest.mark.parametrize("name", NAMES)
def test_every_form_on_every_world_matches_the_oracle(engine, orc, name, model):
    """The same 300 particles and 5000 points through the three planar and the two general instances the world's
    resolution selects; the engine reports the instance that ran."""
    s = cg.scenario(orc, name)
    out = {}
    for form, (pitched, _, _, _) in FORMS.items():
        got, total, ran = score(engine, s, form, model, s.samples, s.pts[pitched])
        assert ran == expected_form(s, form), (name, form, ran)
        want, want_total = oracle(orc, s, model, pitched)
        print(name, model, form, "form", ran, "max rel err", rel_err(got[:, 3], want[:, 3]).max(),
              "total rel err", abs(total - want_total) / want_total)
        assert np.array_equal(got[:, :3], s.samples[:, :3], equal_nan=True)
        bad = rel_err(got[:, 3], want[:, 3]) > W_TOL
        assert bad.sum() <= 1, (name, form, np.flatnonzero(bad))
        assert abs(total - want_total) <= W_TOL * want_total, (name, form)
        out[form] = (got[:, 3].copy(), total)
    # same voxels, same terms, same order: bit-identical among the planar forms and among the general ones
    for a, b in (("border", "planar_dense"), ("border", "planar_two_level"), ("general_dense", "general_two_level")):
        assert np.array_equal(out[a][0], out[b][0]) and out[a][1] == out[b][1], (name, a, b)
    # the scores discriminate: walls, free space, off the map
    assert len(np.unique(np.round(out["border"][0] / s.samples[:, 3], 9))) > 30


def test_the_cases_reach_every_instance(engine, orc):
    """All ten instances score_cloud can launch, walked here: five forms at an exact and at an inexact resolution."""
    seen = set()
    for name in ("V4", "V2"):
        s = cg.scenario(orc, name)
        for form, (pitched, _, _, _) in FORMS.items():
            _, _, ran = score(engine, s, form, "plain", s.samples[:40], s.pts[pitched][:300])
            assert ran == expected_form(s, form)
            seen.add(ran)
    want = {F_RAN | e | p | d | b for e in (0, F_EXACT) for p in (0, F_PLANAR) for d in (0, F_DENSE)
            for b in ((0, F_BORDER) if p and d else (0,))}
    assert seen == want and len(want) == 10


# ------------------------------------------------------------------------------------------------ b. voxel faces
@pytest.mark.parametrize("name", NAMES)
def test_points_on_voxel_faces(engine, orc, name):
    """One particle at (0, 0, 0) under an identity mounting, so that the world point is the input point; points on the
    faces (k + 0.5) res of one axis at a time, -2 .. +2 float ulps, from five cells below the map to five above, the
    other two coordinates where the voxels either side of the face hold different ratios.  No allowance: the kernel's
    quotient forms give the reference's voxel for every float near a face (test_cloud_geometry_cpu.py).  z stands on
    its own: the planar forms make the z voxel at LDS staging, not in the loop."""
    s = cg.scenario(orc, name)
    one = np.array([[0.0, 0.0, 0.0, 1.0]])
    for axis in range(3):
        pts, differs = s.face_cloud(axis)
        assert differs.mean() > 0.1
        want = {}
        for pitched in (False, True):
            # the oracle's voxels are those of the inputs
            w = s.world_points(one, pts, tf_xyz=NO_SHIFT, tf_quat=IDENTITY[pitched])[0]
            assert np.array_equal(cg.voxel_reference(w, s.res), cg.voxel_reference(pts, s.res))
            o = one.copy()
            total = orc.cloud_apply(s.oracle_cloud("plain", tf_xyz=NO_SHIFT, tf_quat=IDENTITY[pitched]), s.lut, o, pts)
            want[pitched] = (o[0, 3], total)
        assert rel_err(want[False][0], want[True][0]) < 1e-12     # the same voxels through either mounting
        for form, (pitched, _, _, _) in FORMS.items():
            got, total, ran = score(engine, s, form, "plain", one, pts, identity=True)
            assert ran == expected_form(s, form), (name, form, ran)
            err = rel_err(got[0, 3], want[pitched][0])
            print(name, "xyz"[axis], form, "form", ran, "weight", got[0, 3], "rel err", float(err))
            assert err <= W_TOL, (name, "xyz"[axis], form, got[0, 3], want[pitched][0])
            assert abs(total - want[pitched][1]) <= W_TOL * want[pitched][1]


# ------------------------------------------------------------------------------------------------ c. the robot's cell
@pytest.mark.parametrize("name", NAMES)
def test_robot_cell_on_a_face(engine, orc, name):
    """k_cloud_finish restates recalcWeight's cell of the robot with true division in double: particles whose x or y
    stands within two double ulps of the faces at min - 1, min, max and max + 1 get the off-map factor exactly where
    the oracle's pose_valid3 gives it."""
    import badger_amcl_amd as bpf
    s = cg.scenario(orc, name)
    r = s.robot_face_samples()
    on = s.robot_on_map(r)
    assert on.any() and (~on).any()
    for form in ("border", "general_dense"):
        pitched = FORMS[form][0]
        got, total, ran = score(engine, s, form, "plain", r, s.pts[pitched])
        assert ran == expected_form(s, form)
        want = r.copy()
        want_total = orc.cloud_apply(s.oracle_cloud("plain", pitched), s.lut, want, s.pts[pitched])
        err = rel_err(got[:, 3] / r[:, 3], want[:, 3] / r[:, 3])
        print(name, form, "max rel err", err.max(), "on the map", int(on.sum()), "off", int((~on).sum()))
        assert (err <= W_TOL).all(), (name, form, np.flatnonzero(err > W_TOL))
        assert abs(total - want_total) <= W_TOL * want_total
        # and the factor by itself: the same launch with an off-map factor of 1
        _, sc = s.gpu_scanner(engine, "plain", pitched)
        sc.setMapFactors(1.0, 0.95, 0.3)
        plain = r.copy()
        sc.applyModelToSampleSet(bpf.PointCloudData(s.pts[pitched]), plain)
        assert np.array_equal(got[:, 3], np.where(on, plain[:, 3], plain[:, 3] * cg.OFF_MAP_FACTOR))


# ------------------------------------------------------------------------------------------------ d. resident path
@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("name", ["V3", "V1"])
def test_resident_update_and_resample(engine, orc, name, resampler):
    """initWithSamples -> updateSensor -> updateResample against the oracle's filter, as
    test_gpu_cloud.py::test_cloud_update_sensor_and_resample, on an inexact resolution far from the origin (V3) and on
    the whole-tile map (V1), for both resamplers."""
    import badger_amcl_amd as bpf
    s = cg.scenario(orc, name)
    n = 2000
    samples = s.converged_samples(n)
    pts = s.pts[False]
    _, sc = s.gpu_scanner(engine, "plain", False)
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
    pf.srand48(5)
    pf.setResampleModel(resampler)
    pf.initWithSamples(samples)
    assert sc.updateSensor(pf, bpf.PointCloudData(pts))
    assert engine.cloud_last_form() == expected_form(s, "border")
    cur = pf.getCurrentSet()
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0, seed=5)
    opf.set_resample_model(resampler)
    opf.set_samples(samples)
    op = s.oracle_cloud("plain", False)
    opf.update_sensor(lambda smp, conv: orc.cloud_apply(op, s.lut, smp, pts))
    assert np.array_equal(cur.samples[:, :3], samples[:, :3])
    assert (rel_err(cur.samples[:, 3], opf.samples[:n, 3]) > W_TOL).sum() <= 1
    assert len(np.unique(np.round(opf.samples[:n, 3] / samples[:, 3], 6))) > 30
    pf.updateResample()
    out = opf.update_resample()
    st = pf.getState()
    assert st.sample_count == out.sample_count and st.leaf_count == out.leaf_count
    assert np.array_equal(pf.getCurrentSet().samples[:, :3], opf.samples[:out.sample_count, :3])


# ------------------------------------------------------------------------------------------------ e. builder -> scoring
def test_lut_built_on_the_engine_scores_without_being_set_again(engine, orc):
    """The path a node takes: updateDistancesLUT builds the two-level LUT on the device and hands it to bpf_map3d_set,
    which lays out the dense copy; scoring follows with no setDistancesLUT in between."""
    import badger_amcl_amd as bpf
    s = cg.scenario(orc, "V2")
    out = {}
    for built in (True, False):
        for form in ("border", "general_dense"):
            pitched = FORMS[form][0]
            om, sc = s.gpu_scanner(engine, "plain", pitched, set_lut=not built)
            if built:
                om.updateDistancesLUT(s.occ, s.mn, s.mx, s.max_dist)
                pi, dr = om.getDistancesLUT()
                assert np.array_equal(pi, s.lut.pose_indices) and np.array_equal(dr, s.lut.distance_ratios)
            got = s.samples.copy()
            total = sc.applyModelToSampleSet(bpf.PointCloudData(s.pts[pitched]), got)
            assert engine.cloud_last_form() == expected_form(s, form)
            out[built, form] = (got[:, 3].copy(), total)
    for form in ("border", "general_dense"):
        assert np.array_equal(out[True, form][0], out[False, form][0]) and out[True, form][1] == out[False, form][1]
        want, want_total = oracle(orc, s, "plain", FORMS[form][0])
        assert (rel_err(out[True, form][0], want[:, 3]) > W_TOL).sum() <= 1
        assert abs(out[True, form][1] - want_total) <= W_TOL * want_total


# ------------------------------------------------------------------------------------------------ f. no dense volume
def test_map_whose_plane_does_not_fit_the_dense_volume(engine, orc):
    """4100 x 4100 x 1 cells: 513 x 513 tiles of 64 bytes are more than 2^24, so bpf_map3d_set keeps the two-level
    layout alone and the kernel takes it with BPF_OPT_CLOUD_DENSE at its default.  The LUT is written by hand (no
    brushfire on 16.8 M columns): every column the shared all-255 one, but a 40 x 40 patch of one-byte columns."""
    import badger_amcl_amd as bpf
    res, max_dist, side = 0.05, 0.3, 4100
    mn = np.array([-1000, 200, 3], dtype=np.int32)
    mx = mn + np.array([side - 1, side - 1, 0], dtype=np.int32)
    ntx = (side + 2 + 7) // 8
    assert ntx * ntx * 64 >= 1 << 24 and side * side < 1 << 30
    rng = np.random.default_rng(12)
    i0, j0, k = 3000, 517, 40
    pi = np.zeros(side * side, dtype=np.uint32)
    jj, ii = np.mgrid[0:k, 0:k]
    pi[(j0 + jj) * side + i0 + ii] = 1 + jj * k + ii
    dr = np.concatenate([[255], rng.integers(0, 250, k * k)]).astype(np.uint8)
    lut = orc.OctoMapLUT(mn, mx, res, max_dist, pi, dr)
    centre = np.array([(mn[0] + i0 + k / 2) * res, (mn[1] + j0 + k / 2) * res])
    n, n_points = 50, 300
    s = np.zeros((n, 4))
    s[:, :2] = centre + rng.normal(0.0, 0.5, (n, 2))
    s[:, 2] = -rng.uniform(-np.pi, np.pi, n)
    s[:, 3] = rng.uniform(0.5, 1.5, n) / n
    s[:3, 0] += 300.0                        # three particles off the map
    pts = np.zeros((n_points, 3), dtype=np.float32)
    pts[:, :2] = rng.uniform(-1.5, 1.5, (n_points, 2))
    pts[:, 2] = mn[2] * res - cg.TF_XYZ[2] + rng.normal(0.0, 0.4 * res, n_points)   # the one plane, and off it
    a = cg.MOUNT_ANGLE
    quats = {False: (0.0, 0.0, np.sin(a / 2), np.cos(a / 2)), True: (0.01, -0.008, np.sin(a / 2), np.cos(a / 2))}
    om = bpf.OctoMap(engine, res)
    om.setDistancesLUT(pi, dr, mn, mx, max_dist)
    sc = bpf.PointCloudScanner(engine)
    sc.init(128, om)
    sc.setPointCloudModel(0.5, 0.05, 0.1)
    sc.setMapFactors(0.95, 0.95, 0.3)
    for pitched, quat in quats.items():
        sc.setPointCloudScannerToFootprintTF(cg.TF_XYZ, quat)
        got = s.copy()
        total = sc.applyModelToSampleSet(bpf.PointCloudData(pts), got)
        assert engine.cloud_last_form() == F_RAN | F_EXACT | (0 if pitched else F_PLANAR)   # DENSE clear
        op = orc.cloud(orc.CLOUD_MODEL, 128, cg.TF_XYZ, quat, z_hit=0.5, z_rand=0.05, sigma_hit=0.1)
        op.off_map_factor = 0.95
        want = s.copy()
        want_total = orc.cloud_apply(op, lut, want, pts)
        err = rel_err(got[:, 3], want[:, 3])
        print("pitched", pitched, "max rel err", err.max(), "distinct scores",
              len(np.unique(np.round(want[:, 3] / s[:, 3], 9))))
        assert np.array_equal(got[:, :3], s[:, :3])
        assert (err <= W_TOL).all(), np.flatnonzero(err > W_TOL)
        assert abs(total - want_total) <= W_TOL * want_total
        assert len(np.unique(np.round(want[:, 3] / s[:, 3], 9))) > 30    # the patch is seen


# ------------------------------------------------------------------------------------------------ g. free space, far out
@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("g0,m", [(0.0, 0.5), (10.0, 0.5)])
def test_free_space_3d_poses_far_from_the_origin(orc, resampler, g0, m):
    """RANDOM_POSE_FREE_SPACE_3D on V3 (columns 20000.. / -30050.., 0.07 m): initWithRandomPoses, then recovery
    resamples after point-cloud updates, K = 0 retries and K = 4, as test_gpu_pose_check.py::
    test_free_space_3d_generator does on the room at 0.05 m."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_pose_check import ALPHA, _check_init, _check_resample
    s = cg.scenario(orc, "V3")
    e = bpf.Engine(0)  # an engine that never saw a 2-D map
    try:
        n = 1000
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        _, sc = s.gpu_scanner(e, "plain", False)
        fs = ref.FreeSpace.octo([int(v) for v in s.mn], [int(v) for v in s.mx], s.res)
        pf = bpf.ParticleFilter(e, 100, n, ALPHA[0], ALPHA[1], 85.0)
        pf.srand48(11)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.setUniformPoseCheck(g0, m)
        assert ref.retries(g0, m) == (0 if g0 == 0.0 else 4)
        _check_init(orc, pf, fs, g0, m, n)
        drawn = pf.getCurrentSet().samples
        assert s.robot_on_map(drawn).all() and drawn[:, 0].min() > 1399.0 and drawn[:, 1].max() < -2099.0
        pf.initWithSamples(s.converged_samples(n))
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=11)
        w_diffs = []
        pts = s.pts[False]
        for scan in (pts, pts * np.float32(0.5), pts * np.float32(0.3)):
            assert sc.updateSensor(pf, bpf.PointCloudData(np.ascontiguousarray(scan)))
            assert e.cloud_last_form() == expected_form(s, "border")
            w_diffs.append(_check_resample(orc, pf, opf, fs, g0, m, resampler))
        assert max(w_diffs) > 0.01
    finally:
        e.close()
