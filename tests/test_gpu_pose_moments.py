"""Pose moments on the device (bpf_planar_pose_moments, bpf_cloud_pose_moments) against the numpy model
(pose_moments_ref.py) evaluated on the call's own scores (byte for byte), against what a one-level refinement implies
(bit for bit), against the oracle's scores and the moments formed from them (within the bound derived below), the
seam's scores (cloud form, bit for bit); invalid and flat rows, a filter left as it was, the refusals, and the chain
search -> refine -> moments -> seed -> track.

Bound against the oracle: the device's scores are within 1e-9 relative of the oracle's (the project's figure for this
scoring path).  w is continuous in s with slope at most 1 + baseline (s_max moves too), so with
delta = 4e-9 * M * s_max / W -- at most 4e-9 * M / (1 - baseline) -- the mean offsets agree within delta * radius and
the covariance entries, in offset units, within 3 * delta * radius_u * radius_v."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mixture_oracle as mo  # noqa: E402
import pose_moments_ref as pmr  # noqa: E402
import pose_refine_ref as prr  # noqa: E402
import test_gpu_pose_search as tps  # noqa: E402  (scanner set-up and the filter record)
import test_gpu_pose_search_cloud as tpc  # noqa: E402  (the room)
from scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BEAMS = 31
LATTICES = ((1, 0), (0, 1), (2, 2), (4, 12))  # M = 9, 3, 125, 2025 (8 points per thread, a ragged last stride)
BASELINES = (0.0, 0.5, 0.9)
THETA_STEP = math.pi / 96.0
_SCENE = {}


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def scene(orc):
    """the 200 x 200 scenario map, 61 beams, no NaN range (the beam model's weight of a scan with one is NaN)"""
    if "geo" not in _SCENE:
        _SCENE["geo"] = Scenario(orc, size=200, beams=61, frac_nan=0.0)
    return _SCENE["geo"]


def start_poses(geo):
    """40: the centres of the 6 x 6 cells around the true pose's cell at the true heading rounded to a sixteenth of
    a turn, and four poses elsewhere on the map at other headings"""
    c = (geo.size // 2) * geo.res
    h = round(geo.pose[2] / (math.pi / 8.0)) * (math.pi / 8.0)
    poses = [[c + i * geo.res, c + j * geo.res, h] for i in range(-2, 4) for j in range(-3, 3)]
    poses += [[c - 2.013, c + 1.4, -2.0], [c + 3.1, c - 2.52, 1.1], [c + 1.0, c + 3.3, 3.0], [c - 3.0, c - 3.1, -0.4]]
    return np.array(poses, dtype=np.float64)


def steps_of(geo):
    return 0.5 * geo.res, THETA_STEP


def assert_rows_equal_model(rows, scores, poses, R, A, d, q, baseline):
    want = pmr.moments(poses, scores, R, A, d, q, baseline)
    assert rows.dtype == pmr.MOMENTS_DTYPE and rows.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------ 1. model, refinement, oracle
@pytest.mark.parametrize("R,A", LATTICES)
@pytest.mark.parametrize("model", prr.MODELS)
def test_rows_against_model_refinement_and_oracle(engine, orc, model, R, A):
    import badger_amcl_amd as bpf
    geo = scene(orc)
    kw = prr.MODEL_KW.get(model)
    m_, sc = tps.scanner_on(engine, geo, model, max_beams=MAX_BEAMS, kw=kw)
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = start_poses(geo)
    n = poses.shape[0]
    d, q = steps_of(geo)
    M, mc = prr.lattice(R, A)
    radius = np.array([R, R, A], dtype=np.float64)
    w = prr.oracle_lattice_scores(geo, geo.oracle_planar(MAX_BEAMS, model, kw=kw), poses, R, A, d, q, 0)
    refined, trace = sc.refinePoses(data, poses, R, d, A, q, 1, trace=True)
    first = None
    for baseline in BASELINES:
        rows, scores = sc.poseMoments(data, poses, R, d, A, q, baseline, scores=True)
        assert rows.shape == (n,) and scores.shape == (n, M)
        assert_rows_equal_model(rows, scores, poses, R, A, d, q, baseline)
        assert sc.poseMoments(data, poses, R, d, A, q, baseline).tobytes() == rows.tobytes()
        if first is None:
            first = scores
            # what a refinement of one level implies, bit for bit
            assert scores[:, mc].tobytes() == refined["score_in"].tobytes()
            assert scores[np.arange(n), trace[:, 0]].tobytes() == refined["score"].tobytes()
            assert np.array_equal(trace[:, 0], [prr.choose(scores[r], mc) for r in range(n)])
            assert refined["score"].tobytes() == rows["score_max"].tobytes()
            dev = np.abs(scores - w) / np.maximum(np.abs(w), 1e-300)
            print("pose moments %s (%d, %d): score deviation %.3e" % (model, R, A, dev.max()))
            assert dev.max() <= 1e-9
        assert scores.tobytes() == first.tobytes()  # the scores do not depend on the baseline
        want = pmr.moments(poses, w, R, A, d, q, baseline)
        assert np.array_equal(rows["flags"] & pmr.VALID, want["flags"] & pmr.VALID)
        assert (want["flags"] & pmr.VALID).sum() >= n - 4
        worst_mean = worst_cov = 0.0
        for r in np.flatnonzero(want["flags"] & pmr.VALID):
            delta = 4e-9 * M * want["score_max"][r] / want["weight_sum"][r]
            assert delta <= 4e-9 * M / (1.0 - baseline) * (1.0 + 1e-12)
            gm, gc = pmr.offset_moments(rows[r], poses[r], R, A, d, q)
            wm, wc = pmr.offset_moments(want[r], poses[r], R, A, d, q)
            em = np.abs(gm - wm) / np.maximum(delta * radius, 1e-300)
            ec = np.array([abs(gc[k] - wc[k]) / max(3.0 * delta * radius[u] * radius[v], 1e-300)
                           for k, (u, v) in enumerate(pmr.PAIRS)])
            worst_mean, worst_cov = max(worst_mean, em.max()), max(worst_cov, ec.max())
        print("  baseline %.1f: mean error %.3g of its bound, covariance error %.3g of its bound"
              % (baseline, worst_mean, worst_cov))
        assert worst_mean <= 1.0 and worst_cov <= 1.0


@pytest.mark.parametrize("R,A", [(2, 2), (4, 12)])
@pytest.mark.parametrize("model", prr.MODELS)
def test_groups_do_not_show(engine, orc, model, R, A):
    """n in {1, g, g + 1} with g = window / M the group size: a call of g + 1 poses equals two calls cut at g, and the
    rows are the model's"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    geo = scene(orc)
    m_, sc = tps.scanner_on(engine, geo, model, max_beams=MAX_BEAMS, kw=prr.MODEL_KW.get(model))
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    M, mc = prr.lattice(R, A)
    g = hpf.pose_search_window() // M
    assert 1 < g < 1023
    rng = np.random.default_rng(M)
    poses = geo.pose[None, :] + rng.uniform(-1.0, 1.0, (g + 1, 3)) * np.array([4 * geo.res, 4 * geo.res, 0.5])
    d, q = steps_of(geo)
    rows, scores = sc.poseMoments(data, poses, R, d, A, q, 0.5, scores=True)
    assert_rows_equal_model(rows, scores, poses, R, A, d, q, 0.5)
    assert np.all(rows["flags"] & pmr.VALID)
    a, sa = sc.poseMoments(data, poses[:g], R, d, A, q, 0.5, scores=True)
    b, sb = sc.poseMoments(data, poses[g:], R, d, A, q, 0.5, scores=True)
    assert a.shape == (g,) and b.shape == (1,)
    assert np.concatenate([a, b]).tobytes() == rows.tobytes()
    assert np.concatenate([sa, sb]).tobytes() == scores.tobytes()
    one = sc.poseMoments(data, poses[:1], R, d, A, q, 0.5)
    assert one.tobytes() == rows[:1].tobytes()
    # hit rows and refined rows are taken by their poses
    hits = np.zeros(3, dtype=hpf.POSE_HIT_DTYPE)
    hits["pose"] = poses[:3]
    refined = np.zeros(3, dtype=hpf.POSE_REFINED_DTYPE)
    refined["pose"] = poses[:3]
    assert sc.poseMoments(data, hits, R, d, A, q, 0.5).tobytes() == rows[:3].tobytes()
    assert sc.poseMoments(data, refined, R, d, A, q, 0.5).tobytes() == rows[:3].tobytes()


# ------------------------------------------------------------------------------------ 2. invalid and flat rows
def _uniform(R, A):
    return [R * (R + 1) / 3.0, 0.0, 0.0, R * (R + 1) / 3.0, 0.0, A * (A + 1) / 3.0]


def assert_flat(rows, scores, poses, R, A, d, q, baseline, values):
    """every lattice's scores are one number, one of `values`"""
    M, mc = prr.lattice(R, A)
    assert np.all(scores == scores[:, :1]) and np.all(np.isin(scores[:, 0], values))
    assert_rows_equal_model(rows, scores, poses, R, A, d, q, baseline)
    assert np.all(rows["flags"] == pmr.VALID) and np.all(rows["support"] == M)
    for r in range(rows.shape[0]):
        gm, gc = pmr.offset_moments(rows[r], poses[r], R, A, d, q)
        assert np.allclose(gc, _uniform(R, A), rtol=1e-13, atol=1e-13) and np.abs(gm).max() <= 1e-9


def assert_invalid(rows, poses):
    assert np.all(rows["flags"] == 0) and np.all(rows["support"] == 0)
    assert np.all(rows["weight_sum"] == 0.0) and np.all(rows["cov"] == 0.0)
    assert np.ascontiguousarray(rows["mean"]).tobytes() == poses.tobytes()  # (-0.0 stays -0.0)


@pytest.mark.parametrize("model", prr.MODELS)
def test_all_nan_scan(engine, orc, model):
    """every range NaN: every beam is skipped, so a model scores 1.0 (flat: the lattice's uniform moments) or NaN (the
    beam model: an invalid row), as the numpy model gives for the call's own scores"""
    import badger_amcl_amd as bpf
    geo = scene(orc)
    m_, sc = tps.scanner_on(engine, geo, model, max_beams=MAX_BEAMS, kw=prr.MODEL_KW.get(model))
    data = bpf.PlanarData(np.full(61, np.nan), geo.angles, geo.range_max)
    # cell centres around the true cell; the lattice stays inside each pose's own cell, so its scores are one number:
    # 1.0, or the non-free-space factor within the radius of a wall
    poses = start_poses(geo)[14:23].copy()
    poses[1, 2] = -0.0
    R, A, d, q = 2, 2, geo.res / 8, 0.01
    rows, scores = sc.poseMoments(data, poses, R, d, A, q, 0.5, scores=True)
    assert_rows_equal_model(rows, scores, poses, R, A, d, q, 0.5)
    if np.isnan(scores).all():
        assert model == "beam"
        assert_invalid(rows, poses)
        assert rows["score_max"].tobytes() == np.full(9, np.nan).tobytes()
    else:
        assert model != "beam"
        assert_flat(rows, scores, poses, R, A, d, q, 0.5, (1.0, geo.map_factors[1]))


def test_max_beams_below_two_scores_one(engine, orc):
    import badger_amcl_amd as bpf
    geo = scene(orc)
    m_, sc = tps.scanner_on(engine, geo, "lf", max_beams=1)
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = start_poses(geo)
    for R, A in LATTICES:
        for baseline in BASELINES:
            rows, scores = sc.poseMoments(data, poses, R, 2 * geo.res, A, 0.3, baseline, scores=True)
            assert_flat(rows, scores, poses, R, A, 2 * geo.res, 0.3, baseline, (1.0,))


def test_pose_off_the_map_is_invalid(engine, orc):
    """off_map_factor 0: every point of a lattice off the map scores 0"""
    import badger_amcl_amd as bpf
    geo = scene(orc)
    m_, sc = tps.scanner_on(engine, geo, "lf", max_beams=MAX_BEAMS)
    sc.setMapFactors(0.0, geo.map_factors[1], geo.map_factors[2])
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = np.array([[-5.0, 3.0, -0.0], [geo.pose[0], geo.pose[1], geo.pose[2]], [4.0, 25.0, 1.0]])
    R, A, d, q = 2, 2, geo.res, 0.05
    rows, scores = sc.poseMoments(data, poses, R, d, A, q, 0.5, scores=True)
    assert_rows_equal_model(rows, scores, poses, R, A, d, q, 0.5)
    assert np.all(scores[[0, 2]] == 0.0)
    assert_invalid(rows[[0, 2]], poses[[0, 2]])
    assert np.all(rows["score_max"][[0, 2]] == 0.0)
    assert rows["flags"][1] & pmr.VALID and rows["support"][1] > 0


# ------------------------------------------------------------------------------------ 3. corridor and corner
def test_corridor_and_corner(engine, orc):
    """the device's moments of the two scenarios against the oracle-only moments tests/test_pose_moments_cpu.py holds
    to the inequalities (principal axis, along > across, the face bits)"""
    import badger_amcl_amd as bpf
    R, d, A, q = pmr.SCENE_LATTICE
    M = prr.lattice(R, A)[0]
    for kind in ("corridor", "corner"):
        sn = pmr.Scene(orc, kind)
        m = bpf.OccupancyMap(engine, sn.res)
        m.setCells(sn.cells)
        m.setOrigin(sn.origin)
        m.setDistancesLUT(sn.lut, sn.max_dist)
        sc = bpf.PlanarScanner(engine)
        sc.init(pmr.SCENE_BEAMS, m)
        sc.setModelLikelihoodField(0.95, 0.05, 0.2, sn.max_dist)
        sc.setMapFactors(*sn.map_factors)
        sc.setPlanarScannerPose(sn.scanner_pose)
        data = bpf.PlanarData(sn.ranges, sn.angles, sn.range_max)
        rows, scores = sc.poseMoments(data, sn.hit[None, :], R, d, A, q, pmr.SCENE_BASELINE, scores=True)
        assert_rows_equal_model(rows, scores, sn.hit[None, :], R, A, d, q, pmr.SCENE_BASELINE)
        want = sn.oracle_moments()
        w = sn.oracle_scores(R, A, d, q)
        assert (np.abs(scores[0] - w) / w).max() <= 1e-9
        delta = 4e-9 * M * want["score_max"] / want["weight_sum"]
        gm, gc = pmr.offset_moments(rows[0], sn.hit, R, A, d, q)
        wm, wc = pmr.offset_moments(want, sn.hit, R, A, d, q)
        radius = np.array([R, R, A], dtype=np.float64)
        print(kind, "device", rows[0], "oracle", want)
        assert np.all(np.abs(gm - wm) <= delta * radius)
        for k, (u, v) in enumerate(pmr.PAIRS):
            assert abs(gc[k] - wc[k]) <= 3.0 * delta * radius[u] * radius[v]
        assert rows["flags"][0] == want["flags"] and rows["support"][0] == want["support"]


# ------------------------------------------------------------------------------------ 4. the 3-D form
def _room_poses():
    heading = lambda h: (2.0 * math.pi * h) / 8.0 - math.pi  # noqa: E731
    cells = [(i, j, 4) for i in range(4, 9) for j in range(2, 6)]
    cells += [(-30, 10, 1), (25, -20, 6), (0, 0, 3), (-12, -25, 7)]
    return np.array([[i * tpc.RES, j * tpc.RES, heading(h)] for i, j, h in cells])


@pytest.mark.parametrize("R,A", [(2, 2), (1, 0), (0, 3)])
@pytest.mark.parametrize("model", ["plain", "gompertz"])
def test_cloud_form_follows_the_seam_exactly(engine, orc, model, R, A):
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    assert pts.shape[0] >= 128
    om, sc = tpc.scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)  # 128 of the points
    data = bpf.PointCloudData(pts)
    poses = _room_poses()
    n = poses.shape[0]
    d, q = 2 * tpc.RES, math.pi / 16.0
    M, mc = prr.lattice(R, A)
    p = prr.lattice_poses(poses, R, A, d, q, 0)
    s = np.ones((n * M, 4), dtype=np.float64)
    s[:, :3] = p.reshape(-1, 3)
    sc.applyModelToSampleSet(data, s)
    for baseline in BASELINES:
        rows, scores = sc.poseMoments(data, poses, R, d, A, q, baseline, scores=True)
        assert scores.tobytes() == s[:, 3].tobytes()
        assert_rows_equal_model(rows, scores, poses, R, A, d, q, baseline)
        assert sc.poseMoments(data, poses, R, d, A, q, baseline).tobytes() == rows.tobytes()
    assert np.all(rows["flags"] & pmr.VALID) and len(np.unique(scores)) > n


def test_cloud_form_in_groups(engine, orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    om, sc = tpc.scanner_on(engine, lut, tf_xyz, tf_quat, max_dist)
    data = bpf.PointCloudData(pts)
    g = hpf.pose_search_window() // 125
    rng = np.random.default_rng(5)
    poses = np.array([0.3, 0.2, 0.1])[None, :] + rng.uniform(-1.0, 1.0, (g + 1, 3)) * np.array([0.5, 0.5, 0.5])
    rows, scores = sc.poseMoments(data, poses, 2, 0.1, 2, 0.1, 0.5, scores=True)
    assert_rows_equal_model(rows, scores, poses, 2, 2, 0.1, 0.1, 0.5)
    a, sa = sc.poseMoments(data, poses[:g], 2, 0.1, 2, 0.1, 0.5, scores=True)
    b, sb = sc.poseMoments(data, poses[g:], 2, 0.1, 2, 0.1, 0.5, scores=True)
    assert np.concatenate([a, b]).tobytes() == rows.tobytes()
    assert np.concatenate([sa, sb]).tobytes() == scores.tobytes()


# ------------------------------------------------------------------------------------ 5. nothing else moves
def _planar_filter_run(orc, recovery, with_moments):
    """tests/test_gpu_pose_refine.py::_planar_filter_run with pose moments where the refinements stood"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from map_geometry import GeoScenario
    geo = GeoScenario.named(orc, "G1", n=2500, beams=61, frac_nan=0.0, cloud="mixture" if recovery else "converged")
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        alpha = (0.001, 0.5) if recovery else (0.0, 0.0)
        m, sc, pf, data = geo.gpu_objects(e, 61, "prob", min_samples=100, seed=31, alpha=alpha,
                                          model_kw=dict(do_beamskip=1))
        scans = [geo.ranges, np.clip(geo.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0)]
        if recovery:
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            pf.setUniformPoseCheck(1e-20, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)  # scores against the remembered scan
        else:
            for _ in range(2):  # to convergence: the updates below run with beam skipping engaged
                sc.updateSensor(pf, data)
                pf.updateResample()
            assert pf.isConverged()
        recs, rows = [], []
        other = bpf.PlanarData(scans[2], geo.angles, geo.range_max)  # not the scan the filter remembers
        ci, cj = geo.size_x // 2, geo.size_y // 2
        poses = np.array([[float(geo.origin[0]) + i * geo.res, float(geo.origin[1]) + j * geo.res, 0.1 * (i + j)]
                          for i in range(-1, 2) for j in range(-1, 2)])
        assert ci > 1 and cj > 1
        sc.updateSensor(pf, bpf.PlanarData(scans[0], geo.angles, geo.range_max))
        if with_moments:
            rows.append(sc.poseMoments(other, poses, 1, geo.res, 1, 0.1, 0.5))
        recs.append(tps._record(pf))
        pf.updateResample()
        if with_moments:
            rows.append(sc.poseMoments(other, np.tile(poses, (70, 1)), 2, geo.res, 2, 0.1, 0.5, scores=True)[0])
        recs.append(tps._record(pf))
        for ranges in scans[1:]:
            sc.updateSensor(pf, bpf.PlanarData(ranges, geo.angles, geo.range_max))
            recs.append(tps._record(pf))
            pf.updateResample()
            recs.append(tps._record(pf))
        return recs, rows
    finally:
        e.close()


@pytest.mark.parametrize("recovery", [False, True])
def test_planar_moments_leave_the_filter_as_they_found_it(orc, recovery):
    a, rows = _planar_filter_run(orc, recovery, True)
    b, _ = _planar_filter_run(orc, recovery, False)
    assert [r.shape[0] for r in rows] == [9, 630] and all(np.all(r["flags"] & pmr.VALID) for r in rows)
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose"):
            assert ra[key] == rb[key], (step, key)


def _cloud_filter_run(orc, with_moments):
    """tests/test_gpu_pose_refine.py::_cloud_filter_run with pose moments where the refinements stood"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_cloud import _setup
    n = 2000
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, n, 8, 256, seed=4)
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        om, sc = tpc.scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 100, n, 0.001, 0.5, 85.0)
        pf.srand48(11)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.initWithSamples(s)
        other = bpf.PointCloudData(np.ascontiguousarray(pts[::3] * np.float32(0.8)))  # not the filter's cloud
        poses = _room_poses()
        recs, rows = [], []
        for scan in (pts, np.ascontiguousarray(pts * np.float32(0.5))):
            assert sc.updateSensor(pf, bpf.PointCloudData(scan))
            if with_moments:
                rows.append(sc.poseMoments(other, poses, 1, 0.1, 1, 0.1, 0.5))
            recs.append(tpc._record(e, pf))
            pf.updateResample()
            if with_moments:
                rows.append(sc.poseMoments(other, np.tile(poses, (25, 1)), 2, 0.1, 2, 0.1, 0.0, scores=True)[0])
            recs.append(tpc._record(e, pf))
        return recs, rows
    finally:
        e.close()


def test_cloud_moments_leave_the_filter_as_they_found_it(orc):
    a, rows = _cloud_filter_run(orc, True)
    b, _ = _cloud_filter_run(orc, False)
    assert [r.shape[0] for r in rows] == [24, 600, 24, 600]
    assert all(np.all(r["flags"] & pmr.VALID) for r in rows)
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose", "form"):
            assert ra[key] == rb[key], (step, key)


# ------------------------------------------------------------------------------------ 6. refusals
GOOD = dict(n_poses=4, xy_radius=1, xy_step=0.05, theta_radius=1, theta_step=0.1, baseline=0.5)
BAD = [dict(n_poses=0), dict(n_poses=1025), dict(n_poses=-1), dict(xy_radius=-1), dict(theta_radius=-1),
       dict(xy_radius=0, theta_radius=0), dict(xy_radius=9, theta_radius=3), dict(xy_radius=0, theta_radius=1024),
       dict(xy_step=0.0), dict(xy_step=-0.05), dict(xy_step=float("nan")), dict(xy_step=float("inf")),
       dict(theta_step=0.0), dict(theta_step=float("nan")), dict(theta_step=float("-inf")),
       dict(baseline=-0.1), dict(baseline=1.0), dict(baseline=1.5), dict(baseline=float("nan")),
       dict(baseline=float("inf")), dict(baseline=float("-inf")),
       dict(bad_pose=float("nan")), dict(bad_pose=float("inf")), dict(poses=None), dict(out=None), dict(scan=None)]
FILL = b"\xab"


def _raw(call, poses, kw):
    """(status, the rows' bytes, the scores' bytes) of one raw call with GOOD overridden by kw"""
    from badger_amcl_amd import _lib
    a = dict(GOOD)
    a.update({k: v for k, v in kw.items() if k in GOOD})
    p = np.array(poses[:4], dtype=np.float64)
    if "bad_pose" in kw:
        p[2, 1] = kw["bad_pose"]
    out = np.frombuffer(bytearray(FILL * (96 * 4)), dtype=np.uint8).copy()
    sco = np.frombuffer(bytearray(FILL * (8 * 4 * 27)), dtype=np.uint8).copy()
    rc = call(None if kw.get("poses", 0) is None else p.ctypes.data_as(C.POINTER(C.c_double)), a["n_poses"],
              a["xy_radius"], a["xy_step"], a["theta_radius"], a["theta_step"], a["baseline"],
              None if kw.get("out", 0) is None else out.ctypes.data_as(C.POINTER(_lib.PoseMoments)),
              sco.ctypes.data_as(C.POINTER(C.c_double)), "scan" in kw)
    return rc, out.tobytes(), sco.tobytes()


def _planar_call(e, data):
    rp, ap = data.pointers()

    def call(p, n, R, xy, A, th, base, out, sco, no_scan):
        return e.lib.bpf_planar_pose_moments(e.h, None if no_scan else rp, ap, data.range_count_, data.range_max_, p,
                                             n, R, xy, A, th, base, out, sco)
    return call


def _cloud_call(e, pts):
    def call(p, n, R, xy, A, th, base, out, sco, no_scan):
        return e.lib.bpf_cloud_pose_moments(e.h, None if no_scan else pts.ctypes.data_as(C.POINTER(C.c_float)),
                                            pts.shape[0], p, n, R, xy, A, th, base, out, sco)
    return call


def _assert_refusals(call, poses):
    for kw in BAD:
        rc, out, sco = _raw(call, poses, kw)
        assert rc == 1, kw
        assert out == FILL * len(out) and sco == FILL * len(sco), kw  # nothing was written
    # a step whose radius is 0 is not read
    for kw in (dict(xy_radius=0, xy_step=float("nan")), dict(theta_radius=0, theta_step=-1.0)):
        rc, out, sco = _raw(call, poses, kw)
        assert rc == 0, kw
        rows = np.frombuffer(out, dtype=pmr.MOMENTS_DTYPE)
        assert np.all(np.isfinite(rows["mean"])) and np.all(np.isfinite(rows["cov"]))
    rc, out, sco = _raw(call, poses, {})
    assert rc == 0 and sco != FILL * len(sco)
    assert _raw(call, poses, dict(baseline=0.0))[0] == 0
    assert _raw(call, poses, dict(baseline=math.nextafter(1.0, 0.0)))[0] == 0


def test_planar_refusals(engine, orc):
    import badger_amcl_amd as bpf
    geo = scene(orc)
    m_, sc = tps.scanner_on(engine, geo, "lf")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = start_poses(geo)
    _assert_refusals(_planar_call(engine, data), poses)
    assert engine.lib.bpf_planar_pose_moments(None, None, None, 0, 0.0, None, 0, 0, 0.0, 0, 0.0, 0.0, None, None) == 1
    # the limits themselves pass: 1024 poses, 2047 points
    assert sc.poseMoments(data, np.tile(poses[:8], (128, 1)), 0, 0.0, 1, 0.1, 0.5).shape[0] == 1024
    assert sc.poseMoments(data, poses[:1], 0, 0.0, 1023, 1e-3, 0.5).shape[0] == 1
    # the scoring path's own status passes through: the beam model with fewer ranges than max_beams
    m2, sc2 = tps.scanner_on(engine, geo, "beam", max_beams=100)
    with pytest.raises(bpf.BpfError) as ei:
        sc2.poseMoments(data, poses, 1, geo.res, 1, 0.1, 0.5)
    assert ei.value.code == 7
    m3, sc3 = tps.scanner_on(engine, geo, "lf")
    assert sc3.poseMoments(data, poses, 1, geo.res, 1, 0.1, 0.5).shape[0] == poses.shape[0]  # the engine goes on


def test_cloud_refusals(orc):
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    pts = np.array(pts)
    e = bpf.Engine(0)
    try:
        om, sc = tpc.scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 10, 100, 0.0, 0.0, 85.0)  # its state shows last_status and the evaluations
        before = bytes(pf.getState())
        _assert_refusals(_cloud_call(e, pts), _room_poses())
        assert bytes(pf.getState()) == before
        assert e.lib.bpf_cloud_pose_moments(None, None, 0, None, 0, 0, 0.0, 0, 0.0, 0.0, None, None) == 1
    finally:
        e.close()


def test_not_configured(orc):
    """the cases of tests/test_gpu_pose_refine.py::test_not_configured"""
    import badger_amcl_amd as bpf
    from test_gpu_pose_check import _cloud_setup
    geo = scene(orc)
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = start_poses(geo)
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    pts = np.array(pts)
    e = bpf.Engine(0)
    try:
        assert _raw(_planar_call(e, data), poses, {})[0] == 2  # nothing at all
        assert _raw(_cloud_call(e, pts), poses, {})[0] == 2
        m = bpf.OccupancyMap(e, geo.res)  # the map and its LUT, no planar model
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        m.setDistancesLUT(geo.lut, geo.max_dist)
        m.upload()
        rc, out, sco = _raw(_planar_call(e, data), poses, {})
        assert rc == 2 and out == FILL * len(out) and sco == FILL * len(sco)
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        m = bpf.OccupancyMap(e, geo.res)  # a map without a LUT (the beam model asks for none)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        sc = bpf.PlanarScanner(e)
        sc.init(tps.MAX_BEAMS, m)
        geo.configure_gpu_model(sc, "beam")
        assert _raw(_planar_call(e, data), poses, {})[0] == 2
        assert _raw(_cloud_call(e, pts), poses, {})[0] == 2  # only the planar scanner configured
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        keep = _cloud_setup(e, orc, 1000)  # only the cloud scanner configured: the planar form refuses
        assert _raw(_planar_call(e, data), poses, {})[0] == 2
        del keep
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        om = bpf.OctoMap(e, tpc.RES)  # the 3-D map without a cloud model
        om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
        assert _raw(_cloud_call(e, pts), poses, {})[0] == 2
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 7. end to end
# The moments' lattice comes from the sensor model, not from the search: the likelihood field's score is a sum of
# cubed Gaussians of sigma_hit, so a beam's term has the width s_eff = sigma_hit / sqrt(3) in the position of its end
# point.  Steps of s_eff / 2 at radius 4 span +-2 s_eff with 9 points per axis; in theta the same displacement of an
# end point at the scan's median range.  That lattice resolves the peak and holds it (no face bit, support well below
# M).  The refinement's own lattices do neither here: at its first level's steps the heading peak is narrower than one
# step (the variance falls to the floor), at a quarter of them the lattice lies inside the peak's flat top and returns
# its uniform moments, R (R + 1) / 3 steps^2.  The components take the moments' mean: the refined pose is the first
# point, in the order rule, of a plateau of a field that is constant over a cell, the weighted mean is its middle.
E2E_LATTICE = (4, 4)


def e2e_moment_steps(sc_):
    from badger_amcl_amd import synth
    s_eff = synth.LF_DEFAULTS["sigma_hit"] / math.sqrt(3.0)
    hit = sc_.ranges[np.isfinite(sc_.ranges) & (sc_.ranges < sc_.range_max)]
    return s_eff / 2.0, (s_eff / 2.0) / float(np.median(hit))


E2E_BASELINE = 0.5
E2E_FLOOR = (0.01, 0.01, 0.005)
E2E_CAP = tuple(2.0 * v for v in mo.E2E_SIGMA)


def _track(engine, orc, sc_, comps):
    """a fresh filter seeded with the components, E2E_CYCLES sensor updates and resamples on the device and the oracle;
    returns the device's max-weight pose after asserting it is the oracle's"""
    m, sc, pf, data = sc_.gpu_objects(engine, mo.E2E_BEAMS, "lf", min_samples=100, seed=mo.E2E_SEED)
    pf.initWithMixture(comps)
    opf = orc.ParticleFilter(100, mo.E2E_N, 0.0, 0.0, 85.0, seed=mo.E2E_SEED)
    want = mo.oracle_init_with_mixture(orc, opf, comps)
    dev = pf.getCurrentSet().samples
    assert pf.getRngState() == opf.pf.rng and np.abs(dev[:, :3] - want[:, :3]).max() <= 1e-12
    opf.set_samples(dev)  # from the DEVICE poses on both sides, as tests/test_gpu_mixture_init.py continues
    p = sc_.oracle_planar(mo.E2E_BEAMS, "lf")
    for _ in range(mo.E2E_CYCLES):
        sc.updateSensor(pf, data)
        pf.updateResample()
        opf.update_sensor(lambda s, conv: sc_.oracle_apply(p, s, conv))
        out = opf.update_resample()
        assert pf.getState().sample_count == out.sample_count and pf.getRngState() == opf.pf.rng
    w, pose = pf.getMaxWeightPose()
    ow, opose = mo.oracle_max_weight_pose(orc, opf.samples[:opf.sample_count])
    assert np.allclose(pose, opose, rtol=1e-12, atol=1e-12) and np.allclose(w, ow, rtol=1e-12, atol=1e-12)
    return pose


def test_search_refine_moments_seed_track(orc):
    """searchPoses -> refinePoses -> mixtureFromHits -> poseMoments -> mixtureApplyMoments -> initWithMixture -> three
    sensor updates and resamples.  The max-weight pose is the oracle run's of the same components, and it lies no
    farther (in the plane) from the true pose than the same chain with mixtureFromHits' fixed sigma.
    Measured on an MI355X (profiles/pose_moments.md): 0.005519 m with the moments against 0.007433 m with the fixed
    sigma."""
    import badger_amcl_amd as bpf
    sc_ = mo.e2e_scenario(orc)
    e = bpf.Engine(0)
    try:
        m, sc, pf, data = sc_.gpu_objects(e, mo.E2E_BEAMS, "lf", min_samples=100, seed=mo.E2E_SEED)
        hits = sc.searchPoses(data, mo.E2E_HEADINGS, mo.E2E_STRIDE, mo.E2E_HITS)
        R, A, L = mo.E2E_REFINE
        xy_step, theta_step = mo.e2e_refine_steps(sc_.res)
        refined = sc.refinePoses(data, hits, R, xy_step, A, theta_step, L)
        xy, th = mo.e2e_merge(sc_.res)
        mixture = bpf.mixtureFromHits(refined, mo.E2E_N, xy, th, mo.E2E_CAP, mo.E2E_SIGMA)
        assert mixture[0].shape[0] == mo.E2E_CAP
        d, q = e2e_moment_steps(sc_)
        rows = sc.poseMoments(data, refined, E2E_LATTICE[0], d, E2E_LATTICE[1], q, E2E_BASELINE)
        used = rows[mixture[1]]
        print("flags", used["flags"].tolist(), "support", used["support"].tolist())
        assert np.all(used["flags"] == pmr.VALID)  # valid, and no best point on a face: the lattice holds the peak
        assert np.all(used["support"] < prr.lattice(*E2E_LATTICE)[0] // 2)
        comps = bpf.mixtureApplyMoments(mixture, rows, E2E_FLOOR, E2E_CAP, take_mean=True)
        assert comps.tobytes() == pmr.apply_moments(mixture[0], mixture[1], rows, E2E_FLOOR, E2E_CAP, 1).tobytes()
        assert np.array_equal(comps["count"], mixture[0]["count"]) and not np.array_equal(comps["sigma"],
                                                                                          mixture[0]["sigma"])
        truth = np.asarray(sc_.pose, dtype=np.float64)
        with_moments = _track(e, orc, sc_, comps)
        fixed = _track(e, orc, sc_, mixture[0])
        d_moments = math.hypot(*(with_moments[:2] - truth[:2]))
        d_fixed = math.hypot(*(fixed[:2] - truth[:2]))
        print("distance to the true pose: %.6f m with the moments' sigma, %.6f m with the fixed sigma"
              % (d_moments, d_fixed))
        print("sigma of the components", comps["sigma"].tolist())
        assert mo.within_e2e_bound(with_moments, truth, sc_.res)
        assert d_moments <= d_fixed
    finally:
        e.close()
