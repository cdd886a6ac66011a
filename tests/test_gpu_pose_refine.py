"""Pose refinement on the device (bpf_planar_refine_poses, bpf_cloud_refine_poses) against its numpy model
(pose_refine_ref.py), the oracle's scores of the explicit lattice poses (planar form) and the seam's (cloud form, bit
for bit): the trajectory, ties, the shapes at which the kernels take another path, a filter left as it was, and the
refusals."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_refine_ref as prr  # noqa: E402
import test_gpu_pose_search as tps  # noqa: E402  (its maps, scanner set-up and filter record)
import test_gpu_pose_search_cloud as tpc  # noqa: E402  (the room)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def assert_replay(rows, trace, poses, R, A, xy_step, theta_step):
    """the rows are what the model makes of the returned trace, bit for bit; returns the centres of every level"""
    final, moved, centres = prr.replay(poses, trace, R, A, xy_step, theta_step)
    assert np.ascontiguousarray(rows["pose"]).tobytes() == final.tobytes()
    assert np.array_equal(rows["moved"], moved)
    assert np.all(rows["reserved"] == 0)
    return centres


# ------------------------------------------------------------------------------------ 1. trajectory against the oracle
@pytest.mark.parametrize("config", prr.CONFIGS)
@pytest.mark.parametrize("model", prr.MODELS)
def test_trajectory_against_the_oracle(engine, orc, model, config):
    """Per case: the share of (pose, level) pairs the oracle decides, and the largest relative deviation of score and
    score_in from the oracle's, printed before the assertions."""
    import badger_amcl_amd as bpf
    R, A, L = config
    geo, poses, xy_step, theta_step = prr.planar_case(orc, model, config)
    m_, sc = tps.scanner_on(engine, geo, model, max_beams=prr.MAX_BEAMS, kw=prr.MODEL_KW.get(model))
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    rows, trace = sc.refinePoses(data, poses, R, xy_step, A, theta_step, L, trace=True)
    n = poses.shape[0]
    M, mc = prr.lattice(R, A)
    assert rows.shape == (n,) and trace.shape == (n, L)
    centres = assert_replay(rows, trace, poses, R, A, xy_step, theta_step)
    op = geo.oracle_planar(prr.MAX_BEAMS, model, kw=prr.MODEL_KW.get(model))
    exact = 0
    w = None
    for level in range(L):
        w = prr.oracle_lattice_scores(geo, op, centres[:, level], R, A, xy_step, theta_step, level)
        if level == 0:
            w_in = w[:, mc].copy()
        for r in range(n):
            best, dec = prr.decided(w[r], mc)
            got = trace[r, level]
            # no pair is left out of this one
            assert w[r, best] - w[r, got] <= prr.DECIDED * abs(w[r, best]), (model, config, r, level, got, best)
            if dec:
                assert got == best, (model, config, r, level, got, best)
                exact += 1
    w_final = w[np.arange(n), trace[:, L - 1]]  # the last level's chosen point is the final pose
    dev = np.abs(rows["score"] - w_final) / np.maximum(np.abs(w_final), 1e-300)
    dev_in = np.abs(rows["score_in"] - w_in) / np.maximum(np.abs(w_in), 1e-300)
    print("pose refine %s %s: %d of %d pairs decided, score deviation %.3e, score_in deviation %.3e"
          % (model, config, exact, n * L, dev.max(), dev_in.max()))
    assert exact >= 0.5 * n * L  # (a condition on the inputs: test_pose_refine_cpu.py holds the oracle alone to it)
    assert dev.max() <= 1e-9 and dev_in.max() <= 1e-9
    assert (trace != mc).any()


# ------------------------------------------------------------------------------------ 2. ties
def _cell_centres(geo, headings=(0.0, -0.0, 1.0)):
    """the centres of the 3 x 3 cells around the scenario's true cell, one heading each in turn"""
    ci, cj = geo.size_x // 2, geo.size_y // 2
    cells = [(i, j) for i in range(ci - 1, ci + 2) for j in range(cj - 1, cj + 2)]
    return np.array([[float(geo.origin[0]) + (i - geo.size_x // 2) * geo.res,
                      float(geo.origin[1]) + (j - geo.size_y // 2) * geo.res, headings[k % len(headings)]]
                     for k, (i, j) in enumerate(cells)])


def assert_untouched(rows, trace, poses, mc):
    assert np.ascontiguousarray(rows["pose"]).tobytes() == poses.tobytes()  # (-0.0 stays -0.0)
    assert np.all(rows["moved"] == 0) and np.all(trace == mc)


def test_flat_scores_leave_the_pose_where_it_was(engine, orc):
    """blind scan: every beam is skipped, and the lattice (steps of a quarter cell, halved twice) stays inside the
    pose's own cell, so all M scores are one number"""
    geo = tps.geometry(orc, "G1")
    m_, sc = tps.scanner_on(engine, geo, "lf")
    poses = _cell_centres(geo)
    assert np.signbit(poses[1, 2]) and poses[1, 2] == 0.0
    R, A, L = 1, 1, 3
    rows, trace = sc.refinePoses(tps.blind_scan(geo), poses, R, geo.res / 4, A, 0.2, L, trace=True)
    assert_untouched(rows, trace, poses, prr.lattice(R, A)[1])
    assert np.all(np.isfinite(rows["score"])) and rows["score"].tobytes() == rows["score_in"].tobytes()


def test_nan_scores_leave_the_pose_where_it_was(engine, orc):
    """the beam model with one NaN range: the weight of every pose is NaN"""
    import badger_amcl_amd as bpf
    geo = tps.geometry(orc, "G1")
    m_, sc = tps.scanner_on(engine, geo, "beam")
    ranges = geo.ranges.copy()
    ranges[30] = np.nan
    poses = _cell_centres(geo)
    R, A, L = 1, 1, 3
    rows, trace = sc.refinePoses(bpf.PlanarData(ranges, geo.angles, geo.range_max), poses, R, 2 * geo.res, A, 0.2, L,
                                 trace=True)
    assert_untouched(rows, trace, poses, prr.lattice(R, A)[1])
    assert np.all(np.isnan(rows["score"])) and np.all(np.isnan(rows["score_in"]))


def test_max_beams_below_two_scores_one(engine, orc):
    import badger_amcl_amd as bpf
    geo = tps.geometry(orc, "G3")
    m_, sc = tps.scanner_on(engine, geo, "lf", max_beams=1)
    poses = _cell_centres(geo)
    rows, trace = sc.refinePoses(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), poses, 2, geo.res, 0, 0.0, 2,
                                 trace=True)
    assert_untouched(rows, trace, poses, prr.lattice(2, 0)[1])
    assert np.all(rows["score"] == 1.0) and np.all(rows["score_in"] == 1.0)


# ------------------------------------------------------------------------------------ 3. shapes
def _shape_cases():
    """(R, A, n, L): n in {1, g, g + 1, 1024} with g = window / M the group size, where g < 1024; M = 3 (R = 0, A = 1:
    heading only, the smallest lattice there is -- M is odd), 25 (no heading), 27, 125 and 1053 (more points than a
    block of k_refine_select has threads); L in {1, 16}"""
    return [(0, 1, 1, 16), (0, 1, 1024, 1), (2, 0, 1024, 1), (1, 1, 1024, 16), (2, 2, "g", 1), (2, 2, "g+1", 16),
            (2, 2, 1024, 1), (4, 6, 1, 16), (4, 6, "g", 1), (4, 6, "g+1", 16), (4, 6, 1024, 1)]


def _seam_choice_holds(sc, data, centres, trace, rows_of, R, A, xy_step, theta_step):
    """for the poses `rows_of` at every level: the chosen point's score, as the host-buffer seam gives it for the
    explicit lattice poses, is within 4e-9 relative of the seam's best, and is the best where that one is decided"""
    M, mc = prr.lattice(R, A)
    for level in range(trace.shape[1]):
        p = prr.lattice_poses(centres[rows_of, level], R, A, xy_step, theta_step, level)
        s = np.ones((p.shape[0] * M, 4), dtype=np.float64)
        s[:, :3] = p.reshape(-1, 3)
        sc.applyModelToSampleSet(data, s, 0)
        w = s[:, 3].reshape(-1, M)
        for k, r in enumerate(rows_of):
            best, dec = prr.decided(w[k], mc)
            got = trace[r, level]
            assert w[k, best] - w[k, got] <= prr.DECIDED * abs(w[k, best]), (r, level, got, best)
            if dec:
                assert got == best, (r, level, got, best)


@pytest.mark.parametrize("R,A,n,L", _shape_cases())
def test_shapes(engine, orc, R, A, n, L):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    M, mc = prr.lattice(R, A)
    g = hpf.pose_search_window() // M
    if isinstance(n, str):
        assert 1 < g < 1023
        n = g if n == "g" else g + 1
    geo = tps.geometry(orc, "G2")
    m_, sc = tps.scanner_on(engine, geo, "lf")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    rng = np.random.default_rng(1000 * M + n)
    poses = geo.pose[None, :] + rng.uniform(-1.0, 1.0, (n, 3)) * np.array([4 * geo.res, 4 * geo.res, 0.5])
    xy_step, theta_step = 1.5 * geo.res, 0.1
    rows, trace = sc.refinePoses(data, poses, R, xy_step, A, theta_step, L, trace=True)
    assert rows.shape == (n,) and trace.shape == (n, L)
    centres = assert_replay(rows, trace, poses, R, A, xy_step, theta_step)
    assert np.all(np.isfinite(rows["score"])) and np.all(rows["score"] >= rows["score_in"])
    # the first and last pose, and those on either side of a group's boundary
    pick = sorted({0, n - 1} | ({g - 1, g} if n > g else set()))
    _seam_choice_holds(sc, data, centres, trace, pick, R, A, xy_step, theta_step)
    # without the trace the rows are the same
    assert sc.refinePoses(data, poses, R, xy_step, A, theta_step, L).tobytes() == rows.tobytes()
    if n > g:
        # the grouping does not show: two calls, cut at the boundary, give the same rows and trace bit for bit
        a, ta = sc.refinePoses(data, poses[:g], R, xy_step, A, theta_step, L, trace=True)
        b, tb = sc.refinePoses(data, poses[g:], R, xy_step, A, theta_step, L, trace=True)
        assert np.concatenate([a, b]).tobytes() == rows.tobytes()
        assert np.array_equal(np.concatenate([ta, tb]), trace)
    if L == 16 and n > 500:
        # the late levels still move (among hundreds of poses: the likelihood field is piecewise constant in the pose,
        # and a step of res / 170 and less rarely carries a beam's end point into another cell)
        assert (trace[:, 8:] != mc).any()
    # a POSE_HIT_DTYPE array is taken by its poses
    hits = np.zeros(min(n, 5), dtype=hpf.POSE_HIT_DTYPE)
    hits["pose"] = poses[:hits.shape[0]]
    assert sc.refinePoses(data, hits, R, xy_step, A, theta_step, L).tobytes() == rows[:hits.shape[0]].tobytes()


# ------------------------------------------------------------------------------------ 4. the 3-D form
def _room_poses():
    """columns around the room's true pose (0.3, 0.2, 0.1) at the nearest of 8 headings, and a few far from it"""
    heading = lambda h: (2.0 * math.pi * h) / 8.0 - math.pi  # noqa: E731
    cells = [(i, j, 4) for i in range(4, 9) for j in range(2, 6)]
    cells += [(-30, 10, 1), (25, -20, 6), (0, 0, 3), (-12, -25, 7)]
    return np.array([[i * tpc.RES, j * tpc.RES, heading(h)] for i, j, h in cells])


@pytest.mark.parametrize("config", [(1, 1, 3), (2, 2, 2), (0, 3, 4)])
@pytest.mark.parametrize("model,pitched", tpc.CASES)
def test_cloud_form_follows_the_seam_exactly(engine, orc, model, pitched, config):
    import badger_amcl_amd as bpf
    R, A, L = config
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc, pitched)
    om, sc = tpc.scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    data = bpf.PointCloudData(pts)
    poses = _room_poses()
    n = poses.shape[0]
    xy_step, theta_step = 2 * tpc.RES, math.pi / 8.0
    rows, trace = sc.refinePoses(data, poses, R, xy_step, A, theta_step, L, trace=True)
    centres = assert_replay(rows, trace, poses, R, A, xy_step, theta_step)
    M, mc = prr.lattice(R, A)
    distinct = 0
    for level in range(L):
        p = prr.lattice_poses(centres[:, level], R, A, xy_step, theta_step, level)
        s = np.ones((n * M, 4), dtype=np.float64)
        s[:, :3] = p.reshape(-1, 3)
        sc.applyModelToSampleSet(data, s)
        w = s[:, 3].reshape(n, M)
        want = np.array([prr.choose(w[r], mc) for r in range(n)])
        assert np.array_equal(trace[:, level], want), (model, pitched, config, level)
        distinct += sum(len(np.unique(w[r])) > 1 for r in range(n))
        if level == 0:
            assert rows["score_in"].tobytes() == w[:, mc].tobytes()
        if level == L - 1:
            assert rows["score"].tobytes() == w[np.arange(n), want].tobytes()
    assert distinct >= 0.5 * n * L and (trace != mc).any()  # the scores discriminate
    assert sc.refinePoses(data, poses, R, xy_step, A, theta_step, L).tobytes() == rows.tobytes()


def test_cloud_form_in_groups(engine, orc):
    """1024 poses at M = 125: two groups; the same rows as two calls cut at the boundary"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    om, sc = tpc.scanner_on(engine, lut, tf_xyz, tf_quat, max_dist)
    data = bpf.PointCloudData(pts)
    g = hpf.pose_search_window() // 125
    n = g + 1
    rng = np.random.default_rng(5)
    poses = np.array([0.3, 0.2, 0.1])[None, :] + rng.uniform(-1.0, 1.0, (n, 3)) * np.array([0.5, 0.5, 0.5])
    rows, trace = sc.refinePoses(data, poses, 2, 0.1, 2, 0.1, 2, trace=True)
    assert_replay(rows, trace, poses, 2, 2, 0.1, 0.1)
    a, ta = sc.refinePoses(data, poses[:g], 2, 0.1, 2, 0.1, 2, trace=True)
    b, tb = sc.refinePoses(data, poses[g:], 2, 0.1, 2, 0.1, 2, trace=True)
    assert np.concatenate([a, b]).tobytes() == rows.tobytes()
    assert np.array_equal(np.concatenate([ta, tb]), trace)


# ------------------------------------------------------------------------------------ 5. nothing else moves
def _planar_filter_run(orc, recovery, with_refine):
    """tests/test_gpu_pose_search.py::_filter_run with a refinement where the search stood"""
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
        poses = _cell_centres(geo)
        sc.updateSensor(pf, bpf.PlanarData(scans[0], geo.angles, geo.range_max))
        if with_refine:
            rows.append(sc.refinePoses(other, poses, 1, geo.res, 1, 0.1, 3))
        recs.append(tps._record(pf))
        pf.updateResample()
        if with_refine:
            rows.append(sc.refinePoses(other, np.tile(poses, (70, 1)), 2, geo.res, 2, 0.1, 2))  # two groups
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
def test_planar_refinement_leaves_the_filter_as_it_found_it(orc, recovery):
    a, rows = _planar_filter_run(orc, recovery, True)
    b, _ = _planar_filter_run(orc, recovery, False)
    assert [r.shape[0] for r in rows] == [9, 630] and all(np.all(np.isfinite(r["score"])) for r in rows)
    if recovery:
        assert max(r["w_diff"] for r in b) > 0.0
    else:
        assert b[0]["converged"] == 1
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose"):  # (state: w_slow, w_fast, last_status, evaluations ...)
            assert ra[key] == rb[key], (step, key)


def _cloud_filter_run(orc, with_refine):
    """tests/test_gpu_pose_search_cloud.py::_filter_run with refinements where the searches stood"""
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
            if with_refine:
                rows.append(sc.refinePoses(other, poses, 1, 0.1, 1, 0.1, 3))
            recs.append(tpc._record(e, pf))
            pf.updateResample()
            if with_refine:
                rows.append(sc.refinePoses(other, np.tile(poses, (25, 1)), 2, 0.1, 2, 0.1, 2))  # two groups
            recs.append(tpc._record(e, pf))
        return recs, rows
    finally:
        e.close()


def test_cloud_refinement_leaves_the_filter_as_it_found_it(orc):
    a, rows = _cloud_filter_run(orc, True)
    b, _ = _cloud_filter_run(orc, False)
    assert [r.shape[0] for r in rows] == [24, 600, 24, 600]
    assert all(np.all(np.isfinite(r["score"])) for r in rows)
    assert max(r["w_slow"] for r in b) > 0.0 and max(r["w_fast"] for r in b) > 0.0
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose", "form"):
            assert ra[key] == rb[key], (step, key)


def test_refinement_needs_no_filter(orc):
    import badger_amcl_amd as bpf
    geo = tps.geometry(orc, "G3")
    e = bpf.Engine(0)  # no bpf_pf_create on this engine
    try:
        m_, sc = tps.scanner_on(e, geo, "lf")
        rows = sc.refinePoses(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), _cell_centres(geo), 1, geo.res,
                              1, 0.1, 2)
        assert rows.shape[0] == 9 and np.all(rows["score"] >= rows["score_in"])
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 6. refusals
GOOD = dict(n_poses=4, xy_radius=1, xy_step=0.05, theta_radius=1, theta_step=0.1, levels=2)
BAD = [dict(n_poses=0), dict(n_poses=1025), dict(n_poses=-1), dict(xy_radius=-1), dict(theta_radius=-1),
       dict(xy_radius=0, theta_radius=0), dict(xy_radius=9, theta_radius=3), dict(xy_radius=0, theta_radius=1024),
       dict(levels=0), dict(levels=17), dict(xy_step=0.0), dict(xy_step=-0.05), dict(xy_step=float("nan")),
       dict(xy_step=float("inf")), dict(theta_step=0.0), dict(theta_step=float("nan")),
       dict(theta_step=float("-inf")), dict(bad_pose=float("nan")), dict(bad_pose=float("inf")), dict(poses=None),
       dict(out=None), dict(scan=None)]
FILL = b"\xab"


def _raw_refine(call, poses, kw):
    """(status, the output's bytes, the trace's bytes) of one raw call with GOOD overridden by kw"""
    from badger_amcl_amd import _lib
    a = dict(GOOD)
    a.update({k: v for k, v in kw.items() if k in GOOD})
    p = np.array(poses[:4], dtype=np.float64)
    if "bad_pose" in kw:
        p[2, 1] = kw["bad_pose"]
    out = np.frombuffer(bytearray(FILL * (48 * 4)), dtype=np.uint8).copy()
    tr = np.frombuffer(bytearray(FILL * (4 * 4 * 16)), dtype=np.uint8).copy()
    rc = call(None if kw.get("poses", 0) is None else p.ctypes.data_as(C.POINTER(C.c_double)), a["n_poses"],
              a["xy_radius"], a["xy_step"], a["theta_radius"], a["theta_step"], a["levels"],
              None if kw.get("out", 0) is None else out.ctypes.data_as(C.POINTER(_lib.PoseRefined)),
              tr.ctypes.data_as(C.POINTER(C.c_int)), "scan" in kw)
    return rc, out.tobytes(), tr.tobytes()


def _planar_call(e, data):
    rp, ap = data.pointers()

    def call(p, n, R, xy, A, th, L, out, tr, no_scan):
        return e.lib.bpf_planar_refine_poses(e.h, None if no_scan else rp, ap, data.range_count_, data.range_max_, p,
                                             n, R, xy, A, th, L, out, tr)
    return call


def _cloud_call(e, pts):
    def call(p, n, R, xy, A, th, L, out, tr, no_scan):
        return e.lib.bpf_cloud_refine_poses(e.h, None if no_scan else pts.ctypes.data_as(C.POINTER(C.c_float)),
                                            pts.shape[0], p, n, R, xy, A, th, L, out, tr)
    return call


def _assert_refusals(call, poses):
    for kw in BAD:
        rc, out, tr = _raw_refine(call, poses, kw)
        assert rc == 1, kw
        assert out == FILL * len(out) and tr == FILL * len(tr), kw  # nothing was written
    # a step whose radius is 0 is not read
    for kw in (dict(xy_radius=0, xy_step=float("nan")), dict(theta_radius=0, theta_step=-1.0)):
        rc, out, tr = _raw_refine(call, poses, kw)
        assert rc == 0, kw
        rows = np.frombuffer(out, dtype=[("pose", "<f8", (3,)), ("score", "<f8"), ("score_in", "<f8"),
                                         ("moved", "<i4"), ("reserved", "<i4")])
        assert np.all(np.isfinite(rows["pose"])) and np.all(rows["score"] >= rows["score_in"])
    assert _raw_refine(call, poses, {})[0] == 0


def test_planar_refusals(engine, orc):
    import badger_amcl_amd as bpf
    geo = tps.geometry(orc, "G2")
    m_, sc = tps.scanner_on(engine, geo, "lf")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = _cell_centres(geo)
    _assert_refusals(_planar_call(engine, data), poses)
    assert engine.lib.bpf_planar_refine_poses(None, None, None, 0, 0.0, None, 0, 0, 0.0, 0, 0.0, 0, None, None) == 1
    # the limits themselves pass: 1024 poses, 2047 points, 16 levels
    assert sc.refinePoses(data, np.tile(poses[:8], (128, 1)), 0, 0.0, 1, 0.1, 1).shape[0] == 1024
    assert sc.refinePoses(data, poses[:1], 0, 0.0, 1023, 1e-3, 1).shape[0] == 1
    assert sc.refinePoses(data, poses[:2], 1, geo.res, 0, 0.0, 16).shape[0] == 2
    # the scoring path's own status passes through: the beam model with fewer ranges than max_beams
    m2, sc2 = tps.scanner_on(engine, geo, "beam", max_beams=100)
    with pytest.raises(bpf.BpfError) as ei:
        sc2.refinePoses(data, poses, 1, geo.res, 1, 0.1, 2)
    assert ei.value.code == 7
    m3, sc3 = tps.scanner_on(engine, geo, "lf")
    assert sc3.refinePoses(data, poses, 1, geo.res, 1, 0.1, 2).shape[0] == 9  # and the engine goes on


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
        assert e.lib.bpf_cloud_refine_poses(None, None, 0, None, 0, 0, 0.0, 0, 0.0, 0, None, None) == 1
    finally:
        e.close()


def test_not_configured(orc):
    import badger_amcl_amd as bpf
    from test_gpu_pose_check import _cloud_setup
    geo = tps.geometry(orc, "G3")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    poses = _cell_centres(geo)
    lut, pts, tf_xyz, tf_quat, max_dist = tpc.room(orc)
    pts = np.array(pts)
    e = bpf.Engine(0)
    try:
        # nothing at all
        assert _raw_refine(_planar_call(e, data), poses, {})[0] == 2
        assert _raw_refine(_cloud_call(e, pts), poses, {})[0] == 2
        # the map and its LUT, no planar model
        m = bpf.OccupancyMap(e, geo.res)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        m.setDistancesLUT(geo.lut, geo.max_dist)
        m.upload()
        assert _raw_refine(_planar_call(e, data), poses, {})[0] == 2
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        # a map without a LUT (the beam model asks for none)
        m = bpf.OccupancyMap(e, geo.res)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        sc = bpf.PlanarScanner(e)
        sc.init(tps.MAX_BEAMS, m)
        geo.configure_gpu_model(sc, "beam")
        assert _raw_refine(_planar_call(e, data), poses, {})[0] == 2
        # only the planar scanner configured: the cloud form refuses
        assert _raw_refine(_cloud_call(e, pts), poses, {})[0] == 2
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        # only the cloud scanner configured: the planar form refuses
        keep = _cloud_setup(e, orc, 1000)
        assert _raw_refine(_planar_call(e, data), poses, {})[0] == 2
        del keep
        # the 3-D map without a cloud model
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        om = bpf.OctoMap(e, tpc.RES)
        om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
        assert _raw_refine(_cloud_call(e, pts), poses, {})[0] == 2
    finally:
        e.close()
