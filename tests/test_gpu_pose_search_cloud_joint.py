"""Joint pose search with the cloud scanner on the device (bpf_cloud_search_poses_joint) against its numpy model
(pose_search_joint_ref.py), the single-cloud search, the seam and the oracle, in the room of
tests/test_gpu_pose_search_cloud.py: one cloud at a zero offset is searchPoses byte for byte, the composed poses are the
model's, the joint score is what three applyModelToSampleSet calls on the composed poses leave (weights carried), the
oracle's sequential scores within 1e-9 with the top-K set, ranges that compose, a 3-D filter cycle left as it was, and
the refusals.

The three clouds: the room's cloud, the same cloud as a scanner at pose (+) D_1 sees it (rigid(), computed in float64
with the yaw-only mounting and cast to float32; only an input), and a thinned, shrunk cloud of another size."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_cloud_ref as pscr  # noqa: E402
import pose_search_joint_ref as psj  # noqa: E402
from test_gpu_pose_search import decided_below, shifted_k  # noqa: E402,F401
from test_gpu_pose_search_cloud import (CASES, GZ, H, RES, S, _record, _status_of, assert_rows_follow_model,  # noqa: E402
                                        room, scanner_on, space_of, window)

pytestmark = pytest.mark.gpu

OFFSETS = np.array([(0.0, 0.0, 0.0), (0.15, -0.1, 0.4), (-0.2, 0.1, -2.9)], dtype=np.float64)
_ORACLE = {}


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rigid(pts, d, tf_xyz):
    """the cloud `pts` as the scanner sees it from pose (+) d: b = Rz(0.3) p + tf, b' = Rz(-dth)(b - (dx, dy, 0)),
    p' = Rz(-0.3)(b' - tf), in float64, cast to float32"""
    t = np.asarray(tf_xyz, dtype=np.float64)
    b = np.asarray(pts, dtype=np.float64) @ rot_z(0.3).T + t
    b = (b - np.array([d[0], d[1], 0.0])) @ rot_z(-d[2]).T
    return np.ascontiguousarray(((b - t) @ rot_z(-0.3).T).astype(np.float32))


def clouds_of(orc, pitched):
    """[PointCloudData] of the three clouds"""
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched, 6, 200)
    return [bpf.PointCloudData(np.array(pts)), bpf.PointCloudData(rigid(pts, OFFSETS[1], tf_xyz)),
            bpf.PointCloudData(np.ascontiguousarray(pts[::3] * np.float32(0.8)))]


def oracle_scores(orc, model, pitched):
    """the oracle's sequential scores of all 11 352 candidates of (H, S) on the model's composed poses, once per case"""
    key = (model, pitched)
    if key not in _ORACLE:
        lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
        if model == "plain":
            op = orc.cloud(orc.CLOUD_MODEL, 128, tf_xyz, tf_quat, z_hit=0.5, z_rand=0.05, sigma_hit=0.1)
        else:
            op = orc.cloud(orc.CLOUD_MODEL_GOMPERTZ, 128, tf_xyz, tf_quat, z_hit=0.5, z_rand=0.5, sigma_hit=0.1, **GZ)
        op.off_map_factor = 0.95
        sp = space_of(lut, H, S)
        datas = clouds_of(orc, pitched)
        poses = psj.compose(sp, np.arange(sp.total), OFFSETS)

        def apply_scan(s, samples):
            orc.cloud_apply(op, lut, samples, np.array(datas[s].points_))

        w = psj.sequential_scores(poses, apply_scan)
        w.setflags(write=False)
        _ORACLE[key] = w
    return _ORACLE[key]


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ 1. one cloud, zero offset
@pytest.mark.parametrize("model,pitched", CASES)
def test_one_cloud_at_zero_offset_equals_search_poses(engine, orc, model, pitched):
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    data = bpf.PointCloudData(pts)
    zero = [(0.0, 0.0, 0.0)]
    for k in (1, 64, 1024):
        want = sc.searchPoses(data, H, S, k)
        assert want.shape[0] == k
        assert sc.searchPosesJoint([data], zero, H, S, k).tobytes() == want.tobytes(), k
    # three windows, from inside the first to inside the last
    wn = window()
    want = sc.searchPoses(data, 24, 1, 64, 1000, 2 * wn)
    assert sc.searchPosesJoint([data], zero, 24, 1, 64, 1000, 2 * wn).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------ 2. composed poses
@pytest.mark.parametrize("headings,stride", [(H, S), (24, 1), (5, 3)])
def test_composed_poses_are_the_models(engine, orc, headings, stride):
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist)
    sp = space_of(lut, headings, stride)
    rng = np.random.default_rng(5)
    wn = window()
    edge = [c for c in (wn - 1, wn) if c < sp.total]
    cands = np.concatenate([[0, sp.total - 1], edge, rng.integers(0, sp.total, 1000)]).astype(np.int64)
    offsets = np.vstack([OFFSETS, [(0.37, -1.9, 7.5)]])
    got = sc.searchJointPoses(offsets, headings, stride, cands)
    assert got.shape == (cands.shape[0], 4, 3)
    assert got.tobytes() == psj.compose(sp, cands, offsets).tobytes()
    assert np.array_equal(got[:, 0], sp.rows(cands)[3])  # the zero offset: the base pose


# ------------------------------------------------------------------------------------ 3. search = seam
@pytest.mark.parametrize("model,pitched", CASES)
def test_joint_search_equals_the_seam_bit_for_bit(engine, orc, model, pitched):
    """three applyModelToSampleSet calls on the composed poses of all candidates, weights carried from 1.0: top_k of the
    result is the 1024 rows, bytes equal (the property test_search_equals_the_seam_bit_for_bit pins for one cloud)"""
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    datas = clouds_of(orc, pitched)
    assert [d.points_.shape[0] for d in datas] == [1200, 1200, 400]
    sp = space_of(lut, H, S)
    assert (sp.columns, sp.total) == (1419, 11352)
    poses = sc.searchJointPoses(OFFSETS, H, S, np.arange(sp.total))

    def apply_scan(s, samples):
        sc.applyModelToSampleSet(datas[s], samples)

    w = psj.sequential_scores(poses, apply_scan)
    want = pscr.top_k(w, 0, 1024)
    hits = sc.searchPosesJoint(datas, OFFSETS, H, S, 1024)
    assert hits.shape[0] == 1024
    assert_rows_follow_model(hits, sp, want)
    assert hits["score"].tobytes() == w[want].tobytes()
    assert len(np.unique(w)) > 1000  # the scores discriminate
    # not the single cloud's list
    assert not np.array_equal(sc.searchPoses(datas[0], H, S, 1024)["candidate"], hits["candidate"])


# ------------------------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize("model,pitched", CASES)
def test_hits_match_the_oracle(engine, orc, model, pitched):
    """Per case: hits outside 1e-9 relative of the oracle's sequential score (allowed: 3 * ceil(k / 300), the share the
    seam's own oracle test grants per application for a point on a voxel face, times three applications), printed with
    the largest deviation.  Both K are decided by the oracle in all four cases, so the top-K set is asserted as it is."""
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
    w = oracle_scores(orc, model, pitched)
    assert not np.isnan(w).any()
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    datas = clouds_of(orc, pitched)
    sp = space_of(lut, H, S)
    ranked = pscr.order(w, np.arange(sp.total))
    sorted_scores = w[ranked]
    for k in (64, 1024):
        assert shifted_k(sorted_scores, k) == k and decided_below(sorted_scores, k) == k
        hits = sc.searchPosesJoint(datas, OFFSETS, H, S, k)
        assert hits.shape[0] == k
        cand = hits["candidate"]
        assert cand.min() >= 0 and cand.max() < sp.total
        dev = np.abs(hits["score"] - w[cand]) / np.maximum(np.abs(w[cand]), 1e-300)
        outside = int((dev > 1e-9).sum())
        print("joint cloud pose search %s pitched=%d k=%d: %d hits outside 1e-9, largest relative deviation %.3e"
              % (model, pitched, k, outside, dev.max()))
        assert outside <= 3 * math.ceil(k / 300), (model, pitched, k, outside)
        d = np.diff(hits["score"])
        assert np.all(d <= 0.0)
        assert np.all(np.diff(cand)[d == 0.0] > 0)
        assert set(cand.tolist()) == set(ranked[:k].tolist()), (model, pitched, k)
        assert_rows_follow_model(hits, sp, cand)  # the BASE pose


# ------------------------------------------------------------------------------------ 5. ranges compose
def test_ranges_compose(engine, orc):
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist)
    datas = clouds_of(orc, False)
    headings, stride, k = 24, 1, 64
    wn = window()
    cut1, cut2 = wn + wn // 6, wn + wn // 4  # both inside the whole search's second window
    total, _ = sc.searchSpace(headings, stride)
    assert total > cut2 + k
    whole = sc.searchPosesJoint(datas, OFFSETS, headings, stride, k)
    assert whole.shape[0] == k
    parts = [sc.searchPosesJoint(datas, OFFSETS, headings, stride, k, 0, cut1),
             sc.searchPosesJoint(datas, OFFSETS, headings, stride, k, cut1, cut2 - cut1),
             sc.searchPosesJoint(datas, OFFSETS, headings, stride, k, cut2)]
    assert [p.shape[0] for p in parts] == [k, k, k]
    assert hpf.merge_pose_hits(parts, k).tobytes() == whole.tobytes()


def test_max_beams_below_two_scores_one(engine, orc):
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, max_beams=1)
    sp = space_of(lut, 5, 3)
    hits = sc.searchPosesJoint(clouds_of(orc, False), OFFSETS, 5, 3, 16, 7)
    assert np.all(hits["score"] == 1.0)
    assert_rows_follow_model(hits, sp, 7 + np.arange(16, dtype=np.int64))


# ------------------------------------------------------------------------------------ 6. nothing else moves
def _raw_joint(e, clouds, offsets, headings=4, stride=1, first=0, count=-1, k=8, hits=None, n_scans=None,
               null_cloud=None, n_points=None):
    """bpf_cloud_search_poses_joint as given, no Python check in between: (status, *n_hits_out)"""
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    if hits is None:
        hits = np.zeros(1024, dtype=hpf.POSE_HIT_DTYPE)
    s = len(clouds)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    pp = (fp * max(s, 1))(*[c.points_.ctypes.data_as(fp) for c in clouds])
    if null_cloud is not None:
        pp[null_cloud] = fp()
    np_ = np.array((n_points if n_points is not None else [c.points_.shape[0] for c in clouds]) + [0], dtype=np.int32)
    off = np.ascontiguousarray(np.vstack([np.asarray(offsets, dtype=np.float64).reshape(-1, 3), np.zeros((1, 3))]))
    n = C.c_int(-7)
    rc = e.lib.bpf_cloud_search_poses_joint(e.h, s if n_scans is None else n_scans, pp,
                                            np_.ctypes.data_as(C.POINTER(C.c_int)), off.ctypes.data_as(dp), headings,
                                            stride, first, count, k, hits.ctypes.data_as(C.POINTER(_lib.PoseHit)),
                                            C.byref(n))
    return rc, n.value


def _filter_run(orc, with_search):
    """the 3-D cycle of test_gpu_pose_search_cloud.py::_filter_run on a fresh engine, with joint searches and refused
    joint calls between its steps"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_cloud import _setup
    n = 2000
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, n, 8, 256, seed=4)
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 100, n, 0.001, 0.5, 85.0)
        pf.srand48(11)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.initWithSamples(s)
        # not the filter's clouds
        others = [bpf.PointCloudData(np.ascontiguousarray(pts[::3] * np.float32(0.8))),
                  bpf.PointCloudData(np.ascontiguousarray(pts[1::2] * np.float32(0.9))),
                  bpf.PointCloudData(rigid(pts, OFFSETS[2], tf_xyz))]
        bad = OFFSETS.copy()
        bad[0, 0] = np.nan
        recs, hits = [], []
        for scan in (pts, np.ascontiguousarray(pts * np.float32(0.5))):
            assert sc.updateSensor(pf, bpf.PointCloudData(scan))
            if with_search:
                hits.append(sc.searchPosesJoint(others, OFFSETS, 6, 2, 100))
                assert _raw_joint(e, others, bad)[0] == 1
                assert _raw_joint(e, others, OFFSETS, n_points=[10, 0, 10])[0] == 1
            recs.append(_record(e, pf))
            pf.updateResample()
            if with_search:
                hits.append(sc.searchPosesJoint(others, OFFSETS, 24, 1, 100, 1000))  # three windows
                assert _raw_joint(e, others, OFFSETS, headings=65537, stride=32)[0] == 8
                assert sc.searchJointPoses(OFFSETS, 6, 2, [0, 5]).shape == (2, 3, 3)
            recs.append(_record(e, pf))
        return recs, hits
    finally:
        e.close()


def test_joint_search_leaves_the_filter_as_it_found_it(orc):
    a, hits = _filter_run(orc, True)
    b, _ = _filter_run(orc, False)
    assert len(hits) == 4
    for h in hits:
        assert h.shape[0] == 100 and np.all(np.isfinite(h["score"]))
    assert hits[0].tobytes() == hits[2].tobytes() and hits[1].tobytes() == hits[3].tobytes()
    assert max(r["w_slow"] for r in b) > 0.0 and max(r["w_fast"] for r in b) > 0.0
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose", "form"):
            assert ra[key] == rb[key], (step, key)


# ------------------------------------------------------------------------------------ 7. refusals
def test_refusals(orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    datas = clouds_of(orc, False)
    e = bpf.Engine(0)
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 10, 100, 0.0, 0.0, 85.0)  # its state shows last_status and the evaluations
        total, cols = sc.searchSpace(4, 1)
        before = _status_of(pf)
        valid = sc.searchPosesJoint(datas, OFFSETS, 4, 1, 8)
        assert valid.shape[0] == 8 and _status_of(pf) == before
        nan_off = OFFSETS.copy()
        nan_off[1, 1] = np.nan
        bad = [dict(clouds=[], offsets=np.zeros((0, 3))),                                   # S = 0
               dict(clouds=[datas[0]] * 17, offsets=np.zeros((17, 3))),                     # S = 17
               dict(offsets=nan_off), dict(null_cloud=2), dict(n_points=[1200, 0, 400]), dict(n_points=[-1, 1200, 400]),
               dict(k=0), dict(k=1025), dict(headings=0), dict(stride=0),
               dict(first=total + 1), dict(count=total + 1), dict(first=1, count=total), dict(first=-1), dict(count=-2)]
        for kw in bad:
            args = dict(clouds=datas, offsets=OFFSETS)
            args.update(kw)
            buf = np.frombuffer(bytearray(b"\xab" * (4 * 56)), dtype=hpf.POSE_HIT_DTYPE).copy()
            assert _raw_joint(e, hits=buf, **args) == (1, -7), kw
            assert buf.tobytes() == b"\xab" * (4 * 56), kw
            assert _status_of(pf) == before, kw
            assert sc.searchPosesJoint(datas, OFFSETS, 4, 1, 8).tobytes() == valid.tobytes(), kw  # the engine goes on
        assert _raw_joint(e, [datas[2]] * 16, np.zeros((16, 3)))[0] == 0  # S = 16 is taken
        # the heading table's limit, and 65536 itself
        assert _raw_joint(e, datas, OFFSETS, headings=65537, stride=32) == (8, -7)
        assert _status_of(pf) == before
        assert sc.searchPosesJoint(datas, OFFSETS, 4, 1, 8).tobytes() == valid.tobytes()
        assert _raw_joint(e, datas, OFFSETS, headings=65536, stride=32, count=70000, k=4) == (0, 4)
        assert sc.searchPosesJoint(datas, OFFSETS, 4, 1, 8, total, -1).shape[0] == 0  # the empty range at the end
        # the diagnostic call's own refusals
        for kw in (dict(cands=[total]), dict(cands=[-1]), dict(offsets=nan_off), dict(headings=0)):
            a = dict(offsets=OFFSETS, headings=4, cands=[0, 1])
            a.update(kw)
            with pytest.raises(bpf.BpfError) as ei:
                sc.searchJointPoses(a["offsets"], a["headings"], 1, a["cands"])
            assert ei.value.code == 1, kw
        assert _status_of(pf) == before
    finally:
        e.close()


def test_not_configured(orc):
    import badger_amcl_amd as bpf
    from scenario import Scenario
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    datas = clouds_of(orc, False)
    e = bpf.Engine(0)
    try:
        # a planar-only engine: 2-D map, LUT and planar model, no 3-D map
        sc_ = Scenario(orc, size=200, n=100, beams=61)
        m_, psc, pf, pdata = sc_.gpu_objects(e, 61, "lf", min_samples=10, seed=3)
        before = _status_of(pf)
        assert _raw_joint(e, datas, OFFSETS) == (2, -7)
        out = np.zeros((1, 3, 3))
        cand = np.zeros(1, dtype=np.int64)
        assert e.lib.bpf_cloud_search_joint_poses(e.h, 4, 1, OFFSETS.ctypes.data_as(C.POINTER(C.c_double)), 3,
                                                  cand.ctypes.data_as(C.POINTER(C.c_longlong)), 1,
                                                  out.ctypes.data_as(C.POINTER(C.c_double))) == 2
        assert _status_of(pf) == before
        # the 3-D map, but no cloud model
        om = bpf.OctoMap(e, RES)
        om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
        assert _raw_joint(e, datas, OFFSETS) == (2, -7)
        assert _status_of(pf) == before
        # with the model, a valid search works
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        assert sc.searchPosesJoint(datas, OFFSETS, 4, 1, 8).shape[0] == 8
        assert _status_of(pf) == before
    finally:
        e.close()
