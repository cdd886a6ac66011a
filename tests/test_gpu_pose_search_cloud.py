"""Exhaustive pose search with the cloud scanner on the device (bpf_cloud_search_poses) against its numpy model
(pose_search_cloud_ref.py), against the seam (applyModelToSampleSet on the explicit candidate poses, bit for bit) and
against the oracle's scores: enumeration and tie order, the top-K set, ranges that compose, a filter left as it was,
and the refusals.

The shared case is "the room" of tests/test_gpu_cloud.py::_setup: box_room_voxels with bounds +-3 (cells
[-43, 43) x [-33, 33)), resolution 0.05 (the exact-reciprocal kernels), max_dist 0.3, tf (0.2, -0.1, 0.5) with mounting
yaw 0.3 (and that file's pitched quaternion for the general kernel), the true pose (0.3, 0.2, 0.1), the cloud
sphere_cloud(6, 200, seed 0) of 1 200 points."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_cloud_ref as pscr  # noqa: E402
from test_gpu_pose_search import decided_below, shifted_k  # noqa: E402  (the planar test's boundary rule)

pytestmark = pytest.mark.gpu

RES = 0.05
GZ = dict(gompertz_a=0.748, gompertz_b=5.0, gompertz_c=1.2, input_shift=-3.2, input_scale=6.7, output_shift=0.25)
H, S = 8, 2  # the scored cases: 1 419 columns, 11 352 candidates
CASES = [("plain", False), ("gompertz", False), ("plain", True), ("gompertz", True)]
_ROOM = {}
_ORACLE = {}


def window():
    import badger_amcl_amd.pf as hpf
    return hpf.pose_search_window()


def room(orc, pitched=False, rows=6, cols=200):
    """(lut, points, tf_xyz, tf_quat, max_dist), built once"""
    key = (pitched, rows, cols)
    if key not in _ROOM:
        from test_gpu_cloud import _setup
        lut, pts, _, tf_xyz, tf_quat, max_dist = _setup(orc, 1, rows, cols, seed=0, pitched=pitched)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        pts.setflags(write=False)
        _ROOM[key] = (lut, pts, tf_xyz, tf_quat, max_dist)
    return _ROOM[key]


def space_of(lut, headings, stride):
    return pscr.Space(list(lut.min_cells), list(lut.max_cells), RES, headings, stride)


def scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model="plain", max_beams=128):
    """3-D map + cloud scanner on the engine, no filter"""
    import badger_amcl_amd as bpf
    om = bpf.OctoMap(engine, RES)
    om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
    sc = bpf.PointCloudScanner(engine)
    sc.init(max_beams, om)
    if model == "plain":
        sc.setPointCloudModel(0.5, 0.05, 0.1)
    else:
        sc.setPointCloudModelGompertz(0.5, 0.5, 0.1, GZ["gompertz_a"], GZ["gompertz_b"], GZ["gompertz_c"],
                                      GZ["input_shift"], GZ["input_scale"], GZ["output_shift"])
    sc.setMapFactors(0.95, 0.95, 0.3)
    sc.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
    return om, sc


def oracle_scores(orc, model, pitched):
    """the oracle's scores of all 11 352 candidates of (H, S) in the room, computed once per case"""
    key = (model, pitched)
    if key not in _ORACLE:
        lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
        if model == "plain":
            op = orc.cloud(orc.CLOUD_MODEL, 128, tf_xyz, tf_quat, z_hit=0.5, z_rand=0.05, sigma_hit=0.1)
        else:
            op = orc.cloud(orc.CLOUD_MODEL_GOMPERTZ, 128, tf_xyz, tf_quat, z_hit=0.5, z_rand=0.5, sigma_hit=0.1, **GZ)
        op.off_map_factor = 0.95
        sp = space_of(lut, H, S)
        s = sp.samples(0, sp.total)
        orc.cloud_apply(op, lut, s, np.array(pts))
        w = s[:, 3].copy()
        w.setflags(write=False)
        _ORACLE[key] = w
    return _ORACLE[key]


def assert_rows_follow_model(hits, sp, cands):
    i, j, h, poses = sp.rows(cands)
    assert np.array_equal(hits["candidate"], cands)
    assert np.array_equal(hits["i"], i) and np.array_equal(hits["j"], j) and np.array_equal(hits["heading"], h)
    assert np.ascontiguousarray(hits["pose"]).tobytes() == poses.tobytes()
    assert np.all(hits["reserved"] == 0)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ 1. enumeration and tie order
@pytest.mark.parametrize("headings,stride,k", [(8, 1, 64), (5, 3, 1024), (1, 2, 7), (24, 1, 1024)])
def test_enumeration_and_tie_order_exact(engine, orc, headings, stride, k):
    """max_beams = 1: every score is 1.0, so the hits are the first k candidates of the range"""
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, max_beams=1)
    sp = space_of(lut, headings, stride)
    data = bpf.PointCloudData(pts)
    assert sc.searchSpace(headings, stride) == (sp.total, sp.columns)
    wn = window()
    ranges = [(0, -1), (1, -1), (1, 5)]
    if (headings, stride) == (24, 1):
        # three windows, the last one partial; and a range that starts in the middle of a window of the space and ends
        # inside another (two windows of its own, the second partial)
        assert sp.total == 136224 and 2 * wn < sp.total < 3 * wn
        ranges += [(wn // 2, wn + wn // 4), (wn - 1, -1), (sp.total - 3, -1)]
    for first, count in ranges:
        hits = sc.searchPoses(data, headings, stride, k, first, count)
        n = sp.total - first if count < 0 else count
        want = first + np.arange(min(k, n), dtype=np.int64)
        assert hits.shape[0] == want.shape[0]
        assert np.all(hits["score"] == 1.0)
        assert_rows_follow_model(hits, sp, want)


# ------------------------------------------------------------------------------------ 2. search = seam
@pytest.mark.parametrize("model,pitched,rows,cols", [c + (6, 200) for c in CASES] + [("plain", False, 8, 300)])
def test_search_equals_the_seam_bit_for_bit(engine, orc, model, pitched, rows, cols):
    """A sample's sum is formed by one wave per chunk of the cloud over that chunk's points and folded in chunk order
    (k_cloud_score, k_cloud_finish): nothing in it depends on how many samples the launch holds.  No tolerance."""
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched, rows, cols)
    assert pts.shape[0] == rows * cols
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    data = bpf.PointCloudData(pts)
    sp = space_of(lut, H, S)
    assert (sp.columns, sp.total) == (1419, 11352)
    s = sp.samples(0, sp.total)
    sc.applyModelToSampleSet(data, s)
    want = pscr.top_k(s[:, 3], 0, 1024)
    hits = sc.searchPoses(data, H, S, 1024)
    assert hits.shape[0] == 1024
    assert_rows_follow_model(hits, sp, want)
    assert hits["score"].tobytes() == s[want, 3].tobytes()
    assert len(np.unique(s[:, 3])) > 1000  # the scores discriminate


# ------------------------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("model,pitched", CASES)
def test_hits_match_the_oracle(engine, orc, model, pitched):
    """Per case: hits outside 1e-9 relative of the oracle's score (allowed: ceil(n / 300), the share
    test_cloud_apply_matches_oracle grants the seam for a point on a voxel face), printed with the largest
    deviation."""
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, pitched)
    w = oracle_scores(orc, model, pitched)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist, model)
    data = bpf.PointCloudData(pts)
    sp = space_of(lut, H, S)
    ranked = pscr.order(w, np.arange(sp.total))
    sorted_scores = w[ranked]
    for k in (64, 1024):
        hits = sc.searchPoses(data, H, S, k)
        assert hits.shape[0] == k
        cand = hits["candidate"]
        assert cand.min() >= 0 and cand.max() < sp.total
        dev = np.abs(hits["score"] - w[cand]) / np.maximum(np.abs(w[cand]), 1e-300)
        outside = int((dev > 1e-9).sum())
        print("cloud pose search %s pitched=%d k=%d: %d hits outside 1e-9, largest relative deviation %.3e"
              % (model, pitched, k, outside, dev.max()))
        assert outside <= math.ceil(k / 300), (model, pitched, k, outside)
        d = np.diff(hits["score"])
        assert np.all(d <= 0.0)
        assert np.all(np.diff(cand)[d == 0.0] > 0)
        k_up = shifted_k(sorted_scores, k)
        if k_up == k:
            assert set(cand.tolist()) == set(ranked[:k].tolist()), (model, pitched, k)
        else:
            # the oracle's k-th and (k+1)-th scores are too close to call: the hits hold the oracle's top K' for the
            # next decided K' below k (as their own best K'), and nothing outside its top k_up
            k_dn = decided_below(sorted_scores, k)
            assert k_dn > 0
            assert set(cand[:k_dn].tolist()) == set(ranked[:k_dn].tolist()), (model, pitched, k_dn)
            assert set(cand.tolist()) <= set(ranked[:k_up].tolist()), (model, pitched, k_up)
        assert_rows_follow_model(hits, sp, cand)
        # the true cell: column (6, 4) at heading 4 of 8
        best = hits[0]
        assert (best["candidate"], best["i"], best["j"], best["heading"]) == (6484, 6, 4, 4)
        assert best["pose"].tobytes() == np.array([6 * RES, 4 * RES, 0.0]).tobytes()
        assert abs(best["pose"][0] - 0.3) < 1e-15 and abs(best["pose"][1] - 0.2) < 1e-15
        if (model, pitched) == ("plain", False):
            print("runner-up / best = %.4f" % (hits[1]["score"] / best["score"]))
            assert hits[1]["score"] < 0.96 * best["score"]  # the runner-up is 5 % below
    assert len(np.unique(w)) < sp.total  # ties by candidate are exercised


# ------------------------------------------------------------------------------------ 4. ranges compose
def test_ranges_compose(engine, orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    om, sc = scanner_on(engine, lut, tf_xyz, tf_quat, max_dist)
    data = bpf.PointCloudData(pts)
    headings, stride, k = 24, 1, 64
    wn = window()
    # both cuts inside the whole search's second window, on either side of the true cell's candidates (column (6, 4) of
    # 86 x 66 at 24 headings: candidates 78 240 ...), so that every range holds some of the best k
    cut1, cut2 = wn + wn // 6, wn + wn // 4
    total, _ = sc.searchSpace(headings, stride)
    assert cut1 < (49 * 66 + 37) * 24 < cut2 and total > cut2 + k
    whole = sc.searchPoses(data, headings, stride, k)
    assert whole.shape[0] == k
    parts = [sc.searchPoses(data, headings, stride, k, 0, cut1),
             sc.searchPoses(data, headings, stride, k, cut1, cut2 - cut1),
             sc.searchPoses(data, headings, stride, k, cut2)]
    assert [p.shape[0] for p in parts] == [k, k, k]
    assert hpf.merge_pose_hits(parts, k).tobytes() == whole.tobytes()
    # the best k come from all three ranges: the merge had something to do
    c = whole["candidate"]
    assert (c < cut1).any() and ((c >= cut1) & (c < cut2)).any() and (c >= cut2).any()


# ------------------------------------------------------------------------------------ 5. nothing else moves
def _record(e, pf):
    st = pf.getState()
    w, pose = pf.getMaxWeightPose()
    return dict(samples=pf.getCurrentSet().samples.copy(), state=bytes(st), rng=pf.getRngState(), max_w=w,
                max_pose=pose.tobytes(), form=e.cloud_last_form(), w_slow=st.w_slow, w_fast=st.w_fast)


def _filter_run(orc, with_search):
    """a 3-D cycle over two steps on a fresh engine: updateSensor with the cloud, updateResample, getMaxWeightPose,
    with recovery armed (alpha_slow / alpha_fast set, random poses over the 3-D free space)"""
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
        other = bpf.PointCloudData(np.ascontiguousarray(pts[::3] * np.float32(0.8)))  # not the filter's cloud
        recs, hits = [], []
        for scan in (pts, np.ascontiguousarray(pts * np.float32(0.5))):
            assert sc.updateSensor(pf, bpf.PointCloudData(scan))
            if with_search:
                hits.append(sc.searchPoses(other, 6, 2, 100))
            recs.append(_record(e, pf))
            pf.updateResample()
            if with_search:
                hits.append(sc.searchPoses(other, 24, 1, 100, 1000))  # three windows
            recs.append(_record(e, pf))
        return recs, hits
    finally:
        e.close()


def test_search_leaves_the_filter_as_it_found_it(orc):
    a, hits = _filter_run(orc, True)
    b, _ = _filter_run(orc, False)
    assert len(hits) == 4
    for h in hits:
        assert h.shape[0] == 100 and np.all(np.isfinite(h["score"]))
    assert max(r["w_slow"] for r in b) > 0.0 and max(r["w_fast"] for r in b) > 0.0
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose", "form"):
            assert ra[key] == rb[key], (step, key)


def test_search_needs_no_filter(orc):
    import badger_amcl_amd as bpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    e = bpf.Engine(0)  # no bpf_pf_create on this engine
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        hits = sc.searchPoses(bpf.PointCloudData(pts), 4, 1, 8)
        assert hits.shape[0] == 8 and np.all(np.diff(hits["score"]) <= 0.0)
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 6. refusals
def _raw_search(e, pts, n_points, headings, stride, first, count, k, hits, n_ptr=True):
    from badger_amcl_amd import _lib
    n = C.c_int(-7)
    rc = e.lib.bpf_cloud_search_poses(e.h, None if pts is None else pts.ctypes.data_as(C.POINTER(C.c_float)), n_points,
                                      headings, stride, first, count, k,
                                      None if hits is None else hits.ctypes.data_as(C.POINTER(_lib.PoseHit)),
                                      C.byref(n) if n_ptr else None)
    return rc, n.value


def _status_of(pf):
    return bytes(pf.getState())


def test_refusals(orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    pts = np.array(pts)
    e = bpf.Engine(0)
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 10, 100, 0.0, 0.0, 85.0)  # its state shows last_status and the evaluations
        data = bpf.PointCloudData(pts)
        total, cols = sc.searchSpace(4, 1)
        assert (total, cols) == (4 * 86 * 66, 86 * 66)
        before = _status_of(pf)
        valid_best = sc.searchPoses(data, 4, 1, 1)["candidate"][0]
        assert _status_of(pf) == before
        bad = [dict(k=0), dict(k=1025), dict(headings=0), dict(cell_stride=0), dict(first=total + 1),
               dict(count=total + 1), dict(first=1, count=total), dict(first=-1), dict(count=-2)]
        for kw in bad:
            args = dict(headings=4, cell_stride=1, k=8, first=0, count=-1)
            args.update(kw)
            with pytest.raises(bpf.BpfError) as ei:
                sc.searchPoses(data, **args)
            assert ei.value.code == 1, kw
            assert _status_of(pf) == before, kw
            assert sc.searchPoses(data, 4, 1, 1)["candidate"][0] == valid_best, kw  # and a valid search works
        hits = np.zeros(8, dtype=hpf.POSE_HIT_DTYPE)
        # null or empty cloud, null outputs
        for raw in (dict(pts=None, n_points=10), dict(n_points=0), dict(n_points=-1), dict(hits=None),
                    dict(n_ptr=False)):
            args = dict(pts=pts, n_points=pts.shape[0], hits=hits, n_ptr=True)
            args.update(raw)
            assert _raw_search(e, args["pts"], args["n_points"], 4, 1, 0, -1, 8, args["hits"], args["n_ptr"])[0] == 1, raw
            assert _status_of(pf) == before, raw
            assert sc.searchPoses(data, 4, 1, 1)["candidate"][0] == valid_best, raw
        for kw in (dict(headings=0), dict(cell_stride=0)):
            with pytest.raises(bpf.BpfError) as ei:
                sc.searchSpace(**dict(dict(headings=4, cell_stride=1), **kw))
            assert ei.value.code == 1
        assert _status_of(pf) == before
        assert sc.searchPoses(data, 4, 1, 8, total, -1).shape[0] == 0  # the empty range at the end of the space
        # more than 2^31 - 1 candidates: refused before anything is launched, the output untouched; the space still
        # reports the product
        assert sc.searchSpace(1 << 29, 1) == (cols << 29, cols)
        buf = np.frombuffer(bytearray(b"\xab" * (4 * 56)), dtype=hpf.POSE_HIT_DTYPE).copy()
        rc, n = _raw_search(e, pts, pts.shape[0], 1 << 29, 1, 0, -1, 4, buf)
        assert rc == 8 and n == -7
        assert buf.tobytes() == b"\xab" * (4 * 56)
        assert _status_of(pf) == before
        assert sc.searchPoses(data, 3, 1, 8).shape[0] == 8  # and the engine goes on
        assert _status_of(pf) == before
        # a stride that leaves no column of all-positive bounds: an empty space, no hits, no error
        om2 = bpf.OctoMap(e, RES)
        om2.setDistancesLUT(np.zeros(5 * 5, dtype=np.uint32), np.full(3, 255, dtype=np.uint8), [1, 1, 0], [5, 5, 2], 0.3)
        assert sc.searchSpace(7, 1) == (7 * 16, 16)
        assert sc.searchSpace(7, 6) == (0, 0)
        assert sc.searchPoses(data, 7, 6, 8).shape[0] == 0
        assert sc.searchPoses(data, 7, 1, 8).shape[0] == 8
        assert _status_of(pf) == before
    finally:
        e.close()


def test_not_configured(orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    pts = np.array(pts)
    hits = np.zeros(8, dtype=hpf.POSE_HIT_DTYPE)
    e = bpf.Engine(0)
    try:
        # a planar-only engine: 2-D map, LUT and planar model, no 3-D map
        sc_ = Scenario(orc, size=200, n=100, beams=61)
        m_, psc, pf, pdata = sc_.gpu_objects(e, 61, "lf", min_samples=10, seed=3)
        before = _status_of(pf)
        assert _raw_search(e, pts, pts.shape[0], 4, 1, 0, -1, 8, hits) == (2, -7)
        total, cols = C.c_longlong(-1), C.c_int(-1)
        assert e.lib.bpf_cloud_search_space(e.h, 4, 1, C.byref(total), C.byref(cols)) == 2
        assert _status_of(pf) == before
        # the 3-D map, but no cloud model
        om = bpf.OctoMap(e, RES)
        om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
        assert e.lib.bpf_cloud_search_space(e.h, 4, 1, C.byref(total), C.byref(cols)) == 0
        assert (total.value, cols.value) == (4 * 86 * 66, 86 * 66)
        assert _raw_search(e, pts, pts.shape[0], 4, 1, 0, -1, 8, hits) == (2, -7)
        assert _status_of(pf) == before
        # with the model, a valid search works
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        assert sc.searchPoses(bpf.PointCloudData(pts), 4, 1, 8).shape[0] == 8
        assert _status_of(pf) == before
    finally:
        e.close()
