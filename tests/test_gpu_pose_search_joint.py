"""Joint pose search on the device (bpf_planar_search_poses_joint) against its numpy model (pose_search_joint_ref.py),
the single-scan search, the seam and the oracle: one scan at a zero offset is searchPoses byte for byte, the composed
poses are the model's byte for byte, the joint score is what three applyModelToSampleSet calls on the composed poses
leave (weights carried), the oracle's sequential scores within the project's 1e-9 bar with the top-K set where the
oracle decides it, ranges that compose, a filter left as it was, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_joint_ref as psj  # noqa: E402
import pose_search_ref as psr  # noqa: E402
from test_gpu_pose_search import (KS, MAX_BEAMS, MODEL_KW, ORACLE_SPACES, _record, assert_rows_follow_model,  # noqa: E402
                                  counts, decided_below, geometry, scanner_on, shifted_k, window)

pytestmark = pytest.mark.gpu

MODELS = ["lf", "gompertz", "prob", "beam"]
_SCANS = {}
_ORACLE = {}


def offsets_of(geo):
    r = geo.res
    return np.array([(0.0, 0.0, 0.0), (7 * r, -3 * r, 0.4), (-11 * r, 5 * r, -2.9)], dtype=np.float64)


def scans_of(orc, name):
    """(geo, offsets, [PlanarData of scan s cast from geo.pose (+) D_s]), built once per map"""
    if name not in _SCANS:
        import badger_amcl_amd as bpf
        from badger_amcl_amd import synth
        geo = geometry(orc, name)
        offs = offsets_of(geo)
        datas = []
        for s, d in enumerate(offs):
            ranges, angles = synth.cast_scan(geo.cells, geo.origin, geo.res, psj.pose_add(geo.pose, d), 61,
                                             range_max=geo.range_max, seed=3 + s, frac_max=0.03)
            datas.append(bpf.PlanarData(ranges, angles, geo.range_max))
        _SCANS[name] = (geo, offs, datas)
    return _SCANS[name]


def oracle_case(orc, name, model):
    """(geo, space, offsets, scans, the oracle's sequential scores of candidates 0 .. 2 Wn + 16 on the model's composed
    poses), computed once per (map, model)"""
    key = (name, model)
    if key not in _ORACLE:
        geo, offs, datas = scans_of(orc, name)
        sp = psr.Space.of(geo, *ORACLE_SPACES[name])
        n = counts()[-1]
        assert sp.total >= n, (name, sp.total)
        poses = psj.compose(sp, np.arange(n), offs)
        p = geo.oracle_planar(MAX_BEAMS, model, kw=MODEL_KW.get(model))

        def apply_scan(s, samples):
            orc.planar_apply(p, geo.omap, samples, datas[s].ranges_, datas[s].angles_, geo.range_max, 0, None)

        w = psj.sequential_scores(poses, apply_scan)
        w.setflags(write=False)
        _ORACLE[key] = (geo, sp, offs, datas, w)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ 1. one scan, zero offset
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_one_scan_at_zero_offset_equals_search_poses(engine, orc, name, model):
    import badger_amcl_amd as bpf
    geo = geometry(orc, name)
    m, sc = scanner_on(engine, geo, model, kw=MODEL_KW.get(model))
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    headings, stride = ORACLE_SPACES[name]
    for count in counts():
        for k in KS:
            want = sc.searchPoses(data, headings, stride, k, 0, count)
            got = sc.searchPosesJoint([data], [(0.0, 0.0, 0.0)], headings, stride, k, 0, count)
            assert want.shape[0] == min(k, count)
            assert got.tobytes() == want.tobytes(), (name, model, count, k)
    # a range that starts inside the space, to its end
    first = window() + 5
    want = sc.searchPoses(data, headings, stride, 64, first)
    assert sc.searchPosesJoint([data], [(0.0, 0.0, 0.0)], headings, stride, 64, first).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------ 2. composed poses
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_composed_poses_are_the_models(engine, orc, name):
    geo, offs, _ = scans_of(orc, name)
    m, sc = scanner_on(engine, geo, "lf")
    headings, stride = ORACLE_SPACES[name]
    sp = psr.Space.of(geo, headings, stride)
    wn = window()
    assert sp.total > wn + 1
    rng = np.random.default_rng(5)
    cands = np.concatenate([[0, sp.total - 1, wn - 1, wn], rng.integers(0, sp.total, 1000)]).astype(np.int64)
    offsets = np.vstack([offs, [(0.37, -1.9, 7.5)]])
    got = sc.searchJointPoses(offsets, headings, stride, cands)
    want = psj.compose(sp, cands, offsets)
    assert got.shape == (cands.shape[0], 4, 3)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got[:, 0], sp.rows(cands)[3])  # the zero offset: the base pose


def test_composed_poses_of_more_than_a_window(engine, orc):
    """the diagnostic call works through its candidates a window at a time"""
    geo, offs, _ = scans_of(orc, "G2")
    m, sc = scanner_on(engine, geo, "lf")
    headings, stride = ORACLE_SPACES["G2"]
    sp = psr.Space.of(geo, headings, stride)
    cands = np.arange(sp.total - 1, sp.total - 1 - (window() + 9), -1, dtype=np.int64)  # descending: a list, not a range
    got = sc.searchJointPoses(offs[1:], headings, stride, cands)
    assert got.tobytes() == psj.compose(sp, cands, offs[1:]).tobytes()
    assert sc.searchJointPoses(offs, headings, stride, []).shape == (0, 3, 3)


# ------------------------------------------------------------------------------------ 3. search = seam
@pytest.mark.parametrize("model", MODELS)
def test_joint_search_equals_the_seam_bit_for_bit(engine, orc, model):
    """The composed poses of ALL candidates of G2's space from the search's own kernel, scored by three
    applyModelToSampleSet calls with the weights carried from 1.0: the joint search's 1024 rows hold exactly top_k of
    those weights, scores equal as bytes.  A sample's sum is formed in an order that does not depend on the launch
    (point (3) of the pruned form).  Holds on an MI355X for all four models."""
    geo, offs, datas = scans_of(orc, "G2")
    m, sc = scanner_on(engine, geo, model, kw=MODEL_KW.get(model))
    headings, stride = ORACLE_SPACES["G2"]
    sp = psr.Space.of(geo, headings, stride)
    poses = sc.searchJointPoses(offs, headings, stride, np.arange(sp.total))

    def apply_scan(s, samples):
        sc.applyModelToSampleSet(datas[s], samples, 0)

    w = psj.sequential_scores(poses, apply_scan)
    want = psr.top_k(w, 0, 1024)
    hits = sc.searchPosesJoint(datas, offs, headings, stride, 1024)
    assert hits.shape[0] == 1024
    differ = int((hits["score"].view(np.uint64) != w[hits["candidate"]].view(np.uint64)).sum())
    print("joint search against the seam, %s: %d of 1024 scores differ in their bits" % (model, differ))
    assert_rows_follow_model(hits, sp, want)
    assert hits["score"].tobytes() == w[want].tobytes()
    assert len(np.unique(w)) > 1000  # the scores discriminate


# ------------------------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_hits_match_the_oracle(engine, orc, name, model):
    """Largest deviation of a hit's score from the oracle's sequential score, printed per case; the bar is 1e-9
    relative.  The top-K set is compared where the oracle decides it, as in test_gpu_pose_search.py."""
    geo, sp, offs, datas, w = oracle_case(orc, name, model)
    assert not np.isnan(w).any()
    m, sc = scanner_on(engine, geo, model, kw=MODEL_KW.get(model))
    headings, stride = ORACLE_SPACES[name]
    worst, up, down = 0.0, 0, 0
    for count in counts():
        scores = w[:count]
        ranked = psr.order(scores, np.arange(count))
        sorted_scores = scores[ranked]
        for k0 in KS:
            k_up = shifted_k(sorted_scores, k0)
            assert k_up - k0 <= 8, (name, model, count, k0, k_up)
            up = max(up, k_up - k0)
            k = min(k_up, 1024)  # (the API's limit)
            hits = sc.searchPosesJoint(datas, offs, headings, stride, k, 0, count)
            assert hits.shape[0] == min(k, count)
            cand = hits["candidate"]
            assert cand.min() >= 0 and cand.max() < count
            assert not np.isnan(hits["score"]).any()
            dev = np.abs(hits["score"] - scores[cand]) / np.maximum(np.abs(scores[cand]), 1e-300)
            worst = max(worst, float(dev.max()))
            assert dev.max() <= 1e-9, (name, model, count, k, dev.max())
            d = np.diff(hits["score"])
            assert np.all(d <= 0.0), (name, model, count, k)
            assert np.all(np.diff(cand)[d == 0.0] > 0), (name, model, count, k)
            if k == k_up:
                assert set(cand.tolist()) == set(ranked[:k].tolist()), (name, model, count, k)
            else:
                # the oracle's 1024-th and 1025-th scores are too close and the API takes no larger K: the hits hold the
                # oracle's top K' for the next decided K' below (as their own best K'), and nothing outside its top k_up
                k_dn = decided_below(sorted_scores, k)
                assert k - k_dn <= 8, (name, model, count, k_dn)
                down = max(down, k - k_dn)
                assert set(cand[:k_dn].tolist()) == set(ranked[:k_dn].tolist()), (name, model, count, k_dn)
                assert set(cand.tolist()) <= set(ranked[:k_up].tolist()), (name, model, count, k_up)
            assert_rows_follow_model(hits, sp, cand)  # the BASE pose
    print("joint pose search %s %s: largest relative score deviation %.3e, smallest oracle score %.3e, "
          "K shifted by up to %d upward / %d downward" % (name, model, worst, float(w.min()), up, down))


# ------------------------------------------------------------------------------------ 5. ranges compose
def test_ranges_compose(engine, orc):
    import badger_amcl_amd.pf as hpf
    geo, offs, datas = scans_of(orc, "G1")
    m, sc = scanner_on(engine, geo, "lf")
    headings, stride, k = 4, 1, 64
    wn = window()
    cut1, cut2 = wn - 5, wn + 64
    total, _ = sc.searchSpace(headings, stride)
    assert total > cut2 + k
    whole = sc.searchPosesJoint(datas, offs, headings, stride, k)
    assert whole.shape[0] == k
    parts = [sc.searchPosesJoint(datas, offs, headings, stride, k, 0, cut1),
             sc.searchPosesJoint(datas, offs, headings, stride, k, cut1, cut2 - cut1),
             sc.searchPosesJoint(datas, offs, headings, stride, k, cut2)]
    assert [p.shape[0] for p in parts] == [k, k, k]
    assert hpf.merge_pose_hits(parts, k).tobytes() == whole.tobytes()
    # and the joint score is not the single-scan score: the three scans changed the list
    single = sc.searchPoses(datas[0], headings, stride, k)
    assert not np.array_equal(single["candidate"], whole["candidate"])


def test_max_beams_below_two_scores_one(engine, orc):
    geo, offs, datas = scans_of(orc, "G3")
    m, sc = scanner_on(engine, geo, "lf", max_beams=1)
    sp = psr.Space.of(geo, 3, 1)
    hits = sc.searchPosesJoint(datas, offs, 3, 1, 16)
    assert np.all(hits["score"] == 1.0)
    assert_rows_follow_model(hits, sp, np.arange(16, dtype=np.int64))


# ------------------------------------------------------------------------------------ 6. nothing else moves
def _raw_joint(e, datas, offsets, headings=4, stride=1, first=0, count=-1, k=8, hits=None, n_scans=None,
               null_scan=None, range_counts=None):
    """bpf_planar_search_poses_joint as given, no Python check in between: (status, *n_hits_out)"""
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    if hits is None:
        hits = np.zeros(1024, dtype=hpf.POSE_HIT_DTYPE)
    s = len(datas)
    dp = C.POINTER(C.c_double)
    ptrs = [d.pointers() for d in datas]
    rp = (dp * max(s, 1))(*[p[0] for p in ptrs])
    ap = (dp * max(s, 1))(*[p[1] for p in ptrs])
    if null_scan is not None:
        rp[null_scan] = dp()
    rc_ = np.array((range_counts if range_counts is not None else [d.range_count_ for d in datas]) + [0], dtype=np.int32)
    mx = np.array([d.range_max_ for d in datas] + [0.0], dtype=np.float64)
    off = np.ascontiguousarray(np.vstack([np.asarray(offsets, dtype=np.float64).reshape(-1, 3), np.zeros((1, 3))]))
    n = C.c_int(-7)
    rc = e.lib.bpf_planar_search_poses_joint(e.h, s if n_scans is None else n_scans, rp, ap,
                                             rc_.ctypes.data_as(C.POINTER(C.c_int)), mx.ctypes.data_as(dp),
                                             off.ctypes.data_as(dp), headings, stride, first, count, k,
                                             hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n))
    return rc, n.value


def _filter_run(orc, recovery, with_search):
    """the filter cycle of test_gpu_pose_search.py::_filter_run (prob + beam skipping on G1, n = 2500, a fresh engine
    per run), with joint searches and refused joint calls between its steps"""
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
        others = [bpf.PlanarData(r, geo.angles, geo.range_max) for r in (scans[2], scans[1], scans[0])]
        offs = offsets_of(geo)
        hits = []

        def between():
            if not with_search:
                return
            hits.append(sc.searchPosesJoint(others, offs, 6, 2, 100))
            bad = offs.copy()
            bad[1, 2] = np.nan
            assert _raw_joint(e, others, bad)[0] == 1
            assert _raw_joint(e, [], np.zeros((0, 3)))[0] == 1
            assert _raw_joint(e, others, offs, headings=65537)[0] == 8
            assert sc.searchJointPoses(offs, 6, 2, [0, 5]).shape == (2, 3, 3)

        if recovery:
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            pf.setUniformPoseCheck(1e-20, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)  # scores against the remembered scan
        else:
            for _ in range(2):  # to convergence: the updates below run with beam skipping engaged
                sc.updateSensor(pf, data)
                pf.updateResample()
            assert pf.isConverged()
        recs = []
        sc.updateSensor(pf, bpf.PlanarData(scans[0], geo.angles, geo.range_max))
        between()
        recs.append(_record(pf))
        pf.updateResample()
        between()
        recs.append(_record(pf))
        for ranges in scans[1:]:
            sc.updateSensor(pf, bpf.PlanarData(ranges, geo.angles, geo.range_max))
            between()
            recs.append(_record(pf))
            pf.updateResample()
            recs.append(_record(pf))
        return recs, hits
    finally:
        e.close()


@pytest.mark.parametrize("recovery", [False, True])
def test_joint_search_leaves_the_filter_as_it_found_it(orc, recovery):
    a, hits = _filter_run(orc, recovery, True)
    b, _ = _filter_run(orc, recovery, False)
    assert len(hits) == 4
    for h in hits:
        assert h.shape[0] == 100 and np.all(np.isfinite(h["score"]))
        assert h.tobytes() == hits[0].tobytes()  # and the filter's steps do not move the search
    if recovery:
        assert max(r["w_diff"] for r in b) > 0.0  # random poses were drawn, through the scored pose check
    else:
        assert b[0]["converged"] == 1
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose"):
            assert ra[key] == rb[key], (step, key)


# ------------------------------------------------------------------------------------ 7. refusals
def test_refusals(engine, orc):
    import badger_amcl_amd.pf as hpf
    geo, offs, datas = scans_of(orc, "G2")
    m, sc = scanner_on(engine, geo, "lf")
    total, _ = sc.searchSpace(4, 1)
    valid = sc.searchPosesJoint(datas, offs, 4, 1, 8)
    assert valid.shape[0] == 8
    nan_off, inf_off = offs.copy(), offs.copy()
    nan_off[2, 0] = np.nan
    inf_off[0, 1] = np.inf
    bad = [dict(datas=[], offsets=np.zeros((0, 3))),                                        # S = 0
           dict(datas=[datas[0]] * 17, offsets=np.zeros((17, 3))),                          # S = 17
           dict(offsets=nan_off), dict(offsets=inf_off),
           dict(null_scan=1), dict(range_counts=[61, 0, 61]), dict(range_counts=[61, 61, -3]),
           dict(k=0), dict(k=1025), dict(headings=0), dict(stride=0),
           dict(first=total + 1), dict(count=total + 1), dict(first=1, count=total), dict(first=-1), dict(count=-2)]
    for kw in bad:
        args = dict(datas=datas, offsets=offs)
        args.update(kw)
        buf = np.frombuffer(bytearray(b"\xab" * (4 * 56)), dtype=hpf.POSE_HIT_DTYPE).copy()
        assert _raw_joint(engine, hits=buf, **args) == (1, -7), kw
        assert buf.tobytes() == b"\xab" * (4 * 56), kw
        assert sc.searchPosesJoint(datas, offs, 4, 1, 8).tobytes() == valid.tobytes(), kw  # and the engine goes on
    # S = 16 is taken
    assert _raw_joint(engine, [datas[0]] * 16, np.zeros((16, 3)))[0] == 0
    # the heading table's limit, and 65536 itself
    assert _raw_joint(engine, datas, offs, headings=65537, stride=16) == (8, -7)
    assert sc.searchPosesJoint(datas, offs, 4, 1, 8).tobytes() == valid.tobytes()
    assert _raw_joint(engine, datas, offs, headings=65536, stride=16, count=70000, k=4) == (0, 4)
    # the empty range at the end of the space
    assert sc.searchPosesJoint(datas, offs, 4, 1, 8, total, -1).shape[0] == 0
    # the diagnostic call's own refusals
    import badger_amcl_amd as bpf
    for kw in (dict(cands=[total]), dict(cands=[-1]), dict(offsets=nan_off), dict(headings=0)):
        a = dict(offsets=offs, headings=4, cands=[0, 1])
        a.update(kw)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchJointPoses(a["offsets"], a["headings"], 1, a["cands"])
        assert ei.value.code == 1, kw
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchJointPoses(offs, 65537, 16, [0])
    assert ei.value.code == 8
    # the scoring path's own status passes through: the beam model with fewer ranges than max_beams
    m2, sc2 = scanner_on(engine, geo, "beam", max_beams=100)
    with pytest.raises(bpf.BpfError) as ei:
        sc2.searchPosesJoint(datas, offs, 4, 1, 8)
    assert ei.value.code == 7
    m, sc = scanner_on(engine, geo, "lf")
    assert sc.searchPosesJoint(datas, offs, 4, 1, 8).tobytes() == valid.tobytes()


def test_not_configured(orc):
    import badger_amcl_amd as bpf
    from test_gpu_pose_check import _cloud_setup
    geo, offs, datas = scans_of(orc, "G3")
    e = bpf.Engine(0)
    try:
        # the map and its LUT, no planar model
        m = bpf.OccupancyMap(e, geo.res)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        m.setDistancesLUT(geo.lut, geo.max_dist)
        m.upload()
        assert _raw_joint(e, datas, offs) == (2, -7)
        # with the model, a valid call returns the rows of a fresh engine's
        m, sc = scanner_on(e, geo, "lf")
        first = sc.searchPosesJoint(datas, offs, 4, 1, 8)
        assert first.shape[0] == 8 and np.all(np.diff(first["score"]) <= 0.0)
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        # a map without a LUT (the beam model asks for none)
        m = bpf.OccupancyMap(e, geo.res)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        sc = bpf.PlanarScanner(e)
        sc.init(MAX_BEAMS, m)
        geo.configure_gpu_model(sc, "beam")
        assert _raw_joint(e, datas, offs) == (2, -7)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchJointPoses(offs, 4, 1, [0])
        assert ei.value.code == 2
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        # only the cloud scanner configured
        keep = _cloud_setup(e, orc, 1000)
        assert _raw_joint(e, datas, offs) == (2, -7)
        del keep
    finally:
        e.close()
