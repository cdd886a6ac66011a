"""Exhaustive pose search on the device (bpf_planar_search_poses) against its numpy model (pose_search_ref.py) and the
oracle's scores of the explicit candidate poses: enumeration and tie order bit for bit, scores within the project's
1e-9 bar, the top-K set, ranges that compose, a filter left as it was, refusals, and the cached free lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_ref as psr  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BEAMS = 31
# (headings, cell_stride) per map so that the space holds 2 Wn + 17 candidates (Wn = 65536: 131 089); the strided
# list on the wide map, many headings on the small one
ORACLE_SPACES = {"G1": (23, 2), "G2": (10, 1), "G3": (211, 1)}
MODEL_KW = {"prob": dict(do_beamskip=1)}  # beam skipping armed (the score runs with set->converged = 0)
KS = (1, 64, 1024)
_ORACLE = {}


def window():
    import badger_amcl_amd.pf as hpf
    return hpf.pose_search_window()


def counts():
    wn = window()
    return [1, 63, 65, wn - 1, wn, wn + 1, 2 * wn + 17]


def geometry(orc, name):
    from map_geometry import GeoScenario
    # (no NaN ranges: the beam model's weight of a scan with one is NaN for every pose)
    return GeoScenario.named(orc, name, beams=61, frac_nan=0.0)


def oracle_case(orc, name, model):
    """(geo, space, oracle scores of candidates 0 .. 2 Wn + 16), computed once per (map, model)"""
    key = (name, model)
    if key not in _ORACLE:
        geo = geometry(orc, name)
        sp = psr.Space.of(geo, *ORACLE_SPACES[name])
        n = counts()[-1]
        assert sp.total >= n, (name, sp.total)
        s = sp.samples(0, n)
        geo.oracle_apply(geo.oracle_planar(MAX_BEAMS, model, kw=MODEL_KW.get(model)), s, 0)
        w = s[:, 3].copy()
        w.setflags(write=False)
        _ORACLE[key] = (geo, sp, w)
    return _ORACLE[key]


def shifted_k(sorted_scores, k):
    """the next K >= k at which the oracle's K-th and (K+1)-th scores differ by more than 4e-9 relative (or K reaches
    the number of candidates): above the 1e-9 bar on either side, so that the top-K SET is decided"""
    n = len(sorted_scores)
    while k < n and not (sorted_scores[k - 1] - sorted_scores[k] > 4e-9 * abs(sorted_scores[k - 1])):
        k += 1
    return k


def decided_below(sorted_scores, k):
    """the next K <= k at which the K-th and (K+1)-th scores differ by more than 4e-9 relative (0: none)"""
    while k > 0 and not (sorted_scores[k - 1] - sorted_scores[k] > 4e-9 * abs(sorted_scores[k - 1])):
        k -= 1
    return k


def scanner_on(engine, geo, model, max_beams=MAX_BEAMS, kw=None):
    """map + planar scanner on the engine, no filter"""
    import badger_amcl_amd as bpf
    m = bpf.OccupancyMap(engine, geo.res)
    m.setCells(geo.cells)
    m.setOrigin(geo.origin)
    m.setDistancesLUT(geo.lut, geo.max_dist)
    sc = bpf.PlanarScanner(engine)
    sc.init(max_beams, m)
    geo.configure_gpu_model(sc, model, kw)
    sc.setMapFactors(*geo.map_factors)
    sc.setPlanarScannerPose(geo.scanner_pose)
    return m, sc


def blind_scan(geo):
    """every range >= range_max: every beam is skipped, so a candidate further than the radius from an obstacle
    scores exactly 1.0 (planar_scanner.cpp:236-323,642-682)"""
    import badger_amcl_amd as bpf
    return bpf.PlanarData(np.full(61, geo.range_max), geo.angles, geo.range_max)


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
@pytest.mark.parametrize("headings,stride,k", [(8, 1, 64), (5, 3, 1024), (1, 2, 7)])
def test_enumeration_and_tie_order_exact(engine, orc, headings, stride, k):
    geo = geometry(orc, "G2")
    m, sc = scanner_on(engine, geo, "lf")
    sp = psr.Space.of(geo, headings, stride)
    assert sc.searchSpace(headings, stride) == (sp.total, sp.ij.shape[0])
    wn = window()
    firsts = [f for f in (0, 1, wn - 1) if f < sp.total]
    if (headings, stride) == (8, 1):
        assert firsts[-1] == wn - 1 and sp.total > wn + k  # the range that starts at a window's last candidate
    for first in firsts:
        hits = sc.searchPoses(blind_scan(geo), headings, stride, k, first)
        want = first + np.arange(min(k, sp.total - first), dtype=np.int64)
        assert hits.shape[0] == want.shape[0]
        assert np.all(hits["score"] == 1.0)
        assert_rows_follow_model(hits, sp, want)
    # a range cut by count, ending inside the space
    hits = sc.searchPoses(blind_scan(geo), headings, stride, k, 1, 5)
    assert_rows_follow_model(hits, sp, 1 + np.arange(min(k, 5), dtype=np.int64))


def test_max_beams_below_two_scores_one(engine, orc):
    """applyModelToSampleSet returns at once with max_beams < 2 (planar_scanner.cpp:144-145): the weight stays 1.0"""
    import badger_amcl_amd as bpf
    geo = geometry(orc, "G3")
    m, sc = scanner_on(engine, geo, "lf", max_beams=1)
    sp = psr.Space.of(geo, 3, 1)
    hits = sc.searchPoses(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), 3, 1, 16)
    assert np.all(hits["score"] == 1.0)
    assert_rows_follow_model(hits, sp, np.arange(16, dtype=np.int64))


# ------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("model", ["lf", "gompertz", "prob", "beam"])
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_hits_match_the_oracle(engine, orc, name, model):
    """Largest deviation of a hit's score from the oracle's, printed per case; the bar is 1e-9 relative (seen on an
    MI355X: 2.5e-15 or less for lf, gompertz and beam, 5.7e-14 to 8.5e-14 for prob)."""
    import badger_amcl_amd as bpf
    geo, sp, w = oracle_case(orc, name, model)
    m, sc = scanner_on(engine, geo, model, kw=MODEL_KW.get(model))
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    headings, stride = ORACLE_SPACES[name]
    worst = 0.0
    for count in counts():
        scores = w[:count]
        ranked = psr.order(scores, np.arange(count))
        sorted_scores = scores[ranked]
        for k0 in KS:
            k_up = shifted_k(sorted_scores, k0)
            assert k_up - k0 <= 8, (name, model, count, k0, k_up)
            k = min(k_up, 1024)  # (the API's limit: see below)
            hits = sc.searchPoses(data, headings, stride, k, 0, count)
            assert hits.shape[0] == min(k, count)
            cand = hits["candidate"]
            assert cand.min() >= 0 and cand.max() < count
            dev = np.abs(hits["score"] - scores[cand]) / np.maximum(np.abs(scores[cand]), 1e-300)
            worst = max(worst, float(dev.max()))
            assert dev.max() <= 1e-9, (name, model, count, k, dev.max())
            d = np.diff(hits["score"])
            assert np.all(d <= 0.0), (name, model, count, k)
            assert np.all(np.diff(cand)[d == 0.0] > 0), (name, model, count, k)
            if k == k_up:
                assert set(cand.tolist()) == set(ranked[:k].tolist()), (name, model, count, k)
            else:
                # K = 1024 is the largest a call takes, so where the oracle's 1024-th and 1025-th scores are too
                # close the shift upward cannot be asked for: the hits then hold the oracle's top K' for the next
                # decided K' below 1024 (as their own best K'), and nothing outside its top k_up
                k_dn = decided_below(sorted_scores, k)
                assert k - k_dn <= 8, (name, model, count, k_dn)
                assert set(cand[:k_dn].tolist()) == set(ranked[:k_dn].tolist()), (name, model, count, k_dn)
                assert set(cand.tolist()) <= set(ranked[:k_up].tolist()), (name, model, count, k_up)
            assert_rows_follow_model(hits, sp, cand)
    print("pose search %s %s: largest relative score deviation %.3e" % (name, model, worst))


# ------------------------------------------------------------------------------------ 3. ranges compose
def test_ranges_compose(engine, orc, tmp_path):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    import cpp_driver
    geo = geometry(orc, "G1")
    m, sc = scanner_on(engine, geo, "lf")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    headings, stride, k = 4, 1, 64
    wn = window()
    cut1, cut2 = wn - 5, wn + 64
    total, _ = sc.searchSpace(headings, stride)
    assert total > cut2 + k
    whole = sc.searchPoses(data, headings, stride, k)
    assert whole.shape[0] == k
    parts = [sc.searchPoses(data, headings, stride, k, 0, cut1),
             sc.searchPoses(data, headings, stride, k, cut1, cut2 - cut1),
             sc.searchPoses(data, headings, stride, k, cut2)]
    assert [p.shape[0] for p in parts] == [k, k, k]
    assert hpf.merge_pose_hits(parts, k).tobytes() == whole.tobytes()
    # the same through the C++ adapter, merged by PlanarScanner::mergePoseHits
    exe = cpp_driver.compile_driver(tmp_path, "pose_search_smoke")
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(cells=geo.cells.astype(np.int32),
                                                                lut=np.asarray(geo.lut, dtype=np.float32),
                                                                ranges=geo.ranges, angles=geo.angles))
    out_whole, out_merged = str(tmp_path / "whole.bin"), str(tmp_path / "merged.bin")
    res = subprocess.run([str(exe), paths["cells"], paths["lut"], paths["ranges"], paths["angles"], str(geo.size_x),
                          str(geo.size_y), repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])),
                          str(MAX_BEAMS), str(headings), str(stride), str(k), str(cut1), str(cut2), out_whole,
                          out_merged], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert [int(v) for v in res.stdout.split()] == [total, total // headings, k, k, k]
    assert open(out_whole, "rb").read() == whole.tobytes()
    assert open(out_merged, "rb").read() == whole.tobytes()


# ------------------------------------------------------------------------------------ 4. nothing else moves
def _record(pf):
    st = pf.getState()
    w, pose = pf.getMaxWeightPose()
    return dict(samples=pf.getCurrentSet().samples.copy(), state=bytes(st), rng=pf.getRngState(), max_w=w,
                max_pose=pose.tobytes(), w_diff=st.w_diff, converged=st.converged)


def _filter_run(orc, recovery, with_search):
    """prob + beam skipping on G1, n = 2500; a fresh engine per run.  Returns what the filter showed after every
    step and the search's hits."""
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
        recs, hits = [], None
        sc.updateSensor(pf, bpf.PlanarData(scans[0], geo.angles, geo.range_max))
        if with_search:
            # another scan than the one the filter remembers for its pose check
            hits = sc.searchPoses(bpf.PlanarData(scans[2], geo.angles, geo.range_max), 6, 2, 100)
        recs.append(_record(pf))
        pf.updateResample()
        recs.append(_record(pf))
        for ranges in scans[1:]:
            sc.updateSensor(pf, bpf.PlanarData(ranges, geo.angles, geo.range_max))
            recs.append(_record(pf))
            pf.updateResample()
            recs.append(_record(pf))
        return recs, hits
    finally:
        e.close()


@pytest.mark.parametrize("recovery", [False, True])
def test_search_leaves_the_filter_as_it_found_it(orc, recovery):
    a, hits = _filter_run(orc, recovery, True)
    b, _ = _filter_run(orc, recovery, False)
    assert hits.shape[0] == 100 and np.all(np.isfinite(hits["score"]))
    if recovery:
        assert max(r["w_diff"] for r in b) > 0.0  # random poses were drawn, through the scored pose check
    else:
        assert b[0]["converged"] == 1
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose"):
            assert ra[key] == rb[key], (step, key)


def test_search_needs_no_filter(orc):
    import badger_amcl_amd as bpf
    geo = geometry(orc, "G3")
    e = bpf.Engine(0)  # no bpf_pf_create on this engine
    try:
        m, sc = scanner_on(e, geo, "lf")
        hits = sc.searchPoses(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), 4, 1, 8)
        assert hits.shape[0] == 8 and np.all(np.diff(hits["score"]) <= 0.0)
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 5. refusals
def _raw_search(e, data, headings, stride, first, count, k, hits):
    from badger_amcl_amd import _lib
    n = C.c_int(-7)
    rp, ap = data.pointers()
    rc = e.lib.bpf_planar_search_poses(e.h, rp, ap, data.range_count_, data.range_max_, headings, stride, first, count,
                                       k, hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n))
    return rc, n.value


def test_refusals(engine, orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    geo = geometry(orc, "G2")
    m, sc = scanner_on(engine, geo, "lf")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    total, _ = sc.searchSpace(4, 1)
    bad = [dict(k=0), dict(k=1025), dict(headings=0), dict(cell_stride=0), dict(first=total + 1),
           dict(count=total + 1), dict(first=1, count=total), dict(first=-1), dict(count=-2)]
    for kw in bad:
        args = dict(headings=4, cell_stride=1, k=8, first=0, count=-1)
        args.update(kw)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchPoses(data, **args)
        assert ei.value.code == 1, kw
    assert sc.searchPoses(data, 4, 1, 8, total, -1).shape[0] == 0  # the empty range at the end of the space
    # the scoring path's own status passes through: the beam model with fewer ranges than max_beams
    m2, sc2 = scanner_on(engine, geo, "beam", max_beams=100)
    with pytest.raises(bpf.BpfError) as ei:
        sc2.searchPoses(data, 4, 1, 8)
    assert ei.value.code == 7
    # more than 2^31 - 1 candidates: refused before anything is launched, the output untouched
    from map_geometry import GeoScenario
    g4 = GeoScenario.named(orc, "G4", beams=61, frac_nan=0.0)
    m4, sc4 = scanner_on(engine, g4, "lf")
    d4 = bpf.PlanarData(g4.ranges, g4.angles, g4.range_max)
    # no cell of G4 is further than 0.3 m from a wall: an empty space, no hits, no error
    assert sc4.searchSpace(7, 1) == (0, 0)
    assert sc4.searchPoses(d4, 7, 1, 8).shape[0] == 0
    sc4.setMapFactors(0.95, 0.95, 0.0)
    cells = sc4.searchSpace(1, 1)[1]
    assert cells > 4 and sc4.searchSpace(1 << 29, 1) == (cells << 29, cells)
    buf = np.frombuffer(bytearray(b"\xab" * (4 * 56)), dtype=hpf.POSE_HIT_DTYPE).copy()
    rc, n = _raw_search(engine, d4, 1 << 29, 1, 0, -1, 4, buf)
    assert rc == 8 and n == -7
    assert buf.tobytes() == b"\xab" * (4 * 56)
    assert sc4.searchPoses(d4, 3, 1, 8).shape[0] == 8  # and the engine goes on


def test_not_configured(orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_pose_check import _cloud_setup
    geo = geometry(orc, "G3")
    data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
    hits = np.zeros(8, dtype=hpf.POSE_HIT_DTYPE)
    e = bpf.Engine(0)
    try:
        # the map and its LUT, no planar model
        m = bpf.OccupancyMap(e, geo.res)
        m.setCells(geo.cells)
        m.setOrigin(geo.origin)
        m.setDistancesLUT(geo.lut, geo.max_dist)
        m.upload()
        assert _raw_search(e, data, 4, 1, 0, -1, 8, hits)[0] == 2
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
        assert _raw_search(e, data, 4, 1, 0, -1, 8, hits)[0] == 2
    finally:
        e.close()
    e = bpf.Engine(0)
    try:
        # only the cloud scanner configured
        keep = _cloud_setup(e, orc, 1000)
        assert _raw_search(e, data, 4, 1, 0, -1, 8, hits)[0] == 2
        del keep
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 6. cached lists
def test_a_new_map_or_radius_invalidates_the_cached_lists(orc):
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    try:
        g2, g3 = geometry(orc, "G2"), geometry(orc, "G3")
        m, sc = scanner_on(e, g2, "lf")
        for stride in (2, 1):
            sp = psr.Space.of(g2, 4, stride)
            hits = sc.searchPoses(blind_scan(g2), 4, stride, 32, 7)
            assert np.all(hits["score"] == 1.0)
            assert_rows_follow_model(hits, sp, 7 + np.arange(32, dtype=np.int64))
        # another geometry on the same engine: both lists are rebuilt
        m3, sc3 = scanner_on(e, g3, "lf")
        for stride in (2, 1):
            sp = psr.Space.of(g3, 4, stride)
            assert sc3.searchSpace(4, stride) == (sp.total, sp.ij.shape[0])
            hits = sc3.searchPoses(blind_scan(g3), 4, stride, 32, 7)
            assert np.all(hits["score"] == 1.0)
            assert_rows_follow_model(hits, sp, 7 + np.arange(32, dtype=np.int64))
        # another radius on the same map
        sc3.setMapFactors(g3.map_factors[0], g3.map_factors[1], 0.1)
        g3.map_factors = (g3.map_factors[0], g3.map_factors[1], 0.1)
        for stride in (2, 1):
            sp = psr.Space.of(g3, 4, stride)
            assert sp.ij.shape[0] > psr.Space.of(geometry(orc, "G3"), 4, stride).ij.shape[0]
            assert sc3.searchSpace(4, stride) == (sp.total, sp.ij.shape[0])
            hits = sc3.searchPoses(blind_scan(g3), 4, stride, 32, 7)
            assert np.all(hits["score"] == 1.0)
            assert_rows_follow_model(hits, sp, 7 + np.arange(32, dtype=np.int64))
    finally:
        e.close()
