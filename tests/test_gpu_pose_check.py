"""Node::uniformPoseGenerator's score check (bpf_pf_set_uniform_pose_check, AS_REFERENCE: K rejected trials per call)
and the 3-D free-space generator on the device, against the Python restatement in pose_check_ref.py (itself pinned
to the oracle in test_pose_check_cpu.py): the oracle side resamples the device's own scored set, so only the random
pose injection and the resampling are under test.  Poses bit for bit, M, leaf and bin counts, the drand48 state and
the reset of w_slow / w_fast."""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pose_check_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CHECKS = [(0.8, 0.5), (10.0, 0.0), (10.0, 0.5), (10.0, 0.99)]
ALPHA = (0.001, 0.1)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _planar_free_space(sc_):
    return ref.FreeSpace.planar(ref.free_cells_2d(sc_.cells, sc_.lut, sc_.map_factors[2]), sc_.size, sc_.size,
                                sc_.origin, sc_.res)


def _check_init(orc, pf, fs, g0, m, n):
    rng0 = pf.getRngState()
    pf.initWithRandomPoses()
    r = ref.Rng(rng0)
    want = np.array(ref.init_with_pose_fn(r, n, ref.FastGen(fs, g0, m)))
    got = pf.getCurrentSet().samples
    st = pf.getState()
    assert st.sample_count == n
    assert np.array_equal(got[:, :3], want)
    assert np.all(got[:, 3] == 1.0 / n)
    assert pf.getRngState() == r.s
    t = orc.KDTree()
    for p in want:
        t.insert_pose(p, 1.0)
    assert st.leaf_count == t.leaf_count()
    assert st.w_slow == 0.0 and st.w_fast == 0.0


def _check_resample(orc, pf, opf, fs, g0, m, resampler, gen=None):
    """One pf.updateResample() against the restatement (gen: the pose generator, AS_REFERENCE by default);
    returns w_diff."""
    cur = pf.getCurrentSet().samples.copy()
    st0 = pf.getState()
    w_diff = 1.0 - st0.w_fast / st0.w_slow if st0.w_slow != 0.0 else 0.0
    if not (w_diff >= 0.0):
        w_diff = 0.0
    rng0 = pf.getRngState()
    pf.updateResample()
    st1 = pf.getState()
    r = ref.Rng(rng0)
    want, leaf, nodes, rnd = ref.resample(cur, st0.leaf_count, w_diff, r, gen or ref.FastGen(fs, g0, m), resampler,
                                          opf, orc.KDTree)
    M = len(want)
    assert st1.w_diff == w_diff
    assert st1.sample_count == M, (w_diff, g0, m)
    assert st1.leaf_count == leaf and st1.bin_count == nodes
    after = pf.getCurrentSet().samples
    assert np.array_equal(after[:, :3], np.array(want))
    assert np.all(after[:, 3] == 1.0 / M)
    assert pf.getRngState() == r.s
    if w_diff > 0:
        assert st1.w_slow == 0.0 and st1.w_fast == 0.0  # particle_filter.cpp:453-455
        assert sum(rnd) > 0
    return w_diff


@pytest.mark.parametrize("n", [2000, 100000])
@pytest.mark.parametrize("g0,m", CHECKS)
def test_init_with_random_poses_as_reference(engine, orc, n, g0, m):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    sc_ = Scenario(orc, size=200, n=256, beams=61)
    m_, sc, _, _ = sc_.gpu_objects(engine, 61, "lf")
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
    pf.srand48(17)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    pf.setUniformPoseCheck(g0, m)
    _check_init(orc, pf, _planar_free_space(sc_), g0, m, n)


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("device_kld", [False, True])
@pytest.mark.parametrize("g0,m", CHECKS)
def test_recovery_resample_as_reference(engine, orc, resampler, device_kld, g0, m):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    n = 2500
    sc_ = Scenario(orc, size=200, n=n, beams=61, cloud="mixture")
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 1 if device_kld else 8192)
    try:
        m_, sc, pf, data = sc_.gpu_objects(engine, 61, "lf", min_samples=100, seed=31, alpha=ALPHA)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.setUniformPoseCheck(g0, m)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=31)
        fs = _planar_free_space(sc_)
        scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0)]
        w_diffs = [0.0]
        for ranges in scans:
            sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
            w_diffs.append(_check_resample(orc, pf, opf, fs, g0, m, resampler))
        assert max(w_diffs) > 0.01
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
        engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 8192)


def test_unknown_scoring_is_refused(engine):
    import badger_amcl_amd as bpf
    pf = bpf.ParticleFilter(engine, 100, 500, 0.0, 0.0, 85.0)
    with pytest.raises(bpf.BpfError) as ei:
        pf.setUniformPoseCheck(10.0, 0.5, 7)
    assert ei.value.code == 1


class _OracleScore:
    """scorePose as the parameter documents it: the weight of the one-sample set {pose, 1.0} after
    applyModelToSampleSet with set->converged = 0, by the oracle; records every (score, threshold) comparison."""

    def __init__(self, orc, sc_, model, beams):
        self.orc, self.sc_ = orc, sc_
        self.p = sc_.oracle_planar(beams, model)
        self.ranges = None
        self.seen = []

    def __call__(self, pose):
        one = np.array([[pose[0], pose[1], pose[2], 1.0]])
        self.orc.planar_apply(self.p, self.sc_.omap, one, self.ranges, self.sc_.angles, self.sc_.range_max, 0)
        return float(one[0, 3])


def _sensor_gen(fs, g0, m, scorer):
    def gen(rng):
        good = g0
        p = fs.pose(rng)
        s = scorer(p)
        scorer.seen.append((s, good))
        while s < good:
            p = fs.pose(rng)
            good *= m
            s = scorer(p)
            scorer.seen.append((s, good))
        return p
    return gen


def _no_knife_edges(seen):
    s = np.array([a for a, _ in seen])
    t = np.array([b for _, b in seen])
    close = np.abs(s - t) <= 1e-9 * np.abs(t)
    assert not close.any(), "a score within 1e-9 of its threshold: pick another seed"


@pytest.mark.parametrize("model", ["lf", "beam", "prob", "gompertz"])
@pytest.mark.parametrize("resampler", [0, 1])
def test_sensor_model_matches_oracle_scores(engine, orc, model, resampler):
    """BPF_POSE_CHECK_SENSOR_MODEL: init after a scan, then recovery resamples, against the reference's loop run
    over oracle scores of the last scan."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    n, beams = 2000, 61
    # (no NaN ranges: the beam model's weight of a scan with one is NaN for every pose, and a NaN score accepts)
    sc_ = Scenario(orc, size=200, n=n, beams=beams, cloud="mixture", frac_nan=0.0)
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    try:
        m_, sc, pf, data = sc_.gpu_objects(engine, beams, model, min_samples=100, seed=29, alpha=ALPHA)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        fs = _planar_free_space(sc_)
        scorer = _OracleScore(orc, sc_, model, beams)
        # a threshold among the scores of random free-space poses: calls reject a varying number of trials
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
        pf.initWithSamples(sc_.samples)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=29)
        scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(beams, 1.0)]
        w_diffs = []
        for ranges in scans:
            sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
            scorer.ranges = ranges
            w_diffs.append(_check_resample(orc, pf, opf, fs, g0, mult, resampler,
                                           gen=_sensor_gen(fs, g0, mult, scorer)))
        assert max(w_diffs) > 0.0  # (_check_resample then also saw random draws)
        _no_knife_edges(scorer.seen)
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)


def test_sensor_model_without_a_scan_is_as_reference(engine, orc):
    """no scan since bpf_map2d_set: every score is 1.0, so the result is AS_REFERENCE's (K = 4 for (10, 0.5))"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    sc_ = Scenario(orc, size=200, n=256, beams=61)
    m_, sc, _, data = sc_.gpu_objects(engine, 61, "lf")
    pf = bpf.ParticleFilter(engine, 100, 2000, 0.0, 0.0, 85.0)
    pf.srand48(23)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    pf.setUniformPoseCheck(10.0, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)
    _check_init(orc, pf, _planar_free_space(sc_), 10.0, 0.5, 2000)
    # a scan, then a new map: the scan is gone again
    sc.updateSensor(pf, data)
    m_.setDistancesLUT(sc_.lut, sc_.max_dist)
    m_.upload()
    _check_init(orc, pf, _planar_free_space(sc_), 10.0, 0.5, 2000)


def test_sensor_model_refused_where_out_of_scope(orc):
    """the cloud scanner and the sharded path take AS_REFERENCE only"""
    import ctypes as C
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    e = bpf.Engine(0)
    try:
        om, sc, pts, s, fs = _cloud_setup(e, orc, 1000)
        pf = bpf.ParticleFilter(e, 100, 1000, 0.0, 0.0, 85.0)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.setUniformPoseCheck(10.0, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)
        with pytest.raises(bpf.BpfError) as ei:
            pf.initWithRandomPoses()
        assert ei.value.code == 4
        wd, cnt = C.c_double(), C.c_int()
        assert e.lib.bpf_shard_begin_resample(e.h, C.c_uint64(pf.getRngState()), 10, C.byref(wd), C.byref(cnt)) == 4
    finally:
        e.close()


def _cloud_setup(engine, orc, n):
    import badger_amcl_amd as bpf
    from test_gpu_cloud import _setup
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, n, 8, 256, seed=4)
    om = bpf.OctoMap(engine, 0.05)
    om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
    sc = bpf.PointCloudScanner(engine)
    sc.init(128, om)
    sc.setPointCloudModel(0.5, 0.05, 0.1)
    sc.setMapFactors(0.95, 0.95, 0.3)
    sc.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
    fs = ref.FreeSpace.octo(list(lut.min_cells), list(lut.max_cells), 0.05)
    return om, sc, pts, s, fs


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("g0,m", [(0.0, 0.5), (10.0, 0.5)])
def test_free_space_3d_generator(orc, resampler, g0, m):
    """BPF_RANDOM_POSE_FREE_SPACE_3D on an engine with the 3-D map only (no 2-D map): init, then recovery resamples
    after point-cloud updates, K = 0 and K = 4."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    e = bpf.Engine(0)  # an engine that never saw a 2-D map
    try:
        n = 2000
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        om, sc, pts, s, fs = _cloud_setup(e, orc, n)
        pf = bpf.ParticleFilter(e, 100, n, ALPHA[0], ALPHA[1], 85.0)
        pf.srand48(11)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.setUniformPoseCheck(g0, m)
        assert ref.retries(g0, m) in (0, 4)
        _check_init(orc, pf, fs, g0, m, n)
        pf.initWithSamples(s)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=11)
        w_diffs = []
        for scan in (pts, pts * np.float32(0.5), pts * np.float32(0.3)):
            assert sc.updateSensor(pf, bpf.PointCloudData(np.ascontiguousarray(scan)))
            w_diffs.append(_check_resample(orc, pf, opf, fs, g0, m, resampler))
        assert max(w_diffs) > 0.01
    finally:
        e.close()


def test_capacity_leaves_the_filter_untouched(engine, orc):
    """(10, 0.999999): K ~ 2.3 M; 1000 calls do not fit 31-bit stream positions."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    sc_ = Scenario(orc, size=200, n=1000, beams=61)
    m_, sc, pf, data = sc_.gpu_objects(engine, 61, "lf", min_samples=100, seed=3)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    pf.setUniformPoseCheck(10.0, 0.999999)
    before = pf.getCurrentSet().samples.copy()
    rng0 = pf.getRngState()
    with pytest.raises(bpf.BpfError) as ei:
        pf.initWithRandomPoses()
    assert ei.value.code == 8
    assert np.array_equal(pf.getCurrentSet().samples, before)
    assert pf.getRngState() == rng0
    pf.setUniformPoseCheck(0.0, 0.5)
    pf.initWithRandomPoses()  # and the filter goes on as before
    assert pf.getState().sample_count == 1000


# ---------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARD_CHECK = (10.0, 0.5)  # K = 4


def _shard_scenario():
    # the scenario of test_gpu_sharded.py::test_two_ranks_recovery_random_poses, whose weight totals the two ranks
    # reproduce bit for bit (the averages are compared exactly)
    from oracle import pyoracle as orc
    from scenario import Scenario
    return orc, Scenario(orc, size=400, n=6000, beams=181, cloud="mixture")


def _shard_scans(sc):
    return [sc.ranges, np.clip(sc.ranges * 0.6, 0.05, 29.0), np.full(sc.ranges.shape[0], 1.0)]


def _attach_3d_map(e):
    """a small 3-D map on a planar engine: the 3-D generator needs nothing else"""
    import badger_amcl_amd as bpf
    mn, mx = np.array([-40, -30, 0], dtype=np.int32), np.array([60, 50, 3], dtype=np.int32)
    cols = int((mx[0] - mn[0] + 1) * (mx[1] - mn[1] + 1))
    nz = int(mx[2] - mn[2] + 1)
    om = bpf.OctoMap(e, 0.05)
    om.setDistancesLUT(np.zeros(cols, dtype=np.uint32), np.zeros(nz, dtype=np.uint8), mn, mx, 0.3)
    return om, ref.FreeSpace.octo(list(mn), list(mx), 0.05)


def _shard_worker(rank, world, port, out_dir, resampler, gen3d):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    from scenario import Scenario
    orc, sc = _shard_scenario()
    n = sc.samples.shape[0]
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world
    e = bpf.Engine(0)
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    m, scn, pf, data = shard.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21, alpha=ALPHA)
    om = _attach_3d_map(e)[0] if gen3d else None
    pf.setResampleModel(resampler)
    sf = ShardedFilter(HipShardBackend(e, scn, pf, torch.device("cuda", 0)), dist, first_window=1024)
    sf.set_random_pose_generator(hpf.RANDOM_POSE_FREE_SPACE_3D if gen3d else hpf.RANDOM_POSE_FREE_SPACE_2D)
    sf.set_uniform_pose_check(*SHARD_CHECK)
    recs = []
    for ranges in _shard_scans(sc):
        sf.update_sensor(bpf.PlanarData(ranges, sc.angles, sc.range_max))
        sf.update_resample()
        st = sf.state()
        recs.append(dict(samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                         rng=pf.getRngState(), w_slow=st.w_slow))
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(recs, dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    del om
    e.close()


@pytest.mark.parametrize("gen3d", [False, True])
@pytest.mark.parametrize("resampler", [0, 1])
def test_two_ranks_pose_check_equals_single_engine(tmp_path, resampler, gen3d):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_shard_worker, args=(2, port, str(tmp_path), resampler, gen3d), nprocs=2, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r), allow_pickle=True) for r in range(2)]
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    orc, sc = _shard_scenario()
    n = sc.samples.shape[0]
    e = bpf.Engine(0)
    try:
        m, scn, pf, data = sc.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21, alpha=ALPHA)
        om, fs3 = _attach_3d_map(e) if gen3d else (None, None)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D if gen3d else hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.setUniformPoseCheck(*SHARD_CHECK)
        w_diffs = []
        for cycle, ranges in enumerate(_shard_scans(sc)):
            scn.updateSensor(pf, bpf.PlanarData(ranges, sc.angles, sc.range_max))
            pf.updateResample()
            st = pf.getState()
            w_diffs.append(st.w_diff)
            cur = pf.getCurrentSet().samples
            for r in (recs[0][cycle], recs[1][cycle]):
                assert r["M"] == st.sample_count and r["leaf"] == st.leaf_count and r["rng"] == pf.getRngState()
                if gen3d:
                    # (the random poses differ from the 2-D case, so the set the next scan scores differs, and the two
                    # ranks' partial weight totals can round differently from the one engine's sum in the last bit;
                    # the averages are the subject of test_gpu_sharded.py, the random poses and the stream this one's)
                    assert r["w_slow"] == pytest.approx(st.w_slow, rel=1e-13, abs=0.0)
                else:
                    assert r["w_slow"] == st.w_slow
            merged = np.concatenate([recs[0][cycle]["samples"], recs[1][cycle]["samples"]])
            assert np.array_equal(merged[:, :3], cur[:, :3])
        assert max(w_diffs) > 0.01
    finally:
        e.close()
