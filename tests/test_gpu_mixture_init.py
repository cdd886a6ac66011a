"""Mixture initialiser on the device (include/badger_pf.h, bpf_pf_init_with_mixture and its sharded forms) against
the oracle: K successive orc_pf_init_with_gaussian calls on consecutive slices of one sample array, sharing the rng.

Exact: the drand48 state, the weights, w_slow / w_fast / converged, the leaf and bin counts (of the DEVICE poses, as
tests/test_gpu_motion.py::test_init_with_gaussian_matches_oracle compares them), and every pin that needs no device
log: equal components against initWithGaussian, zero-sigma components against their means, slices against the single
engine.  Poses: within POSE_TOL, the allowance of tests/test_gpu_motion.py for the same expression.

Sizes: a Gaussian tile is 2048 attempts (about 536 samples), the device tree starts at 8192 samples, a wave is 64
samples and a block 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_init.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mixture_oracle as mo  # noqa: E402
from scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-12  # tests/test_gpu_motion.py
RNG0 = 0xABCDEF12330E
INVALID, NOT_CONFIGURED = 1, 2
ZEROS = {1: (), 2: (), 7: (0, 3, 4, 6), 64: (0, 30, 31, 63), 100: (), 1024: ()}
CASES = [(n, k) for n in (1, 63, 64, 65, 257, 700, 5000, 10000) for k in (1, 2, 7, 64)] + [(1024, 1024), (5000, 1024),
                                                                                             (37, 100)]


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def case_components(n, k):
    if (n, k) == (1024, 1024):
        comps = mo.components(n, k, seed=5)
        comps["count"] = 1
        return comps
    return mo.components(n, k, seed=n + k, zeros=ZEROS[k])


def new_filter(engine, n, kld=0, rng=RNG0):
    import badger_amcl_amd as bpf
    pf = bpf.ParticleFilter(engine, 10, n, 0.001, 0.1, 85.0)
    pf.setKldCount(kld)
    pf.setRngState(rng)
    return pf


def oracle_counts(orc, poses, kld):
    t = orc.KDTree()
    for r in poses[:, :3]:
        t.insert_pose(r, 1.0)
    return (t.leaf_count(), t.node_count()) if kld == 0 else (t.node_count(), t.node_count())


@pytest.mark.parametrize("n,k", CASES)
def test_matches_the_oracle(engine, orc, n, k):
    comps = case_components(n, k)
    assert int(comps["count"].sum()) == n
    if k in (7, 64) and n >= 257:
        assert all(comps["count"][i] == 0 for i in ZEROS[k]) and (comps["count"] > 0).sum() >= 2
    opf = orc.ParticleFilter(10, n, 0.001, 0.1, 85.0)
    opf.pf.rng = RNG0
    want = mo.oracle_init_with_mixture(orc, opf, comps)
    first = None
    for kld in (0, 1):
        pf = new_filter(engine, n, kld)
        pf.initWithMixture(comps)
        st = pf.getState()
        got = pf.getCurrentSet().samples
        assert st.sample_count == n and pf.getRngState() == opf.pf.rng
        err = np.abs(got[:, :3] - want[:, :3]).max()
        print("n %d k %d kld %d: max pose error %.3g" % (n, k, kld, err))
        assert err <= POSE_TOL
        assert np.all(got[:, 3] == 1.0 / n)
        assert st.w_slow == 0.0 and st.w_fast == 0.0 and st.converged == 0
        assert (st.leaf_count, st.bin_count) == oracle_counts(orc, got, kld)
        if first is None:
            first = got.tobytes()
        assert got.tobytes() == first  # two runs give identical bytes


@pytest.mark.parametrize("n,k", [(1, 1), (64, 2), (700, 7), (5000, 64), (10000, 1), (5000, 1024)])
def test_equal_components_are_init_with_gaussian(engine, n, k):
    same = ((12.5, -3.25, 0.8), [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], (0.5, 0.2, 0.1))
    comps = mo.components(n, k, seed=3 * n + k, zeros=ZEROS[k], same=same)
    pf = new_filter(engine, n)
    pf.initWithGaussian(*same)
    want, rng, st1 = pf.getCurrentSet().samples.copy(), pf.getRngState(), pf.getState()
    pf = new_filter(engine, n)
    pf.initWithMixture(comps)
    st = pf.getState()
    assert pf.getCurrentSet().samples.tobytes() == want.tobytes() and pf.getRngState() == rng
    assert (st.leaf_count, st.bin_count) == (st1.leaf_count, st1.bin_count)


def boundary_counts():
    """Counts whose boundaries fall inside a wave, at lane 63 / 64, at sample 255 / 256 and around the first
    Gaussian tile's edge (near sample 536: every boundary from 520 to 552 is one)."""
    counts = [3, 61, 1, 63, 128, 7, 249] + [8] + [1] * 32
    assert np.cumsum(counts)[:8].tolist() == [3, 64, 65, 128, 256, 263, 512, 520]
    return counts + [700 - sum(counts), 300]


def test_zero_sigma_components_pin_every_boundary(engine, orc):
    counts = boundary_counts()
    n, k = sum(counts), len(counts)
    # one live component at a time, then live and dead alternating both ways: every listed boundary has a live
    # component on one side and a dead one on the other, so the sigma k_mixture_gauss picks is pinned at each
    for live in ({0}, {6}, {k - 1}, set(range(0, k, 2)), set(range(1, k, 2))):
        comps = mo.components(n, k, seed=11)
        comps["count"] = counts
        for i in range(k):
            if i not in live:
                comps[i]["sigma"] = 0.0
        pf = new_filter(engine, n)
        pf.initWithMixture(comps)
        got = pf.getCurrentSet().samples
        owner = np.repeat(np.arange(k), counts)
        dead = ~np.isin(owner, sorted(live))
        assert got[dead, :3].tobytes() == comps["mean"][owner[dead]].tobytes()
        assert np.all(np.all(got[~dead, :3] != comps["mean"][owner[~dead]], axis=1))
        # the draws still consumed their uniforms: the stream is where the oracle's is
        opf = orc.ParticleFilter(10, n, 0.001, 0.1, 85.0)
        opf.pf.rng = RNG0
        want = mo.oracle_init_with_mixture(orc, opf, comps)
        assert pf.getRngState() == opf.pf.rng and np.abs(got[:, :3] - want[:, :3]).max() <= POSE_TOL


def test_the_stream_goes_on(engine, orc):
    """After the init one motion update, one sensor update and one resample follow the oracle's."""
    import badger_amcl_amd as bpf
    n = 5000
    sc_ = Scenario(orc, size=400, n=n, beams=91, cloud="converged")
    m, sc, pf, data = sc_.gpu_objects(engine, 91, "lf", min_samples=100, seed=21)
    comps = mo.components(n, 7, seed=2, zeros=(0, 3, 4, 6))
    comps["mean"][:, :2] = np.asarray(sc_.pose[:2]) + np.random.default_rng(4).uniform(-0.3, 0.3, (7, 2))
    comps["mean"][:, 2] = sc_.pose[2]
    comps["sigma"] = (0.1, 0.1, 0.03)
    pf.initWithMixture(comps)
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0, seed=21)
    want = mo.oracle_init_with_mixture(orc, opf, comps)
    assert pf.getRngState() == opf.pf.rng
    dev = pf.getCurrentSet().samples
    assert np.abs(dev[:, :3] - want[:, :3]).max() <= POSE_TOL
    od = bpf.Odom(engine)
    od.setModel(bpf.pf.ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.05, 0.05, 0.05)
    odata = bpf.OdomData((1.0, 2.0, 0.3), (0.02, 0.01, 0.01))
    opf.set_samples(dev)  # from the DEVICE poses on both sides
    od.updateAction(pf, odata)
    cur = opf.samples[:n]
    opf.pf.rng = orc.odom_update_action(2, (0.05, 0.05, 0.05, 0.05, 0.0), odata.pose, odata.delta,
                                        odata.absolute_motion, cur, opf.pf.rng)
    assert pf.getRngState() == opf.pf.rng
    dev = pf.getCurrentSet().samples
    assert np.abs(dev[:, :3] - opf.samples[:n, :3]).max() <= POSE_TOL
    # (the tree stays the one of the poses the set was created with: the leaf count goes along)
    leaf = opf.leaf_count
    opf.set_samples(dev, leaf_count=leaf)
    sc.updateSensor(pf, data)
    pf.updateResample()
    p = sc_.oracle_planar(91, "lf")
    opf.update_sensor(lambda s, conv: sc_.oracle_apply(p, s, conv))
    out = opf.update_resample()
    assert pf.getState().sample_count == out.sample_count and pf.getRngState() == opf.pf.rng
    assert np.array_equal(pf.getCurrentSet().samples[:, :3], opf.samples[:out.sample_count, :3])


def _raw(engine, comps, k, null=False):
    from badger_amcl_amd import _lib
    ptr = None if null else comps.ctypes.data_as(C.POINTER(_lib.MixtureComponent))
    return engine.lib.bpf_pf_init_with_mixture(engine.h, ptr, k)


def bad_tables(n):
    good = mo.components(n, 4, seed=1)
    assert np.all(good["count"] > 0)
    out = []
    for field, index, value in [("mean", 0, np.nan), ("mean", 2, np.inf), ("rotation", (1, 1), np.nan),
                                ("rotation", (2, 0), -np.inf), ("sigma", 1, np.nan), ("sigma", 2, np.inf)]:
        c = good.copy()
        c[1][field][index] = value
        out.append((c, 4, field))
    c = good.copy()
    c["count"][0] -= 1
    out.append((c, 4, "sum below"))
    c = good.copy()
    c["count"][3] += 1
    out.append((c, 4, "sum above"))
    c = good.copy()
    c["count"][0] += c["count"][1] + 1
    c["count"][1] = -1
    out.append((c, 4, "negative count"))
    out.append((good, 0, "k = 0"))
    out.append((good, -1, "k < 0"))
    out.append((np.concatenate([good] + [np.zeros(1021, dtype=good.dtype)]), 1025, "k = 1025"))
    return good, out


def test_refusals_leave_everything_untouched(engine):
    import badger_amcl_amd as bpf
    n = 700
    good, bad = bad_tables(n)
    pf = new_filter(engine, n)
    pf.initWithMixture(good)
    before, rng0, st0 = pf.getCurrentSet().samples.copy(), pf.getRngState(), pf.getState()
    for comps, k, what in bad:
        assert _raw(engine, np.ascontiguousarray(comps), k) == INVALID, what
    assert _raw(engine, good, 4, null=True) == INVALID
    assert engine.lib.bpf_pf_init_with_mixture(None, good.ctypes.data_as(C.POINTER(bpf._lib.MixtureComponent)),
                                               4) == INVALID
    st = pf.getState()
    assert pf.getCurrentSet().samples.tobytes() == before.tobytes() and pf.getRngState() == rng0
    assert (st.leaf_count, st.bin_count, st.sample_count) == (st0.leaf_count, st0.bin_count, st0.sample_count)
    # a non-finite field of a component WITHOUT samples is not read
    c = good.copy()
    c["count"][0] += c["count"][1]
    c["count"][1] = 0
    c[1]["mean"], c[1]["sigma"], c[1]["rotation"] = np.nan, np.inf, np.nan
    pf.initWithMixture(c)
    assert np.all(np.isfinite(pf.getCurrentSet().samples))
    e2 = bpf.Engine(0)
    try:
        assert _raw(e2, good, 4) == NOT_CONFIGURED
        ptr = good.ctypes.data_as(C.POINTER(bpf._lib.MixtureComponent))
        assert e2.lib.bpf_shard_init_with_mixture(e2.h, ptr, 4, 0, n, n) == NOT_CONFIGURED
        assert e2.lib.bpf_shard_init_with_mixture_all(e2.h, ptr, 4) == NOT_CONFIGURED
    finally:
        e2.close()


# ---------------------------------------------------------------------------------------------------- end to end
def test_search_refine_seed_track_planar(engine, orc):
    """searchPoses -> refinePoses -> mixtureFromHits -> initWithMixture -> sensor update + resample cycles.  The
    max-weight pose agrees with the oracle run of the same components to the tolerance of a cycle in
    tests/sequence_model.py (1e-12, relative and absolute) and lies within one cell and one search heading step of the
    true pose; tests/test_pose_mixture_cpu.py checks with the oracle alone that the scenario allows that."""
    import badger_amcl_amd as bpf
    sc_ = mo.e2e_scenario(orc)
    m, sc, pf, data = sc_.gpu_objects(engine, mo.E2E_BEAMS, "lf", min_samples=100, seed=mo.E2E_SEED)
    hits = sc.searchPoses(data, mo.E2E_HEADINGS, mo.E2E_STRIDE, mo.E2E_HITS)
    R, A, L = mo.E2E_REFINE
    xy_step, theta_step = mo.e2e_refine_steps(sc_.res)
    rows = sc.refinePoses(data, hits, R, xy_step, A, theta_step, L)
    xy, th = mo.e2e_merge(sc_.res)
    comps, src, merged = bpf.mixtureFromHits(rows, mo.E2E_N, xy, th, mo.E2E_CAP, mo.E2E_SIGMA)
    assert comps.shape[0] == mo.E2E_CAP and int(comps["count"].sum()) == mo.E2E_N
    pf.initWithMixture(comps)
    opf = orc.ParticleFilter(100, mo.E2E_N, 0.0, 0.0, 85.0, seed=mo.E2E_SEED)
    want = mo.oracle_init_with_mixture(orc, opf, comps)
    dev = pf.getCurrentSet().samples
    assert pf.getRngState() == opf.pf.rng and np.abs(dev[:, :3] - want[:, :3]).max() <= POSE_TOL
    opf.set_samples(dev)  # from the DEVICE poses on both sides, as tests/test_gpu_motion.py continues
    p = sc_.oracle_planar(mo.E2E_BEAMS, "lf")
    for _ in range(mo.E2E_CYCLES):
        sc.updateSensor(pf, data)
        pf.updateResample()
        opf.update_sensor(lambda s, conv: sc_.oracle_apply(p, s, conv))
        out = opf.update_resample()
        assert pf.getState().sample_count == out.sample_count and pf.getRngState() == opf.pf.rng
    w, pose = pf.getMaxWeightPose()
    ow, opose = mo.oracle_max_weight_pose(orc, opf.samples[:opf.sample_count])
    print("max-weight pose", pose, "oracle", opose, "truth", sc_.pose, "weights", w, ow)
    assert np.allclose(pose, opose, rtol=1e-12, atol=1e-12) and np.allclose(w, ow, rtol=1e-12, atol=1e-12)
    assert mo.within_e2e_bound(pose, np.asarray(sc_.pose, dtype=np.float64), sc_.res)


def test_search_refine_seed_track_cloud(orc):
    """The same chain with the cloud scanner on the 3-D map: the room, cloud, mounting and model of
    tests/test_gpu_pose_search_cloud.py at its smallest shape (8 headings, stride 2).  The cycles are
    mixture_oracle.E2E_CLOUD_CYCLES, for the reason given there."""
    import badger_amcl_amd as bpf
    import test_gpu_pose_search_cloud as tpc
    scene = mo.CloudScene(orc)
    H = mo.E2E_CLOUD_HEADINGS
    e = bpf.Engine(0)
    try:
        om, sc = tpc.scanner_on(e, scene.lut, scene.tf_xyz, scene.tf_quat, scene.max_dist, "plain",
                                mo.E2E_CLOUD_BEAMS)
        data = bpf.PointCloudData(scene.points)
        pf = bpf.ParticleFilter(e, 100, mo.E2E_N, 0.0, 0.0, 85.0)
        pf.srand48(mo.E2E_SEED)
        hits = sc.searchPoses(data, H, mo.E2E_STRIDE, mo.E2E_HITS)
        R, A, L = mo.E2E_REFINE
        xy_step, theta_step = mo.e2e_refine_steps(scene.res, H)
        rows = sc.refinePoses(data, hits, R, xy_step, A, theta_step, L)
        xy, th = mo.e2e_merge(scene.res, H)
        comps, src, merged = bpf.mixtureFromHits(rows, mo.E2E_N, xy, th, mo.E2E_CAP, mo.E2E_SIGMA)
        assert comps.shape[0] == mo.E2E_CAP and int(comps["count"].sum()) == mo.E2E_N
        pf.initWithMixture(comps)
        opf = orc.ParticleFilter(100, mo.E2E_N, 0.0, 0.0, 85.0, seed=mo.E2E_SEED)
        want = mo.oracle_init_with_mixture(orc, opf, comps)
        dev = pf.getCurrentSet().samples
        assert pf.getRngState() == opf.pf.rng and np.abs(dev[:, :3] - want[:, :3]).max() <= POSE_TOL
        opf.set_samples(dev)  # from the DEVICE poses on both sides
        for _ in range(mo.E2E_CLOUD_CYCLES):
            sc.updateSensor(pf, data)
            pf.updateResample()
            opf.update_sensor(lambda s, conv: scene.oracle_apply(scene.op, s, conv))
            out = opf.update_resample()
            assert pf.getState().sample_count == out.sample_count and pf.getRngState() == opf.pf.rng
        w, pose = pf.getMaxWeightPose()
        ow, opose = mo.oracle_max_weight_pose(orc, opf.samples[:opf.sample_count])
        print("max-weight pose", pose, "oracle", opose, "truth", scene.truth, "weights", w, ow)
        assert np.allclose(pose, opose, rtol=1e-12, atol=1e-12) and np.allclose(w, ow, rtol=1e-12, atol=1e-12)
        assert mo.within_e2e_bound(pose, scene.truth, scene.res, H)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- sharded
@pytest.fixture(scope="module")
def pool():
    import test_gpu_shard_init as tsi
    p = tsi.Pool()
    yield p
    p.close()


def mixture_cuts(n, W, split, prefix):
    """test_gpu_shard_init.splits, with the first inner cut moved onto a component boundary ("boundary")."""
    import test_gpu_shard_init as tsi
    if split != "boundary":
        return tsi.splits(n, W, split)
    cuts = tsi.splits(n, W, "even")
    for r in range(1, W):
        cuts[r] = int(prefix[np.searchsorted(prefix, cuts[r])])  # the first boundary at or after the even cut
    return [int(v) for v in np.maximum.accumulate(cuts)]


@pytest.mark.parametrize("split", ["even", "ragged", "empty", "boundary"])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("kld", [0, 1])
def test_shards_equal_one_engine(pool, orc, kld, W, split):
    import test_gpu_shard_init as tsi
    n, k = 6000, 7
    comps = mo.components(n, k, seed=9, zeros=(0, 3, 4, 6))
    prefix = np.concatenate([[0], np.cumsum(comps["count"])])
    cuts = mixture_cuts(n, W, split, prefix)
    assert cuts[0] == 0 and cuts[-1] == n and len(cuts) == W + 1 and all(b >= a for a, b in zip(cuts, cuts[1:]))
    inner = set(cuts[1:-1])
    if split == "boundary" and W > 1:
        assert inner <= set(prefix.tolist())
    if split == "even" and W > 1:
        assert inner - set(prefix.tolist())  # a cut inside a component
    pf1 = pool.filter(0, orc, 400, n)
    bs = tsi.make_ranks(pool, orc, W, 400, n)
    for pf in [pf1] + [b.pf for b in bs]:
        pf.setKldCount(kld)
    pf1.initWithMixture(comps)
    for r, b in enumerate(bs):
        lo, cnt = cuts[r], cuts[r + 1] - cuts[r]
        b.init_mixture(comps, lo, cnt, n)
        st = b.pf.getState()
        assert (st.sample_count, st.leaf_count, st.bin_count) == (cnt, -1, -1)  # the tree is marked as not built
    counts = tsi.global_tree(bs, cuts)
    want, st1 = tsi.check_against_single(bs, cuts, pf1, counts, (kld, W, split))
    assert (st1.leaf_count, st1.bin_count) == tsi.oracle_counts(orc, want, kld)


def test_sharded_refusals(pool, orc):
    import test_gpu_shard_init as tsi
    import badger_amcl_amd as bpf
    n = 700
    good, bad = bad_tables(n)
    b = tsi.make_ranks(pool, orc, 1, 400, n)[0]
    b.init_mixture(good, 0, n, n)
    before, rng0 = b.pf.getCurrentSet().samples.copy(), b.pf.getRngState()
    for comps, k, what in bad:
        ptr = np.ascontiguousarray(comps).ctypes.data_as(C.POINTER(bpf._lib.MixtureComponent))
        assert b.e.lib.bpf_shard_init_with_mixture(b.e.h, ptr, k, 0, n, n) == INVALID, what
    for args in [(0, n - 1, n - 1), (0, n, n + 1), (1, n, n), (-1, 5, n)]:
        with pytest.raises(bpf.BpfError) as ei:
            b.init_mixture(good, *args)
        assert ei.value.code == INVALID, args
    assert b.e.lib.bpf_shard_init_with_mixture(b.e.h, None, 4, 0, n, n) == INVALID
    assert b.pf.getCurrentSet().samples.tobytes() == before.tobytes() and b.pf.getRngState() == rng0


@pytest.mark.parametrize("W", [2, 3])
def test_sharded_filter_method(pool, orc, W):
    """ShardedFilter.init_with_mixture on the harness of test_gpu_shard_init.py (W filters in W threads, the exchange
    by torch ops): the even shares concatenate to the single engine's set, with its rng state and tree counts."""
    import test_gpu_shard_init as tsi
    from badger_amcl_amd.sharded import ShardedFilter
    n = 6000
    comps = mo.components(n, 7, seed=9, zeros=(0, 3, 4, 6))
    pf1 = pool.filter(0, orc, 400, n)
    bs = tsi.make_ranks(pool, orc, W, 400, n)
    for pf in [pf1] + [b.pf for b in bs]:
        pf.setKldCount(0)

    def body(rank, dist):
        sf = ShardedFilter(bs[rank], dist, rank=rank, world=W, first_window=1024, exchange="collective",
                           init_follows=True)
        sf.init_with_mixture(comps)
        return dict(init=tsi.read_set(bs[rank].pf)[0], leaf=sf.leaf_count, bins=sf.bin_count, counts=list(sf.counts),
                    rng=bs[rank].pf.getRngState(), total=sf.sample_count)

    recs = tsi.run_ranks(W, body)
    pf1.initWithMixture(comps)
    s0, st0 = tsi.read_set(pf1)
    assert np.concatenate([r["init"] for r in recs]).tobytes() == s0.tobytes()
    for r in recs:
        assert (r["leaf"], r["bins"], r["rng"], r["total"]) == (st0.leaf_count, st0.bin_count, pf1.getRngState(), n)
        assert r["counts"] == [(n * (k + 1)) // W - (n * k) // W for k in range(W)]


# ---------------------------------------------------------------------------------------------------- local world
_REF = {}


def _world_reference(orc, resampler):
    import badger_amcl_amd as bpf
    import test_gpu_local_world as tlw
    if resampler not in _REF:
        sc = tlw._cycle_scenario(orc)
        comps = _world_components(sc)
        e, scn, pf, data, od = tlw._single(sc, resampler=resampler)
        try:
            pf.initWithMixture(comps)
            st0 = pf.getState()
            start = dict(samples=pf.getCurrentSet().samples.copy(), leaf=st0.leaf_count, bins=st0.bin_count,
                         rng=pf.getRngState())

            def step(c):
                od.updateAction(pf, bpf.OdomData(*tlw.ODATA))
                scn.updateSensor(pf, data)
            _REF[resampler] = (start, tlw._single_cycles(pf, 1, step))
        finally:
            e.close()
    return _REF[resampler]


def _world_components(sc):
    import test_gpu_local_world as tlw
    comps = mo.components(tlw.N, 7, seed=6, zeros=(0, 3, 4, 6))
    comps["mean"][:, :2] = np.asarray(sc.pose[:2]) + np.random.default_rng(8).uniform(-0.2, 0.2, (7, 2))
    comps["mean"][:, 2] = sc.pose[2]
    comps["rotation"] = np.eye(3)
    comps["sigma"] = tlw.INIT_SIGMA
    return comps


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("resampler", [0, 1])
def test_local_world_then_one_cycle(orc, resampler, W):
    """bpf_shard_init_with_mixture_all over the local world: the slices concatenate to the single engine's set, the
    tree counts and the rng agree, and one cycle from there equals the single engine's under the cap of
    tests/test_gpu_local_world.py::_check_cycles."""
    import badger_amcl_amd as bpf
    import test_gpu_local_world as tlw
    sc = tlw._cycle_scenario(orc)
    start, ref = _world_reference(orc, resampler)
    w = tlw.World(sc, W, resampler=resampler)
    try:
        w.f.init_with_mixture(_world_components(sc))
        assert np.array_equal(np.concatenate(w.f.local_sets()), start["samples"])
        assert (w.f.leaf_count, w.f.bin_count) == (start["leaf"], start["bins"])
        assert w.f.rng_states() == [start["rng"]] * W

        def step(c):
            w.f.update_action(None, bpf.OdomData(*tlw.ODATA))
            w.f.update_sensor(w.data)
        tlw._check_cycles(tlw._world_cycles(w.f, 1, step), ref, W)
    finally:
        w.close()
