"""The copies that go through the engine's pinned bounce buffer since every host-device copy lives in host_copy.hpp
(the KLD limit table, the cluster list, the gathered slices of the host-statistics route, the local self-test, the
candidate scores): one case each, with a payload that takes more than one piece of the buffer (kBounceHalf = 2 MiB)
where the public interface can reach one, checked against what the other tests already treat as truth.  They check
that the right bytes arrive across the piece boundary; they are not detectors of the intermittent fault the bounce
buffer was built for, and nothing here repeats a run."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py

from badger_amcl_amd import _lib, synth

pytestmark = pytest.mark.gpu

PIECE = 2 << 20  # kBounceHalf


# ------------------------------------------------------------------------------------------------ the limit table
LIMIT_N = 524300  # (LIMIT_N + 1) ints = 2 MiB + 52 B: two pieces


def _two_thousand_bins(n, seed):
    """A 16 m x 16 m patch, headings within two bins: 2048 histogram bins.  The KLD bound for the leaves the first
    window of 4096 draws sees then lies more than kld_device_min = 8192 draws ahead, at the default pop_err and at
    twice that, so the whole stream goes to the device tree; and it lies far below n."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    s[:, 0] = rng.uniform(10.0, 26.0, n)
    s[:, 1] = rng.uniform(20.0, 36.0, n)
    s[:, 2] = rng.uniform(0.01, 0.3, n)
    s[:, 3] = rng.uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    return s


def _resample_against_oracle(orc, samples, pop):
    """test_gpu_parity.py's checks of one multinomial resample whose stop the device tree finds, on an engine of its
    own (created here, destroyed here)."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_parity import _oracle_resample_from
    n = samples.shape[0]
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)  # no draw on a summation-order knife edge (test_gpu_parity.py)
        pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
        pf.srand48(7)
        pf.setResampleModel(0)
        if pop:
            pf.setPopulationSizeParameters(*pop)
        pf.initWithSamples(samples)  # the set's tree: ensure_limit_table(n) with n = max_samples
        st0 = pf.getState()
        pf.updateResample()          # the device tree over the whole stream [0, max_samples)
        after, st1, rng1 = pf.getCurrentSet().samples, pf.getState(), pf.getRngState()
    finally:
        e.close()
    # no sensor update has run: w_slow = w_fast = 0; the oracle is given equal averages, as in
    # test_resample_of_degenerate_weight_vectors_matches_oracle
    opf, out = _oracle_resample_from(orc, samples, 1.0, 1.0, st0.leaf_count, 7, 0, 100, n, pop)
    assert out.status == 0 and st1.last_status == 0
    M = out.sample_count
    assert 4096 + 8192 < M < n and st1.kld_on_device == 1
    assert (st1.sample_count, st1.leaf_count, st1.bin_count) == (M, out.leaf_count, out.node_count)
    assert np.array_equal(after[:, :3], opf.samples[:M, :3])
    assert np.all(after[:, 3] == 1.0 / M)
    assert rng1 == opf.pf.rng
    return M


def test_limit_table_of_two_pieces_and_rebuilt_for_the_next_engine(orc):
    assert (LIMIT_N + 1) * 4 > PIECE
    s = _two_thousand_bins(LIMIT_N, 3)
    first = _resample_against_oracle(orc, s, None)
    # a second engine, made after the first is gone, with another pop_err: ITS table, not an inherited one
    second = _resample_against_oracle(orc, s, (0.02, 3.0))
    assert second < first


# ------------------------------------------------------------------------------------------------ the cluster list
def test_cluster_list_of_two_pieces_matches_oracle(orc):
    """One sample per histogram bin on a lattice of every second bin: every sample is a cluster of its own, and the
    list of them is longer than one piece.  Counts exact; weights, means and covariances within the budget
    test_gpu_next_rows.py's _assert_stats_equal gives the device evaluation."""
    import badger_amcl_amd as bpf
    from test_gpu_next_rows import _oracle_stats
    from test_gpu_shard_stats import read_stats
    need = PIECE // C.sizeof(_lib.Cluster) + 1
    side = int(np.ceil(np.sqrt(need)))
    n = side * side
    assert n * C.sizeof(_lib.Cluster) > PIECE
    ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    rng = np.random.default_rng(17)
    s = np.zeros((n, 4))
    s[:, 0] = ii.reshape(-1) + 0.25
    s[:, 1] = jj.reshape(-1) + 0.25
    s[:, 2] = 0.02
    s[:, 3] = rng.uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    s = np.ascontiguousarray(s[rng.permutation(n)])
    want = _oracle_stats(orc, s, n)
    assert want["n"] == n
    e = bpf.Engine(0)
    try:
        pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
        pf.initWithSamples(s)
        got = read_stats(pf)
    finally:
        e.close()
    assert int(got["n"][0]) == n
    assert np.array_equal(got["count"], np.asarray(want["count"]))
    assert np.allclose(got["weight"], want["weight"], rtol=1e-12, atol=1e-12)
    assert np.allclose(got["mean"], np.asarray(want["mean"]).reshape(n, 3), rtol=1e-12, atol=1e-12)
    assert np.allclose(got["cov"], np.asarray(want["cov"]).reshape(n, 5), rtol=1e-12, atol=1e-10, equal_nan=True)
    k = int(np.argmax(want["weight"]))
    assert np.allclose(got["best_w"][0], want["weight"][k], rtol=1e-12, atol=1e-12)
    assert np.allclose(got["best_pose"], want["mean"][k], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the gathered slices
def test_gathered_slices_of_two_pieces_on_the_host_route(orc):
    """A local world of 2 ranks, host statistics: 4 rows x 66 000 doubles come down into a std::vector in two pieces.
    The same bits on every rank as one engine holding the whole set."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    from test_gpu_local_world import _world_stats
    from test_gpu_shard_stats import assert_same_bits, reference_stats
    W, n = 2, 66000
    assert 4 * 8 * n > PIECE
    pose = np.array([10.0, 12.0, 0.3])
    blobs = [synth.converged_cloud(n // 3, pose + off, seed=5 + i, sigma=(0.15, 0.15, 0.05))
             for i, off in enumerate([(0, 0, 0), (4.0, -2.0, 1.0), (-3.0, 3.5, -2.0)])]
    whole = np.ascontiguousarray(np.concatenate(blobs))
    whole[:, 3] = np.random.default_rng(9).uniform(0.5, 1.5, n)
    whole[:, 3] /= whole[:, 3].sum()
    engines = [bpf.Engine(0) for _ in range(W + 1)]
    try:
        pfs = [bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0) for e in engines[:W]]
        for e in engines[:W]:
            e.set_option(hpf.OPT_STATS_HOST, 1)
        f = LocalShardedFilter(pfs)
        f.load([whole[:n // 2], whole[n // 2:]], tree=False)
        want = reference_stats(engines[W], whole, host=True)
        got = _world_stats(f)
        assert f.stats_route == "host"
        for r in range(W):
            assert_same_bits(got[r], want, r)
        f.close()
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ the local self-test
def test_local_selftest_at_the_first_world_size_beyond_a_megabyte():
    """World size 6: the receive vector of the widest ragged gather ((6 * 4096 + 3 + r) words from each of five
    ranks, guards) is the first to pass 1 MB.  One round; every cell is compared inside the call."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    W = 6
    engines = [bpf.Engine(0) for _ in range(W)]
    try:
        pfs = [bpf.ParticleFilter(e, 100, 3000, 0.0, 0.0, 85.0) for e in engines]
        f = LocalShardedFilter(pfs)
        f.selftest(1)
        f.close()
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ the candidate scores
def test_candidate_scores_of_the_largest_reachable_batch(orc):
    """BPF_POSE_CHECK_SENSOR_MODEL scores its trial poses in windows of kScoreWindow = 16 384 whatever the settings:
    the largest batch that comes down is 16 384 doubles = 128 KiB, one piece; a batch of 262 145 is not reachable.
    Every call here fetches such a batch.  An init with the scored check against the reference's loop over oracle
    scores, as test_gpu_pose_check.py::test_sensor_model_matches_oracle_scores checks it."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    import pose_check_ref as ref
    from scenario import Scenario
    from test_gpu_pose_check import _OracleScore, _no_knife_edges, _planar_free_space, _sensor_gen
    n, beams = 300, 61
    sc_ = Scenario(orc, size=200, n=n, beams=beams, cloud="mixture", frac_nan=0.0)
    e = bpf.Engine(0)
    try:
        m_, sc, pf, data = sc_.gpu_objects(e, beams, "lf", min_samples=100, seed=29, alpha=(0.001, 0.1))
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        fs = _planar_free_space(sc_)
        scorer = _OracleScore(orc, sc_, "lf", beams)
        scorer.ranges = sc_.ranges
        probe = ref.Rng(12345)
        sample = sorted(scorer(fs.pose(probe)) for _ in range(200))
        g0, mult = max(sample[180], 1e-300), 0.5
        pf.setUniformPoseCheck(g0, mult, hpf.POSE_CHECK_SENSOR_MODEL)
        sc.updateSensor(pf, data)  # the scan scorePose uses
        rng0 = pf.getRngState()
        pf.initWithRandomPoses()
        got, rng1 = pf.getCurrentSet().samples, pf.getRngState()
    finally:
        e.close()
    r = ref.Rng(rng0)
    want = np.array(ref.init_with_pose_fn(r, n, _sensor_gen(fs, g0, mult, scorer)))
    assert np.array_equal(got[:, :3], want)
    assert rng1 == r.s
    assert len(scorer.seen) > n  # some trials were rejected
    _no_knife_edges(scorer.seen)
