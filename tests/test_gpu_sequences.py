"""Call order as a tested dimension: the committed operation sequences of tests/sequence_model.py on the engine, every
operation compared with the cache-free model (which computes leaf and bin counts, converged, the drand48 state and the
running averages itself and only ever takes weights -- and device-libm poses -- from the engine), then the same
sequence again without looking (nothing read until the end) and once more on a fresh engine: the final set, state,
stream, statistics and pose array of the three runs must be the same bits.  The module's engine is shared, so every
sequence starts on an engine with a history.

Sizes (read from the code, not guessed): 257 -- one block everywhere; 3000 -- k_stats_block (<= 4096 samples) and
the one-block resample (kFusedWindow = 4096); 6000 -- the general statistics form with the small resample tail
(M <= 8192) still in use; 12000 -- beyond that tail's hand-over (bpf_pf_update_resample, M <= 8192)."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sequence_model as sm  # noqa: E402
from scenario import Scenario, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
KNIFE_EDGE_SHARE = 0.05  # of the scoring operations, over all committed sequences


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(orc):
    return sm.World(orc)


def _driver(engine, world, spec):
    return sm.Driver(engine, world, spec["n"], pop=spec.get("pop"), fused=spec.get("fused", 1))


def _checked(engine, world, spec, tally):
    d = _driver(engine, world, spec)
    try:
        sm.run_checked(d, sm.Model(world, spec["n"], pop=spec.get("pop")), spec["ops"], tally)
        return d.final()
    finally:
        d.close()


def _blind(engine, world, spec):
    d = _driver(engine, world, spec)
    try:
        sm.run_blind(d, spec["ops"])
        return d.final()
    finally:
        d.close()


def _differing(a, b):
    return [k for k in a if not sm.same_bits(a[k], b[k])]


@pytest.mark.parametrize("name", sorted(sm.SEQUENCES))
def test_sequence_against_the_model_blind_and_on_a_fresh_engine(engine, world, name):
    import badger_amcl_amd as bpf
    spec = sm.SEQUENCES[name]
    # 1. every operation against the model
    observed = _checked(engine, world, spec, sm.Tally())
    # 2. observation independence: the same calls with nothing read in between
    blind = _blind(engine, world, spec)
    assert not _differing(observed, blind), ("observed and blind runs differ in", _differing(observed, blind))
    # 3. history independence: the same calls on an engine that has done nothing else
    fresh = bpf.Engine(0)
    try:
        cold = _blind(fresh, world, spec)
    finally:
        fresh.close()
    assert not _differing(observed, cold), ("warm and fresh engines differ in", _differing(observed, cold))


KNIFE_EDGE_SET = [name for name in sorted(sm.SEQUENCES) if not name.startswith("matrix_")]


def test_knife_edge_allowance_is_rarely_used(engine, world):
    """One particle per scoring operation may resolve a cell edge differently (test_gpu_parity.py); over the committed
    hand-written sequences at most 5 % of the scoring operations may need it.  Runs them itself (the checked run
    only: about a second on an MI355X), so the share does not depend on which other tests ran; tools/soak_sequences.py
    asserts the same share over its walks."""
    assert len(KNIFE_EDGE_SET) >= 25
    tally = sm.Tally()
    for name in KNIFE_EDGE_SET:
        _checked(engine, world, sm.SEQUENCES[name], tally)
    print("scoring operations %d, knife-edge uses %d" % (tally.scoring, tally.knife))
    assert tally.scoring >= 60
    assert tally.share() <= KNIFE_EDGE_SHARE


# ---------------------------------------------------------------------------------------------- sharded stage calls
class _WorldOfOne:
    """torch.distributed's part in ShardedFilter for one rank: every gather returns the contribution."""
    class ReduceOp:
        SUM, MIN = "sum", "min"

    @staticmethod
    def get_rank():
        return 0

    @staticmethod
    def get_world_size():
        return 1

    @staticmethod
    def get_backend():
        return "gloo"

    @staticmethod
    def all_gather(outs, src):
        outs[0].copy_(src)

    @staticmethod
    def all_reduce(t, op=None):
        return None


def test_normalising_twice_between_score_and_resample(engine, orc):
    """score -> normalise -> bpf_shard_build_cdf -> normalise again -> build and resample, world 1, the totals in
    device tensors: the first normalisation leaves the weights summing to 1/3 and a CDF of those is built, the second
    brings them to 1; the oracle resamples the twice-normalised weights.  This holds the ORDER to the oracle; it does
    not hold bpf_shard_normalize_dev's drop of an earlier CDF, and passes without it: with totals of the caller's the
    normalisation leaves tile sums only and bpf_shard_build_cdf always scans (it has a sum to leave), so nothing stale
    is within reach of the stage calls in one process -- the drop is held by the transitions' rule (DESIGN.md
    section 5)."""
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    n = 3000
    sc = Scenario(orc, size=200, n=n, beams=61, cloud="mixture", seed=3)
    m, scn, pf, data = sc.gpu_objects(engine, 61, "lf", min_samples=100, seed=17)
    dev = torch.device("cuda", 0)
    b = HipShardBackend(engine, scn, pf, dev)
    sf = ShardedFilter(b, _WorldOfOne, first_window=1024, exchange="collective")
    before = pf.getCurrentSet().samples.copy()
    assert b.score(data) is None
    total = b.local_total().clone()
    b.normalize(total * 3.0, n)
    b.build_cdf(sf.flags)
    third = float(b.local_sum().cpu()[0])
    assert abs(third - 1.0 / 3.0) < 1e-12
    b.normalize(torch.tensor([third], dtype=torch.float64, device=dev), n)
    sf.totals = None
    w = pf.getCurrentSet().samples.copy()
    want = before.copy()
    tot = sc.oracle_apply(sc.oracle_planar(61, "lf"), want, 0)
    assert (rel_err(w[:, 3], want[:, 3] / tot) > 1e-9).sum() <= 1 and abs(w[:, 3].sum() - 1.0) < 1e-12
    rng0 = pf.getRngState()
    sf.update_resample()
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0)
    opf.set_samples(w, leaf_count=0)
    opf.pf.rng = rng0
    out = opf.update_resample()
    got = pf.getCurrentSet().samples
    assert sf.sample_count == got.shape[0] == out.sample_count, "a resample drawn from the CDF of other weights"
    assert np.array_equal(got[:, :3], opf.samples[:out.sample_count, :3]), "a resample drawn from another CDF"
    assert (sf.leaf_count, sf.bin_count) == (out.leaf_count, out.node_count) and pf.getRngState() == opf.pf.rng
    assert int(sf.flags[0].cpu()) == 0  # no CDF miss


def test_sharded_statistics_stay_the_global_sets_when_a_cluster_is_light(orc):
    """Two ranks in one process, one prob-model update: all but one of the global set's clusters weigh less than the
    device sums resolve (weight < 4e12 x count x 2^-96).  The single engine evaluates such clusters again on the host;
    a rank of a sharded filter holds a slice only, so there the statistics must stay the GLOBAL set's: every rank the
    same bits, cluster count and counts the oracle's over the whole set, the heavy cluster within the device budget,
    and computeClusterStats / getMaxWeightPose the same bits before and after the clusters were asked for."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    n = 3000
    sc = Scenario(orc, size=200, n=n, beams=61, cloud="mixture", seed=3)
    cuts = [0, n // 2, n]
    engines = [bpf.Engine(0) for _ in range(2)]
    keep, pfs = [], []
    for r, e in enumerate(engines):
        shard = Scenario.__new__(Scenario)
        shard.__dict__.update(sc.__dict__)
        shard.samples = np.ascontiguousarray(sc.samples[cuts[r]:cuts[r + 1]])
        m, scn, pf, data = shard.gpu_objects(e, 61, "prob", min_samples=100, max_samples=n, seed=21)
        keep.append((m, scn, data))
        pfs.append(pf)
    f = LocalShardedFilter(pfs)
    try:
        f.load([sc.samples[cuts[r]:cuts[r + 1]] for r in range(2)])
        f.update_sensor(keep[0][2])
        whole = np.ascontiguousarray(np.concatenate(f.local_sets()))
        t = orc.KDTree()
        for k in range(n):
            t.insert_pose(whole[k, :3], whole[k, 3])
        want = t.cluster_stats(whole, n)
        light = want["weight"] < 4e12 * want["count"] * 2.0 ** -96
        assert light.sum() >= 10 and (~light).sum() >= 1
        first = (f.compute_cluster_stats(), f.get_max_weight_pose())
        assert first[0][0] == want["n"]
        per_rank = [[pf.getClusterStats(k) for k in range(want["n"])] for pf in pfs]
        assert sm.same_bits(per_rank[0], per_rank[1])
        assert all(pf.getClusterStats(want["n"]) is None for pf in pfs)
        for k in range(want["n"]):
            w, mean, cnt, cov = per_rank[0][k]
            assert cnt == want["count"][k]
            if not light[k]:
                assert np.allclose(w, want["weight"][k], rtol=1e-12, atol=1e-12)
                assert np.allclose(mean, want["mean"][k], rtol=1e-12, atol=1e-12)
                assert np.allclose(cov, want["cov"][k], rtol=1e-12, atol=1e-10, equal_nan=True)
        again = (f.compute_cluster_stats(), f.get_max_weight_pose())
        assert sm.same_bits(list(first[0]) + list(first[1]), list(again[0]) + list(again[1]))
        heavy = int(np.argmax(want["weight"]))
        assert np.allclose(again[1][0], want["weight"][heavy], rtol=1e-12)
        assert np.allclose(again[1][1], want["mean"][heavy], rtol=1e-12, atol=1e-12)
    finally:
        f.close()
        for e in engines:
            e.close()
