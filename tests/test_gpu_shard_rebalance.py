"""Rebalancing the slices of a sharded set (include/badger_pf.h, bpf_shard_rebalance_*): the slices go back to the even
split in global order and only the samples on the wrong rank move.  W engines on one device, through both bindings:
LocalShardedFilter.rebalance() (the one-call form over the local exchange) and ShardedFilter.rebalance() (the stage
functions, every rank on a thread of its own over the thread-based stand-in for torch.distributed).  The model is
shard_rebalance_ref.py; the reference for everything a rebalance must NOT change is the filter before the call, and for
the AUTO mode one engine holding the whole set, rotated by the in-place model's i_wrap."""
import os
import sys

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shard_in_place_ref as ipr  # noqa: E402
import shard_rebalance_ref as rbr  # noqa: E402
import test_gpu_shard_in_place as ip  # noqa: E402 -- the in-process harness: ThreadDist, run_ranks, Pool, cuts_for, cloud

pytestmark = pytest.mark.gpu

RNG0 = 0x1234ABCD5678
NOT_CONFIGURED, INVALID_ARGUMENT = 2, 1


@pytest.fixture(scope="module")
def pool(orc):
    """[0]: the single engine; [1 .. 8]: the ranks of the staged path (they run on torch's stream)."""
    p = ip.Pool(orc)
    yield p
    p.close()


@pytest.fixture(scope="module")
def lpool(orc):
    """[1 .. 8]: the ranks of the local world (streams of their own)."""
    p = ip.Pool(orc)
    yield p
    p.close()


def even(n, W):
    return [(n * (r + 1)) // W - (n * r) // W for r in range(W)]


def rank_state(pf):
    st = pf.getState()
    return (st.leaf_count, st.bin_count, st.converged, st.w_slow, st.w_fast, pf.getRngState())


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def local_sets(f):
    """The ranks' slices on the host (a rank without samples: an empty array; bpf_pf_get_samples takes none)."""
    return f.for_each_rank(lambda r, pf: ip.read_set(pf)[0])


def cat(parts):
    return np.concatenate([np.asarray(p).reshape(-1, 4) for p in parts])


# ---------------------------------------------------------------------------------------------------- the two paths
class LocalRun:
    """LocalShardedFilter on lpool's engines with slices loaded by hand (the global tree over the exchange)."""

    def __init__(self, lpool, samples, cuts, with_map=False, alpha=(0.0, 0.0), seed=None, **kw):
        from badger_amcl_amd.local_world import LocalShardedFilter
        import badger_amcl_amd.pf as hpf
        W, n = len(cuts) - 1, samples.shape[0]
        self.pfs = []
        for r in range(W):
            pf = lpool.filter(1 + r, n, min_samples=min(100, max(n // 2, 2)), alpha=alpha, with_map=with_map)
            pf.setResampleModel(1)
            if with_map:
                pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
                pf.setUniformPoseCheck(0.0, 0.5)
            if seed is None:
                pf.setRngState(RNG0)
            else:
                pf.srand48(seed)
            self.pfs.append(pf)
        self.f = LocalShardedFilter(self.pfs, **kw)
        self.f.load([samples[cuts[r]:cuts[r + 1]] for r in range(W)])

    def __enter__(self):
        return self.f

    def __exit__(self, *exc):
        self.f.shutdown()
        self.f.close()


def staged_ranks(pool, samples, cuts, body, with_map=False, alpha=(0.0, 0.0), seed=None, **kw):
    """ShardedFilter per rank over ThreadDist; body(sf, backend, rank) on every rank's thread, after the global tree's
    counts were installed in the engines (sf._global_tree, the bin-list route)."""
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    W, n = len(cuts) - 1, samples.shape[0]
    bs = []
    for r in range(W):
        pf = pool.filter(1 + r, n, min_samples=min(100, max(n // 2, 2)), alpha=alpha, with_map=with_map)
        pf.setResampleModel(1)
        if with_map:
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            pf.setUniformPoseCheck(0.0, 0.5)
        if seed is None:
            pf.setRngState(RNG0)
        else:
            pf.srand48(seed)
        ip.load_slice(pf, samples[cuts[r]:cuts[r + 1]], n)
        bs.append(HipShardBackend(pool.engines[1 + r], pool.scanner(1 + r)[0], pf, torch.device("cuda", 0)))

    def run(rank, dist):
        sf = ShardedFilter(bs[rank], dist, rank=rank, world=W, exchange="collective", init_follows=True, **kw)
        sf.leaf_count, sf.bin_count = sf._global_tree()
        return body(sf, bs[rank], rank)

    return ip.run_ranks(W, run)


# ---------------------------------------------------------------------------------------------------- 1. stand-alone
def _cases():
    out = []
    for W in (1, 2, 3, 8):
        for kind in (("even",) if W == 1 else ("even", "uneven", "empty")):
            out.append((1200, ip.cuts_for(1200, W, kind), "W%d-%s" % (W, kind)))
    out.append((1200, [0, 1, 1199, 1200], "W3-head-and-tail"))
    out.append((5, ip.cuts_for(5, 8, "even"), "W8-five-samples"))
    # 34 999 samples leave rank 1: more than the 64 x 256 threads of the pack grid and of the exchanges' copy grids, so
    # their grid-stride loops make a second and a third pass
    out.append((70000, [0, 1, 70000], "W2-70000"))
    return out


CASES = _cases()


def _check_after(samples, cuts, sets, slices, before, after, moved):
    W, n = len(cuts) - 1, samples.shape[0]
    counts = [cuts[r + 1] - cuts[r] for r in range(W)]
    pl = rbr.plan(counts)
    assert moved == [pl["moved"]] * W
    assert [s.shape[0] for s in sets] == even(n, W)
    got = cat(sets)
    assert got.shape == samples.shape and np.array_equal(u64(got), u64(samples))  # x, y, theta AND the weight, bit for bit
    # the model's assemble, rank by rank (a wrong row offset that happens to tile would show here)
    want, _ = rbr.rebalance([samples[cuts[r]:cuts[r + 1]] for r in range(W)])
    for r in range(W):
        assert np.array_equal(u64(sets[r].reshape(-1, 4)), u64(want[r])), r
        assert slices[r][:2] == (pl["Q"][r], pl["Q"][r + 1] - pl["Q"][r]), (r, slices[r])
        assert after[r] == before[r], (r, before[r], after[r])
    return pl


@pytest.mark.parametrize("n,cuts,name", CASES, ids=[c[2] for c in CASES])
def test_rebalance_one_call_over_the_local_exchange(lpool, n, cuts, name):
    samples = ip.cloud(n, "spread", seed=41)  # weights that are NOT uniform: a dropped or re-derived weight shows
    W = len(cuts) - 1
    with LocalRun(lpool, samples, cuts) as f:
        before = [rank_state(pf) for pf in f.pfs]
        assert before[0][0] > 0 and len(set(before)) == 1
        f.compute_cluster_stats()  # statistics in force: a rebalance that moves nothing must leave them in force
        x0 = f.exchange_counts()
        moved = f.rebalance()
        x1 = f.exchange_counts()
        pl = _check_after(samples, cuts, local_sets(f), [f.slice(r) for r in range(W)], before,
                          [rank_state(pf) for pf in f.pfs], [moved] * W)
        assert f.counts == even(n, W) and f.rebalanced == moved
        assert [b - a for a, b in zip(x0, x1)] == [2 if pl["moved"] else 1] * W
        f.compute_cluster_stats()
        x2 = f.exchange_counts()
        if pl["moved"] == 0:
            assert x2 == x1  # the set's epoch is untouched: the statistics are still in force, no exchange
        else:
            assert all(b > a for a, b in zip(x1, x2))  # evaluated again
        # a second rebalance finds the even split
        assert f.rebalance() == 0 and [b - a for a, b in zip(x2, f.exchange_counts())] == [1] * W


@pytest.mark.parametrize("n,cuts,name", CASES, ids=[c[2] for c in CASES])
def test_rebalance_stage_functions_over_threads(pool, n, cuts, name):
    samples = ip.cloud(n, "spread", seed=43)
    W = len(cuts) - 1

    def body(sf, b, rank):
        before = rank_state(b.pf)
        moved = sf.rebalance()
        s, _ = ip.read_set(b.pf)
        return dict(before=before, after=rank_state(b.pf), moved=moved, set=s, slice=b.slice(), counts=list(sf.counts),
                    rebalanced=sf.rebalanced, totals=sf.totals, again=sf.rebalance())

    recs = staged_ranks(pool, samples, cuts, body)
    assert recs[0]["before"][0] > 0
    _check_after(samples, cuts, [r["set"] for r in recs], [r["slice"] for r in recs], [r["before"] for r in recs],
                 [r["after"] for r in recs], [r["moved"] for r in recs])
    for r in recs:
        assert r["counts"] == even(n, W) and r["rebalanced"] == r["moved"] and r["totals"] is None and r["again"] == 0


# ---------------------------------------------------------------------------------------------------- 2. statistics
@pytest.mark.parametrize("n,W,kind", [(1200, 3, "uneven"), (5000, 8, "empty")])
def test_statistics_and_pose_array_after_a_rebalance(pool, lpool, n, W, kind):
    """get_max_weight_pose, compute_cluster_stats and get_pose_array of the rebalanced set equal, bit for bit, those of
    one engine holding the concatenation (the bar of the sharded statistics and pose-array tests)."""
    samples = ip.cloud(n, "blob", seed=47)
    samples[n // 2:, :2] += 3.0  # a second cluster
    pf1 = pool.filter(0, n)
    pf1.initWithSamples(samples, -1)
    nc1, mean1, cov1 = pf1.computeClusterStats()
    best1 = pf1.getMaxWeightPose()
    poses1 = pf1.getPoseArray(1, 3).copy()
    with LocalRun(lpool, samples, ip.cuts_for(n, W, kind)) as f:
        assert f.rebalance() > 0
        nc, mean, cov = f.compute_cluster_stats()
        assert f.stats_route == ("gathered" if n <= 4096 else "distributed")
        assert nc == nc1 and np.array_equal(mean, mean1) and np.array_equal(cov, cov1, equal_nan=True)
        best = f.get_max_weight_pose()
        assert best[0] == best1[0] and np.array_equal(best[1], best1[1])
        assert np.array_equal(u64(f.get_pose_array(root=-1, first=1, stride=3)), u64(poses1))


# ---------------------------------------------------------------------------------------------------- 3. AUTO
def _lopsided(n, W, heavy):
    """A spread cloud whose rank `heavy` (of the even split) holds a tight blob with most of the weight."""
    cuts = ip.cuts_for(n, W, "even")
    s = ip.cloud(n, "spread", seed=53)
    lo, hi = cuts[heavy], cuts[heavy + 1]
    s[lo:hi] = ip.cloud(hi - lo, "blob", seed=54)
    w = np.random.default_rng(55).random(n) + 1e-3
    w[lo:hi] *= 60.0
    s[:, 3] = w / w.sum()
    return s, cuts


@pytest.mark.parametrize("W", [3, 8])
def test_auto_rebalances_behind_the_in_place_resample(pool, W):
    n = 3000
    samples, cuts = _lopsided(n, W, heavy=1)
    rng = ip.state_for_u0(0.21)
    leaf = ip.tree_of(pool, samples, n, 0)[0]

    def body(sf, b, rank):
        b.pf.setRngState(rng)
        sf.leaf_count = leaf
        sf.update_resample()
        st = sf.state()
        s, est = ip.read_set(b.pf)
        return dict(set=s, M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count, eleaf=est.leaf_count,
                    ebins=est.bin_count, rng=b.pf.getRngState(), conv=st.converged, miss=st.cdf_miss,
                    counts=list(sf.counts), form=sf.form_used, windows=sf.windows_used, rebalanced=sf.rebalanced,
                    slice=b.slice())

    auto = staged_ranks(pool, samples, cuts, body, resample_form="in_place", rebalance="auto", trigger_share=1.0)
    off = staged_ranks(pool, samples, cuts, body, resample_form="in_place")
    pf1, S, st1, rng_after = ip.single_resample(pool, samples, n, 0, rng)
    M = st1.sample_count
    sums = []
    for q in range(W):
        acc = 0.0
        for w in samples[cuts[q]:cuts[q + 1], 3]:
            acc += float(w)
        sums.append(acc)
    P = ipr.plan(rng, M, 0, sums, False)  # max_share = 2.0, the default
    assert P["form"] == ipr.WINDOW and max(P["counts"]) > 2.0 * ((M + W - 1) // W)  # the cap would trip
    want = ipr.rotate(S, 0, P["i_wrap"])
    got = cat([r["set"] for r in auto])
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    assert np.all(got[:, 3] == 1.0 / M)
    leaf1, bins1 = ip.tree_of(pool, want, n, 0)
    T = rbr.plan(P["counts"])["moved"]
    assert T > 0
    for k, r in enumerate(auto):
        assert r["form"] == "in_place" and r["windows"] == 0 and r["rebalanced"] == T, k
        assert r["counts"] == even(M, W) and r["set"].shape[0] == even(M, W)[k], k
        assert r["slice"] == ((M * k) // W, even(M, W)[k], ipr.IN_PLACE), k
        assert (r["M"], r["rng"], r["conv"], r["miss"]) == (M, rng_after, st1.converged, False), k
        assert (r["leaf"], r["bins"]) == (r["eleaf"], r["ebins"]) == (leaf1, bins1), k
    # the behaviour that is kept: without AUTO the cap sends the same set to the window form
    for k, r in enumerate(off):
        assert r["form"] == "window" and r["windows"] == 1 and r["rebalanced"] == 0, k
        assert r["counts"] == even(M, W) and r["M"] == M, k
    assert np.array_equal(cat([r["set"] for r in off])[:, :3], S[:, :3])


@pytest.mark.parametrize("W", [3, 8])
def test_auto_one_call_on_a_set_whose_cap_would_trip(pool, lpool, W):
    """The one-call form (bpf_shard_update_resample, local exchange) on a blob + spread mixture: rank 1 of the even
    split holds a tight blob around the true pose, the sensor update gives it nearly all the weight, and the cap at the
    default max_share would send this resample to the window form (checked with the in-place model from the single
    engine's weights).  With AUTO at trigger_share = 1 it stays in place: five exchanges, no window, even counts, the
    single engine's set rotated.  With rebalance="off" the same set reports the window form."""
    from badger_amcl_amd import synth
    sc = pool.scenario()
    n = 3000
    cuts = ip.cuts_for(n, W, "even")
    samples = ip.cloud(n, "spread", seed=57)
    samples[cuts[1]:cuts[2]] = synth.converged_cloud(cuts[2] - cuts[1], sc.pose, seed=58, sigma=(0.05, 0.05, 0.02))
    samples[:, 3] = 1.0 / n
    pf1, od, scn, data = ip.single_with_map(pool, samples, (0.0, 0.0))
    scn.updateSensor(pf1, data)
    w1 = ip.read_set(pf1)[0]
    rng0 = pf1.getRngState()
    pf1.updateResample()
    S, st1 = ip.read_set(pf1)
    M, rng_after = st1.sample_count, pf1.getRngState()
    P = ipr.plan(rng0, M, 0, [float(np.sum(w1[cuts[q]:cuts[q + 1], 3])) for q in range(W)], True)
    assert P["form"] == ipr.WINDOW and max(P["counts"]) > 2.0 * ((M + W - 1) // W)  # the cap would trip
    cdf = np.concatenate([[0.0], np.cumsum(w1[:, 3])])
    gap = np.min(np.abs(np.asarray(P["targets"])[:, None] - cdf[None, :]))
    assert gap > 1e-9, gap  # no tooth within rounding of a CDF edge (the ranks add the same weights in another order)
    want = ipr.rotate(S, 0, P["i_wrap"])
    leaf1, bins1 = ip.tree_of(pool, want, n, 0)
    with LocalRun(lpool, samples, cuts, with_map=True, seed=21, resample_form="in_place", rebalance="auto",
                  trigger_share=1.0) as f:
        f.update_sensor(lpool.scanner(1)[1])
        x0 = f.exchange_counts()
        f.update_resample()
        assert [b - a for a, b in zip(x0, f.exchange_counts())] == [5] * W
        assert f.form_used == "in_place" and f.windows_used == 0 and not f.cdf_miss
        assert f.rebalanced == rbr.plan(P["counts"])["moved"] > 0
        sets = local_sets(f)
        got = cat(sets)
        assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3]) and np.all(got[:, 3] == 1.0 / M)
        assert f.counts == even(M, W) == [s.shape[0] for s in sets]
        assert [f.slice(r) for r in range(W)] == [((M * r) // W, even(M, W)[r], ipr.IN_PLACE) for r in range(W)]
        assert (f.sample_count, f.leaf_count, f.bin_count) == (M, leaf1, bins1)
        assert set(f.rng_states()) == {rng_after}
        for r, pf in enumerate(f.pfs):
            est = pf.getState()
            assert (est.leaf_count, est.bin_count, est.converged) == (leaf1, bins1, st1.converged), r
    with LocalRun(lpool, samples, cuts, with_map=True, seed=21, resample_form="in_place") as f:
        f.update_sensor(lpool.scanner(1)[1])
        f.update_resample()
        assert f.form_used == "window" and f.windows_used == 1 and f.rebalanced == 0 and f.counts == even(M, W)
        assert np.array_equal(cat(local_sets(f))[:, :3], S[:, :3])


# ---------------------------------------------------------------------------------------------------- 3. + 4. cycles
@pytest.mark.parametrize("W", [3, 8])
def test_two_cycles_with_auto_on_a_rebalanced_filter(pool, lpool, W):
    """An uneven load, a stand-alone rebalance, then motion, sensor update and resample twice with AUTO at
    trigger_share = 1 through the one-call forms: five exchanges per resample that rebalances.  One engine is fed the
    rotated set between the rounds, as in test_two_cycles_on_the_uneven_slices, with its bars: motion within 1e-12,
    the normalised weights within 1e-9 relative, the resample exact.  Precondition, from the single engine's CDF: no
    target within 1e-9 of a CDF edge."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    sc = pool.scenario()
    n = 3000
    samples = synth.converged_cloud(n, sc.pose, seed=33)
    cuts = ip.cuts_for(n, W, "uneven")
    pf1, od, scn, data = ip.single_with_map(pool, samples, (0.0, 0.0))
    with LocalRun(lpool, samples, cuts, with_map=True, seed=21, resample_form="in_place", rebalance="auto",
                  trigger_share=1.0) as f:
        for r in range(W):
            o = bpf.Odom(lpool.engines[1 + r])
            o.setModel(*ip.ODOM)
        assert f.rebalance() == rbr.plan([cuts[r + 1] - cuts[r] for r in range(W)])["moved"] > 0
        ldata = lpool.scanner(1)[1]
        for k in range(2):
            f.update_action(None, bpf.OdomData(*ip.ODATA))
            od.updateAction(pf1, bpf.OdomData(*ip.ODATA))
            moved, moved1 = cat(local_sets(f)), ip.read_set(pf1)[0]
            assert moved.shape == moved1.shape and np.max(np.abs(moved - moved1)) <= 1e-12, k
            f.update_sensor(ldata)
            scn.updateSensor(pf1, data)
            w, w1 = cat(local_sets(f)), ip.read_set(pf1)[0]
            assert np.array_equal(w[:, :3], w1[:, :3])
            assert np.max(np.abs(w[:, 3] - w1[:, 3]) / w1[:, 3]) <= 1e-9
            rng0 = pf1.getRngState()
            x0 = f.exchange_counts()
            f.update_resample()
            x1 = f.exchange_counts()
            pf1.updateResample()
            S, st1 = ip.read_set(pf1)
            M = st1.sample_count
            targets, i_wrap, _ = ipr.target_chain(rng0, M)
            cdf = np.concatenate([[0.0], np.cumsum(w1[:, 3])])
            gap = np.min(np.abs(np.asarray(targets)[:, None] - cdf[None, :]))
            assert gap > 1e-9, gap  # the precondition
            want = ipr.rotate(S, 0, i_wrap)
            sets = local_sets(f)
            got = cat(sets)
            assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3]), k
            assert np.all(got[:, 3] == 1.0 / M)
            assert f.form_used == "in_place" and f.windows_used == 0 and not f.cdf_miss
            assert f.counts == even(M, W) == [s.shape[0] for s in sets]
            assert [b - a for a, b in zip(x0, x1)] == [5 if f.rebalanced else 4] * W
            if k == 0:
                assert f.rebalanced > 0  # the even slices of a converged cloud do not resample to even ones
            rng_after = pf1.getRngState()
            pf1.initWithSamples(want, -1)  # the rotated set: what the ranks hold
            pf1.setRngState(rng_after)
            st = pf1.getState()
            assert (f.sample_count, f.leaf_count, f.bin_count) == (M, st.leaf_count, st.bin_count)
            assert set(f.rng_states()) == {rng_after} and f.state().converged == st1.converged
            for r, pf in enumerate(f.pfs):
                est = pf.getState()
                assert (est.leaf_count, est.bin_count, est.converged) == (st.leaf_count, st.bin_count, st1.converged), r
            best, best1 = f.get_max_weight_pose(), pf1.getMaxWeightPose()
            assert best[0] == best1[0] and np.array_equal(best[1], best1[1])


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_stage_calls_refuse_what_they_cannot_do(pool):
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend
    n = 600
    pf = pool.filter(1, n)
    pf.setResampleModel(1)
    s = ip.cloud(n, "blob", seed=19)
    pf.initWithSamples(s[:400])
    b = HipShardBackend(pool.engines[1], None, pf, torch.device("cuda", 0))

    def code(fn):
        with pytest.raises(bpf.BpfError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: b.set_rebalance(1, 0.5)) == INVALID_ARGUMENT
    assert code(lambda: b.set_rebalance(1, float("nan"))) == INVALID_ARGUMENT
    assert code(lambda: b.set_rebalance(2, 1.5)) == INVALID_ARGUMENT
    assert b.rebalance_setting() == (0, 1.5)  # the default: off, and a policy value
    b.set_rebalance(1, 1.0)
    assert b.rebalance_setting() == (1, 1.0)
    b.set_rebalance(0, 1.5)
    assert code(lambda: b.rebalance_export()) == NOT_CONFIGURED  # no plan
    assert code(lambda: b.rebalance_plan([399, 201], 0, 2)) == INVALID_ARGUMENT  # counts[rank] != sample_count
    assert code(lambda: b.rebalance_plan([400] + [0] * 16, 0, 17)) == INVALID_ARGUMENT
    assert code(lambda: b.rebalance_plan([400, 200], 2, 2)) == INVALID_ARGUMENT
    assert code(lambda: b.rebalance_plan([400, -1], 0, 2)) == INVALID_ARGUMENT
    assert code(lambda: b.rebalance_plan([400, 201], 0, 2)) == INVALID_ARGUMENT  # G > max_samples
    out, first, cnt = b.rebalance_plan([400, 200], 0, 2)
    assert (out, first, cnt) == ([100, 0], 0, 300)
    pf.initWithSamples(s[:400])  # the set changed between plan and export: the plan is stale
    assert code(lambda: b.rebalance_export()) == NOT_CONFIGURED
    rows = torch.zeros((2, 4, 100), dtype=torch.int64, device="cuda")
    assert code(lambda: b.rebalance_import(rows, [0, 400], 100)) == NOT_CONFIGURED
    got, st = ip.read_set(pf)
    assert st.sample_count == 400 and np.array_equal(u64(got), u64(s[:400]))


def test_one_call_resample_after_a_rebalance_needs_new_totals(pool, lpool):
    """A rebalance between a sensor update and a resample keeps the normalised weights and drops the W totals: the
    one-call resample answers NOT_CONFIGURED and leaves the set alone; w_slow / w_fast stay."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    sc = pool.scenario()
    n, W = 1200, 3
    samples = synth.converged_cloud(n, sc.pose, seed=35)
    cuts = ip.cuts_for(n, W, "uneven")
    with LocalRun(lpool, samples, cuts, with_map=True, alpha=(0.001, 0.1), seed=21, resample_form="in_place") as f:
        f.update_sensor(lpool.scanner(1)[1])
        scored = cat(local_sets(f))
        before = [rank_state(pf) for pf in f.pfs]
        assert before[0][3] > 0.0 and before[0][4] > 0.0  # w_slow, w_fast
        assert f.rebalance() > 0
        assert [rank_state(pf) for pf in f.pfs] == before
        held = cat(local_sets(f))
        assert np.array_equal(u64(held), u64(scored))
        with pytest.raises(bpf.BpfError) as ei:
            f.update_resample()
        assert ei.value.code == NOT_CONFIGURED
        assert np.array_equal(u64(cat(local_sets(f))), u64(held)) and f.counts == even(n, W)
        assert [rank_state(pf) for pf in f.pfs] == before
