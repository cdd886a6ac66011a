"""The multinomial resample of a sharded set in place (include/badger_pf.h, bpf_shard_set_multinomial_form): every rank
keeps the candidate draws of its own slice, the stop index comes from the merged bin lists, and the concatenation of the
ranks' new slices is the set ONE engine produces, sorted stably by the owner of each sample's source particle.

Two drivers: ShardedFilter on W engines in W threads, stage by stage over a thread-based stand-in for
torch.distributed (weights set by hand, the slices from the gathered CDF sums), and LocalShardedFilter, whose ranks
enter the engine's one-call form over the local exchange (the slices from the totals of a sensor update).

The reference is one engine holding the whole set (bpf_pf_update_resample).  The clouds' poses are pairwise distinct, so
a pose of the new set names its source particle and with it the rank that holds the source; random poses of the
recovery draws are rank 0's.  Every comparison first requires that the WINDOW form on the same input equals the single
engine bit for bit: a seed for which a draw falls within rounding of a slice edge would fail there, not here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_check_ref as pcr  # noqa: E402
import shard_in_place_mn_ref as mnr  # noqa: E402
from scenario import Scenario  # noqa: E402
from test_gpu_shard_in_place import Pool, load_slice, read_set, run_ranks, single_resample, tree_of  # noqa: E402

pytestmark = pytest.mark.gpu

ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))
EXCHANGES = 4  # per in-place resample: the (count, flag) words, the bin lists, the limb words, the converged count


@pytest.fixture(scope="module")
def pool(orc):
    p = Pool(orc)
    yield p
    p.close()


def cloud(n, kind, seed, extent=8.0):
    """blob: stops early with min_samples = 100 (about 1 800 of 3 000); spread: no stop.  Pairwise distinct poses."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    if kind == "blob":
        s[:, 0], s[:, 1], s[:, 2] = rng.normal(3.0, 0.3, n), rng.normal(-2.0, 0.3, n), rng.normal(0.3, 0.1, n)
    elif kind == "tight":  # a handful of bins: the bound on the BIN count is passed early too
        s[:, 0], s[:, 1], s[:, 2] = rng.normal(3.0, 0.05, n), rng.normal(-2.0, 0.05, n), rng.normal(0.3, 0.02, n)
    else:
        s[:, 0], s[:, 1] = rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n)
        s[:, 2] = rng.uniform(-np.pi, np.pi, n)
    w = rng.random(n) ** 2 + 1e-3
    s[:, 3] = w / w.sum()
    assert len(set(map(tuple, s[:, :3]))) == n  # a pose names its source
    return s


def cuts_for(n, W, kind):
    if kind == "even" or W == 1:
        return [(n * r) // W for r in range(W + 1)]
    if kind == "uneven":
        return {3: [0, 1, (5 * n) // 12, n], 4: [0, 1, 3, (5 * n) // 12, n]}[W]
    if kind == "empty":  # one shard without samples
        return {3: [0, n // 3, n // 3, n], 4: [0, 0, n // 3, (2 * n) // 3, n]}[W]
    raise ValueError(kind)


def permuted(S, source_set, cuts):
    """The single engine's new set sorted stably by the rank that holds each sample's source (a pose that is not in the
    source set is a random pose: rank 0); and every rank's count."""
    where = {tuple(p): i for i, p in enumerate(source_set[:, :3])}
    src = [where.get(tuple(p), -1) for p in S[:, :3]]
    owner = np.array(mnr.owner_of_sources(src, cuts))
    perm = np.argsort(owner, kind="stable")
    W = len(cuts) - 1
    return S[perm], [int(np.sum(owner == q)) for q in range(W)]


def mn_sharded(pool, samples, cuts, max_samples, kld, rng_state, min_samples=100, form="in_place", max_share=None,
               rebalance="off", leaf=0):
    """ShardedFilter (multinomial resampler) on W engines, one resample from slices loaded by hand, stage by stage."""
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    W = len(cuts) - 1
    bs = []
    for r in range(W):
        pf = pool.filter(1 + r, max_samples, min_samples)
        pf.setResampleModel(0)
        pf.setKldCount(kld)
        pf.setRngState(rng_state)
        load_slice(pf, samples[cuts[r]:cuts[r + 1]], samples.shape[0])
        bs.append(HipShardBackend(pool.engines[1 + r], None, pf, torch.device("cuda", 0)))

    def body(rank, dist):
        b = bs[rank]
        sf = ShardedFilter(b, dist, rank=rank, world=W, exchange="collective", init_follows=True,
                           multinomial_form=form, max_share=float(W) if max_share is None else max_share,
                           rebalance=rebalance)
        sf.leaf_count = leaf
        sf.update_resample()
        st = sf.state()
        s, est = read_set(b.pf)
        return dict(set=s, M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count, eleaf=est.leaf_count,
                    ebins=est.bin_count, rng=b.pf.getRngState(), conv=st.converged, miss=st.cdf_miss,
                    counts=list(sf.counts), form=sf.form_used, windows=sf.windows_used, route=sf.tree_route,
                    slice=b.slice() if sf.form_used == "in_place" else None, rebalanced=sf.rebalanced,
                    w_slow=st.w_slow, w_fast=st.w_fast)

    return run_ranks(W, body)


def check_mn(pool, samples, cuts, max_samples, kld, rng_state, min_samples=100, what=None, window_too=True):
    """One in-place resample against the single engine's permuted set; returns (records, single state, counts)."""
    W = len(cuts) - 1
    pf1, S, st1, rng_after = single_resample(pool, samples, max_samples, kld, rng_state, resampler=0,
                                             min_samples=min_samples)
    M = st1.sample_count
    if window_too:  # the precondition: no knife-edge input
        win = mn_sharded(pool, samples, cuts, max_samples, kld, rng_state, min_samples, form="window")
        assert np.array_equal(np.concatenate([r["set"] for r in win]), S), what
        assert all(r["form"] == "window" and r["M"] == M and r["rng"] == rng_after for r in win), what
    recs = mn_sharded(pool, samples, cuts, max_samples, kld, rng_state, min_samples)
    want, counts = permuted(S, samples, cuts)
    got = np.concatenate([r["set"] for r in recs])
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, :3], want[:, :3]), what
    assert np.all(got[:, 3] == 1.0 / M), what
    firsts = [sum(counts[:q]) for q in range(W)]
    for k, r in enumerate(recs):
        assert r["form"] == "in_place" and r["windows"] == 0, (what, k)
        assert r["M"] == M and r["rng"] == rng_after and not r["miss"], (what, k)
        assert r["counts"] == counts and r["set"].shape[0] == counts[k], (what, k, r["counts"], counts)
        assert r["slice"] == (firsts[k], counts[k], mnr.IN_PLACE), (what, k)
        assert (r["leaf"], r["bins"]) == (r["eleaf"], r["ebins"]) == (st1.leaf_count, st1.bin_count), (what, k)
        assert r["conv"] == st1.converged, (what, k)
        assert (r["w_slow"], r["w_fast"]) == (st1.w_slow, st1.w_fast), (what, k)
    return recs, st1, counts


# ---------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("maxs,kind", [(3, "spread"), (255, "blob"), (256, "spread"), (257, "blob"), (2047, "blob"),
                                       (2048, "spread"), (2049, "blob")])
def test_sizes_around_the_compaction_tile(pool, maxs, kind):
    """max_samples one below, at and one above the select's tile of 256 and around 2 048 (eight tiles: the scan of the
    tile counts), and 3; W = 3 over an uneven cut."""
    n = maxs
    samples = cloud(n, kind, seed=maxs)
    cuts = [0, 1, (5 * n) // 12, n] if n > 3 else [0, 1, 2, 3]
    recs, st1, _ = check_mn(pool, samples, cuts, maxs, 0, 4242 + maxs, min_samples=2, what=(maxs, kind))
    if kind == "spread":
        assert st1.sample_count == maxs  # no stop


@pytest.mark.parametrize("split", ["even", "uneven", "empty"])
@pytest.mark.parametrize("W", [1, 3, 4])
def test_world_sizes_and_cuts_on_a_blob_that_stops(pool, W, split):
    n = 3000
    samples = cloud(n, "blob", seed=7)
    recs, st1, counts = check_mn(pool, samples, cuts_for(n, W, split), n, 0, 98765, what=(W, split))
    assert 1000 < st1.sample_count < n  # the stop rule fired
    assert recs[0]["route"] == "host"   # few bins: the host tree
    if split == "empty" and W > 1:
        assert 0 in counts


def test_spread_cloud_draws_every_candidate(pool):
    n = 3000
    recs, st1, _ = check_mn(pool, cloud(n, "spread", seed=9), cuts_for(n, 3, "uneven"), n, 0, 5551212)
    assert st1.sample_count == n


@pytest.mark.parametrize("kld", [0, 1])
def test_many_bins_take_the_device_route(pool, kld):
    """20 000 samples over 300 m x 300 m: n draws with replacement reach about 0.6 n distinct particles, so this is the
    smallest round size that leaves more than 8 192 distinct keys; the leaf count after every key then comes from the
    device tree (BPF_KLD_COUNT_BINS: the key count itself, no tree)."""
    n = 20000
    samples = cloud(n, "spread", seed=10, extent=150.0)
    recs, st1, _ = check_mn(pool, samples, cuts_for(n, 4, "even"), n, kld, 777)
    assert st1.bin_count >= 8192
    assert recs[0]["route"] == ("device" if kld == 0 else "bins")


@pytest.mark.parametrize("kind", ["tight", "blob"])
def test_bins_mode_on_a_blob(pool, kind):
    """BPF_KLD_COUNT_BINS counts distinct keys (more than leaves): the tight blob stops early, the wider one does not."""
    n = 3000
    recs, st1, _ = check_mn(pool, cloud(n, kind, seed=12), cuts_for(n, 3, "uneven"), n, 1, 31337)
    assert (st1.sample_count < n) == (kind == "tight") and recs[0]["route"] == "bins"


def test_a_rank_that_owns_every_draw_and_ranks_that_own_none(pool):
    """All weight on the particles of the middle rank: it keeps every candidate, the others none."""
    n, W = 1500, 3
    samples = cloud(n, "blob", seed=14)
    cuts = cuts_for(n, W, "even")
    w = np.zeros(n)
    w[cuts[1]:cuts[2]] = np.random.default_rng(15).random(cuts[2] - cuts[1]) + 1e-3
    samples[:, 3] = w / w.sum()
    recs, st1, counts = check_mn(pool, samples, cuts, n, 0, 2468, what="one owner")
    assert counts == [0, st1.sample_count, 0]


# ---------------------------------------------------------------------------------------------------- 2. cap, rebalance
def lopsided(n, W, seed):
    samples = cloud(n, "blob", seed=seed)
    cuts = cuts_for(n, W, "even")
    w = np.random.default_rng(seed + 1).random(n) + 1e-3
    w[cuts[2]:cuts[3]] *= 27.0
    samples[:, 3] = w / w.sum()
    return samples, cuts


def test_the_cap_takes_the_window_form(pool):
    n, W = 2000, 4
    samples, cuts = lopsided(n, W, 16)
    capped = mn_sharded(pool, samples, cuts, n, 0, 1357, max_share=1.0)
    window = mn_sharded(pool, samples, cuts, n, 0, 1357, form="window")
    M = window[0]["M"]
    for k in range(W):
        assert capped[k]["form"] == "window" and capped[k]["windows"] >= 1
        assert capped[k]["counts"] == window[k]["counts"] == [(M * (r + 1)) // W - (M * r) // W for r in range(W)]
        assert np.array_equal(capped[k]["set"], window[k]["set"])
        for key in ("M", "leaf", "bins", "rng", "conv", "miss"):
            assert capped[k][key] == window[k][key], key
    recs, st1, counts = check_mn(pool, samples, cuts, n, 0, 1357, what="max_share = W", window_too=False)
    assert max(counts) > 1.0 * ((M + W - 1) // W)


def test_auto_rebalance_behind_it_keeps_the_concatenation(pool):
    n, W = 2000, 4
    samples, cuts = lopsided(n, W, 18)
    plain = mn_sharded(pool, samples, cuts, n, 0, 97531)
    auto = mn_sharded(pool, samples, cuts, n, 0, 97531, max_share=1.0, rebalance="auto")
    M = plain[0]["M"]
    assert np.array_equal(np.concatenate([r["set"] for r in auto]), np.concatenate([r["set"] for r in plain]))
    for k in range(W):
        assert auto[k]["form"] == "in_place" and auto[k]["rebalanced"] > 0
        assert auto[k]["counts"] == [(M * (r + 1)) // W - (M * r) // W for r in range(W)]
        for key in ("M", "leaf", "bins", "rng", "conv"):
            assert auto[k][key] == plain[k][key], key


# ---------------------------------------------------------------------------------------------------- 3. miss
def test_a_miss_beyond_the_stop_does_not_flag_the_resample(pool):
    """Weights that sum to 0.999 (set by hand: the slices are the CDF sums themselves) and an empty LAST shard: a
    uniform in [0.999, 1) is the reference's failed search, and the empty shard has no particle to give it.  The seed
    is chosen so that the first such uniform comes after the stop: a draw the reference never made."""
    n, W = 3000, 3
    samples = cloud(n, "blob", seed=20)
    samples[:, 3] *= 0.999
    cuts = [0, n // 2, n, n]
    top = 0.0
    for w in samples[:, 3]:
        top += float(w)
    for seed in range(1, 200):
        rng0 = pcr.skip(seed * 7919, 3)
        u = [pcr.skip(rng0, 2 * m + 2) / 2.0 ** 48 for m in range(n)]
        late = [m for m in range(n) if u[m] >= top - 1e-9]
        if late and late[0] > 2500:
            break
    assert late and late[0] > 2500 and u[late[0]] >= top + 1e-9  # (clear of the edge by more than the sums' rounding)
    recs, st1, counts = check_mn(pool, samples, cuts, n, 0, rng0, what="late miss", window_too=False)
    assert st1.sample_count <= 2500 and counts[2] == 0
    assert not any(r["miss"] for r in recs)


# ---------------------------------------------------------------------------------------------------- 4. the stage calls
def test_setter_and_stage_calls_refuse_what_they_cannot_do(pool):
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend
    n = 600
    e = bpf.Engine(0)  # a fresh engine: the default is part of what is checked
    request_close = e.close
    pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
    pf.setResampleModel(0)
    pf.initWithSamples(cloud(n, "blob", seed=19))
    b = HipShardBackend(e, None, pf, torch.device("cuda", 0))
    for bad in (2, -1):
        with pytest.raises(bpf.BpfError) as ei:
            b.set_multinomial_form(bad)
        assert ei.value.code == 1
    assert b.multinomial_form() == 0  # the default: window
    b.set_multinomial_form(1)
    assert b.multinomial_form() == 1 and b.resample_form()[0] == 0  # a setting of its own
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    sums = torch.ones(1, dtype=torch.float64, device="cuda")
    rng = pf.getRngState()
    b.begin_resample(rng, 50)
    b.build_cdf(flags)
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_mn_bins()  # no select
    assert ei.value.code == 2
    dummy = torch.zeros((1, 2, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_mn_stop(dummy, [1], 4)  # no bins
    assert ei.value.code == 2
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_mn_select(rng + 1, sums, False, 0, 1, flags)  # not the resample begun
    assert ei.value.code == 1
    pf.setResampleModel(1)
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_mn_select(rng, sums, False, 0, 1, flags)  # the systematic resampler has its own select
    assert ei.value.code == 1
    pf.setResampleModel(0)
    assert b.inplace_mn_select(rng, sums, False, 0, 1, flags) == n  # W = 1: every candidate is this rank's
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_mn_stop(dummy, [1], 4)  # select, but no bins yet
    assert ei.value.code == 2
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_xy_sums()  # nothing committed yet
    assert ei.value.code == 2
    assert pf.getState().sample_count == n  # nothing of the filter has changed
    request_close()


# ---------------------------------------------------------------------------------------------------- 5. one-call form
class LocalWorld:
    """W engines on device 0 with the map, the scanner and the GLOBAL bounds, connected as one local world."""

    def __init__(self, sc, slices, n, form, alpha=(0.0, 0.0), kld=0, seed=21, max_share=None, pose_check=None):
        import badger_amcl_amd as bpf
        import badger_amcl_amd.pf as hpf
        from badger_amcl_amd.local_world import LocalShardedFilter
        W = len(slices)
        self.engines = [bpf.Engine(0) for _ in range(W)]
        self.keep, pfs = [], []
        for e in self.engines:
            m, scn, pf, data = sc.gpu_objects(e, 60, "lf", min_samples=100, max_samples=n, seed=seed, alpha=alpha)
            pf.setResampleModel(0)
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            pf.setUniformPoseCheck(*(pose_check or (0.0, 0.5)))
            bpf.Odom(e).setModel(*ODOM)
            self.keep.append((m, scn, data))
            pfs.append(pf)
        self.data = self.keep[0][2]
        self.f = LocalShardedFilter(pfs, kld_count=kld, multinomial_form=form,
                                    max_share=float(W) if max_share is None else max_share)
        self.f.load(slices, tree=False)

    def close(self):
        self.f.close()
        for e in self.engines:
            e.close()


def single_engine(sc, n, alpha=(0.0, 0.0), kld=0, seed=21, pose_check=None):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    e = bpf.Engine(0)
    m, scn, pf, data = sc.gpu_objects(e, 60, "lf", min_samples=100, max_samples=n, seed=seed, alpha=alpha)
    pf.setResampleModel(0)
    pf.setKldCount(kld)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    pf.setUniformPoseCheck(*(pose_check or (0.0, 0.5)))
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    return e, (m, scn, data), pf, od


def split(s, counts):
    at, out = 0, []
    for c in counts:
        out.append(np.ascontiguousarray(s[at:at + c]))
        at += c
    return out


def test_two_cycles_through_the_one_call_form(orc):
    """Motion update, sensor update and resample, twice, through LocalShardedFilter (bpf_shard_update_resample over the
    local exchange, the slices from the sensor update's totals) beside a single engine that is loaded with the
    permuted set after every resample.  A second world in the window form, loaded with the in-place world's slices
    before every cycle, is the precondition: it must equal the single engine bit for bit."""
    import badger_amcl_amd as bpf
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged")
    n, W = 3000, 3
    counts0 = [1, (5 * n) // 12 - 1, n - (5 * n) // 12]
    e1, keep1, pf1, od1 = single_engine(sc, n)
    pf1.initWithSamples(sc.samples)
    ip = LocalWorld(sc, split(sc.samples, counts0), n, "in_place")
    win = LocalWorld(sc, split(sc.samples, counts0), n, "window")
    try:
        for cycle in range(2):
            cur = np.concatenate(ip.f.local_sets())
            assert np.array_equal(cur, read_set(pf1)[0])
            cuts = [0] + list(np.cumsum(ip.f.counts))
            win.f.load(split(cur, ip.f.counts), tree=False)
            for p in win.f.pfs:
                p.setRngState(pf1.getRngState())
            win.f.leaf_count = ip.f.leaf_count
            od1.updateAction(pf1, bpf.OdomData(*ODATA))
            keep1[1].updateSensor(pf1, keep1[2])
            scored = read_set(pf1)[0]
            assert len(set(map(tuple, scored[:, :3]))) == scored.shape[0]  # a pose names its source
            pf1.updateResample()
            S, st1 = read_set(pf1)
            M = st1.sample_count
            for w in (win, ip):
                w.f.update_action(None, bpf.OdomData(*ODATA))
                w.f.update_sensor(w.data)
            before = ip.f.exchange_counts()
            win.f.update_resample()
            ip.f.update_resample()
            assert np.array_equal(np.concatenate(win.f.local_sets()), S), cycle  # the precondition
            assert win.f.form_used == "window" and win.f.windows_used >= 1
            assert [a - b for a, b in zip(ip.f.exchange_counts(), before)] == [EXCHANGES] * W
            want, counts = permuted(S, scored, cuts)
            got = np.concatenate(ip.f.local_sets())
            assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3]), cycle
            assert np.all(got[:, 3] == 1.0 / M)
            assert ip.f.form_used == "in_place" and ip.f.windows_used == 0 and not ip.f.cdf_miss
            assert ip.f.counts == counts and ip.f.sample_count == M
            assert (ip.f.leaf_count, ip.f.bin_count) == (st1.leaf_count, st1.bin_count)
            assert ip.f.rng_states() == [pf1.getRngState()] * W
            assert [s.converged for s in ip.f.rank_states()] == [st1.converged] * W
            assert [ip.f.slice(r) for r in range(W)] == [(sum(counts[:r]), counts[r], 1) for r in range(W)]
            rng_after = pf1.getRngState()
            pf1.initWithSamples(np.ascontiguousarray(want), -1)  # the permuted set: what the ranks hold
            pf1.setRngState(rng_after)
    finally:
        ip.close()
        win.close()
        e1.close()


@pytest.mark.parametrize("pose_check,K", [((0.0, 0.5), 0), ((10.0, 0.5), 4)])
def test_recovery_through_the_one_call_form(orc, pose_check, K):
    """w_diff > 0 (two sensor updates, the second against a scan that fits nowhere, fast decay rates): the draws follow
    the resolved chain, the random free-space poses (K rejected trials each) are rank 0's, in draw order, and the
    stream ends where the single engine's does; w_slow and w_fast are reset."""
    import badger_amcl_amd as bpf
    assert pcr.retries(*pose_check) == K
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged")
    n, W, alpha = 3000, 3, (0.5, 0.9)
    counts0 = [n // 4, n // 4, n - 2 * (n // 4)]
    cuts = [0] + list(np.cumsum(counts0))
    bad = bpf.PlanarData(np.full(sc.ranges.shape[0], 1.0), sc.angles, sc.range_max)
    e1, keep1, pf1, od1 = single_engine(sc, n, alpha=alpha, pose_check=pose_check)
    pf1.initWithSamples(sc.samples)
    keep1[1].updateSensor(pf1, keep1[2])
    keep1[1].updateSensor(pf1, bad)
    scored = read_set(pf1)[0]
    pf1.updateResample()
    S, st1 = read_set(pf1)
    M = st1.sample_count
    assert st1.w_diff > 0.05
    worlds = {form: LocalWorld(sc, split(sc.samples, counts0), n, form, alpha=alpha, pose_check=pose_check)
              for form in ("window", "in_place")}
    try:
        for w in worlds.values():
            w.f.update_sensor(w.data)
            w.f.update_sensor(bad)
            w.f.update_resample()
        assert np.array_equal(np.concatenate(worlds["window"].f.local_sets()), S)  # the precondition
        f = worlds["in_place"].f
        want, counts = permuted(S, scored, cuts)
        n_random = sum(1 for p in S[:, :3] if tuple(p) not in set(map(tuple, scored[:, :3])))
        assert n_random > 10
        got = np.concatenate(f.local_sets())
        assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
        assert f.form_used == "in_place" and f.counts == counts and f.sample_count == M and not f.cdf_miss
        assert (f.leaf_count, f.bin_count) == (st1.leaf_count, st1.bin_count)
        assert f.rng_states() == [pf1.getRngState()] * W
        for s in f.rank_states():
            assert (s.w_slow, s.w_fast) == (0.0, 0.0) == (st1.w_slow, st1.w_fast) and s.converged == st1.converged
    finally:
        for w in worlds.values():
            w.close()
        e1.close()
