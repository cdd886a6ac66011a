"""The systematic resample of a sharded set in place (include/badger_pf.h, bpf_shard_set_resample_form): every rank
resamples its own slice into its own slice, and the concatenation of the slices is the set ONE engine produces, with
the wrapped teeth moved to the front (shard_in_place_ref.rotate).  W engines in one process; ShardedFilter drives the
stage functions of every rank on a thread of its own, over a thread-based stand-in for torch.distributed that plays
the transport with torch ops on the device.  The reference is one engine holding the whole set: update_resample,
get_samples, then the rotation by the model's i_wrap."""
import os
import sys
import threading

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shard_in_place_ref as ipr  # noqa: E402
from scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu

ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion
LCG_A, LCG_C = 0x5DEECE66D, 0xB
BIG_LEAF = 1 << 20  # a leaf count whose resample limit is beyond any max_samples here: M = max_samples


# ---------------------------------------------------------------------------------------------------- harness
class ThreadDist:
    """torch.distributed for W ShardedFilters in W threads of this process (device tensors, one stream)."""

    class ReduceOp:
        SUM, MIN = "sum", "min"

    def __init__(self, world):
        self.world = world
        self.slots = [None] * world
        self.bar = threading.Barrier(world, timeout=120)

    class View:
        def __init__(self, group, rank):
            self.g, self.rank = group, rank
            self.ReduceOp = ThreadDist.ReduceOp

        def get_rank(self):
            return self.rank

        def get_world_size(self):
            return self.g.world

        def get_backend(self):
            return "threads"

        def all_gather(self, outs, src):
            g = self.g
            g.slots[self.rank] = src
            g.bar.wait()
            for r in range(g.world):
                outs[r].copy_(g.slots[r])
            g.bar.wait()

        def all_reduce(self, t, op):
            g = self.g
            g.slots[self.rank] = t.clone()
            g.bar.wait()
            stacked = torch.stack(g.slots)
            res = stacked.sum(dim=0) if op == "sum" else stacked.min(dim=0).values
            g.bar.wait()
            t.copy_(res)


def run_ranks(W, body):
    """body(rank, dist_view) in W threads; the first exception is raised here."""
    group = ThreadDist(W)
    out, errs = [None] * W, []

    def run(r):
        try:
            out[r] = body(r, ThreadDist.View(group, r))
        except BaseException as err:  # noqa: BLE001 -- reported below; the others are released from their barrier
            errs.append(err)
            group.bar.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    real = [e for e in errs if not isinstance(e, threading.BrokenBarrierError)]
    if real or errs:
        raise (real or errs)[0]
    return out


class Pool:
    """[0]: the single engine; [1 .. 8]: the ranks.  The map and the scanner are attached to an engine when a test
    first asks for them."""

    def __init__(self, orc):
        import badger_amcl_amd as bpf
        torch.cuda.set_device(0)  # torch's context first; the engines run on its stream
        torch.zeros(1, device="cuda")
        self.orc = orc
        self.engines = [bpf.Engine(0) for _ in range(9)]
        self.keep = [None] * 9
        self.sc = None

    def scenario(self):
        if self.sc is None:
            self.sc = Scenario(self.orc, size=400, n=256, beams=181)
        return self.sc

    def filter(self, k, max_samples, min_samples=100, alpha=(0.0, 0.0), with_map=False):
        import badger_amcl_amd as bpf
        e = self.engines[k]
        if with_map and self.keep[k] is None:
            m, scn, _, data = self.scenario().gpu_objects(e, 181, "lf")
            self.keep[k] = (m, scn, data)
        return bpf.ParticleFilter(e, min_samples, max_samples, alpha[0], alpha[1], 85.0)

    def scanner(self, k):
        return (self.keep[k][1], self.keep[k][2]) if self.keep[k] else (None, None)

    def close(self):
        self.keep = []
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def pool(orc):
    p = Pool(orc)
    yield p
    p.close()


def read_set(pf):
    st = pf.getState()
    s = pf.getCurrentSet().samples if st.sample_count > 0 else np.zeros((0, 4))
    return s, st


def load_slice(pf, s, total):
    if s.shape[0] > 0:
        pf.initWithSamples(np.ascontiguousarray(s))
    else:
        # a shard without samples (bpf_pf_set_samples takes none): adopt an empty slice of the global set
        pf.e.check(pf.e.lib.bpf_shard_adopt_dev(pf.e.h, None, None, None, 0, int(total), 0, 0))


def cuts_for(n, W, kind):
    if kind == "even" or W == 1:
        return [(n * r) // W for r in range(W + 1)]
    if kind == "uneven":
        full = [0, 1, 2, 3, (5 * n) // 12, (5 * n) // 12 + 1, (3 * n) // 4, n - 1, n]
        return {2: [0, 1, n], 3: [0, 1, (5 * n) // 12, n], 8: full}[W]
    if kind == "empty":  # two shards without samples (W = 2: the one there can be)
        return {2: [0, 0, n], 3: [0, 0, n, n], 8: [0, 0, 2, n // 4, n // 4, n // 2, n // 2 + 1, n - 1, n]}[W]
    raise ValueError(kind)


def cloud(n, kind, seed):
    """blob: clearly converged (sigma 0.05 m against dist_threshold 0.5 m); spread: clearly not (16 m x 16 m)."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    if kind == "blob":
        s[:, 0], s[:, 1], s[:, 2] = rng.normal(3.0, 0.05, n), rng.normal(-2.0, 0.05, n), rng.normal(0.3, 0.02, n)
    else:
        s[:, 0], s[:, 1], s[:, 2] = rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-np.pi, np.pi, n)
    w = rng.random(n) ** 2 + 1e-3
    s[:, 3] = w / w.sum()
    return s


def state_for_u0(u):
    """The drand48 state whose next element is floor(u 2^48): the systematic start lands at u."""
    x = int(u * 2.0 ** 48)
    return ((x - LCG_C) * pow(LCG_A, -1, 1 << 48)) & ipr.MASK48


def single_resample(pool, samples, max_samples, kld, rng_state, resampler=1, leaf=-1, min_samples=100):
    """One engine holding the whole set: (new set, state, rng after, rng before)."""
    pf1 = pool.filter(0, max_samples, min_samples)
    pf1.setResampleModel(resampler)
    pf1.setKldCount(kld)
    pf1.setRngState(rng_state)
    pf1.initWithSamples(samples, leaf)
    pf1.updateResample()
    s, st = read_set(pf1)
    return pf1, s, st, pf1.getRngState()


def tree_of(pool, samples, max_samples, kld, min_samples=100):
    """(leaf, bin) counts one engine reports for `samples` (set_samples(..., -1))."""
    pf1 = pool.filter(0, max_samples, min_samples)
    pf1.setKldCount(kld)
    pf1.initWithSamples(np.ascontiguousarray(samples), -1)
    st = pf1.getState()
    return st.leaf_count, st.bin_count


def sharded_resample(pool, samples, cuts, max_samples, kld, rng_state, resampler=1, leaf=None, min_samples=100,
                     form="in_place", max_share=None):
    """ShardedFilter on W engines, one resample from slices loaded by hand; per rank a dict of what it ended with."""
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    W = len(cuts) - 1
    if leaf is None:  # of the whole set's tree, as the reference builds it when the set is created
        leaf = tree_of(pool, samples, max_samples, kld, min_samples)[0]
    bs = []
    for r in range(W):
        pf = pool.filter(1 + r, max_samples, min_samples)
        pf.setResampleModel(resampler)
        pf.setKldCount(kld)
        pf.setRngState(rng_state)
        load_slice(pf, samples[cuts[r]:cuts[r + 1]], samples.shape[0])
        bs.append(HipShardBackend(pool.engines[1 + r], None, pf, torch.device("cuda", 0)))

    def body(rank, dist):
        b = bs[rank]
        sf = ShardedFilter(b, dist, rank=rank, world=W, exchange="collective", init_follows=True,
                           resample_form=form, max_share=float(W) if max_share is None else max_share)
        sf.leaf_count = leaf
        sf.update_resample()
        st = sf.state()
        s, est = read_set(b.pf)
        return dict(set=s, M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count, eleaf=est.leaf_count,
                    ebins=est.bin_count, rng=b.pf.getRngState(), conv=st.converged, miss=st.cdf_miss,
                    counts=list(sf.counts), form=sf.form_used, windows=sf.windows_used,
                    slice=b.slice() if sf.form_used == "in_place" else None, pct=est.percent_converged)

    return run_ranks(W, body)


def check_rotation(pool, samples, cuts, max_samples, kld, rng_state, leaf=None, min_samples=100, what=None):
    """The whole comparison of one in-place resample with the rotated single-engine set; returns the model's plan."""
    W = len(cuts) - 1
    n = samples.shape[0]
    recs = sharded_resample(pool, samples, cuts, max_samples, kld, rng_state, leaf=leaf, min_samples=min_samples)
    pf1, S, st1, rng_after = single_resample(pool, samples, max_samples, kld, rng_state,
                                             leaf=-1 if leaf is None else leaf, min_samples=min_samples)
    M = st1.sample_count
    # the model's plan from the CDF sums the ranks gather (weights set by hand: no totals of a sensor update)
    sums = []
    for q in range(W):
        acc = 0.0
        for w in samples[cuts[q]:cuts[q + 1], 3]:
            acc += float(w)  # the engine's scan adds in another order; a tooth within rounding of an edge would show
        sums.append(acc)
    P = ipr.plan(rng_state, M, 0, sums, False, max_share=float(W))
    want = ipr.rotate(S, 0, P["i_wrap"])
    got = np.concatenate([r["set"] for r in recs])
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, :3], want[:, :3]), what
    assert np.all(got[:, 3] == 1.0 / M), what
    leaf1, bins1 = tree_of(pool, want, max_samples, kld, min_samples)
    for k, r in enumerate(recs):
        assert r["form"] == "in_place" and r["windows"] == 0, (what, k)
        assert r["M"] == M and r["rng"] == rng_after and not r["miss"], (what, k)
        assert r["counts"] == P["counts"], (what, k, r["counts"], P["counts"])
        assert r["set"].shape[0] == P["counts"][k], (what, k)
        assert r["slice"] == (P["firsts"][k], P["counts"][k], ipr.IN_PLACE), (what, k)
        assert (r["leaf"], r["bins"]) == (r["eleaf"], r["ebins"]) == (leaf1, bins1), (what, k)
        assert r["conv"] == st1.converged, (what, k, r["pct"], st1.percent_converged)
    return P, recs, st1


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("kind", ["blob", "spread"])
@pytest.mark.parametrize("kld", [0, 1])
@pytest.mark.parametrize("split", ["even", "uneven", "empty"])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_slices_concatenate_to_the_rotated_single_engine_set(pool, W, split, kld, kind):
    n = 1200
    samples = cloud(n, kind, seed=7)
    P, recs, st1 = check_rotation(pool, samples, cuts_for(n, W, split), n, kld, state_for_u0(0.37),
                                  what=(W, split, kld, kind))
    assert st1.converged == (1 if kind == "blob" else 0)
    assert (st1.percent_converged == 100.0) if kind == "blob" else (st1.percent_converged < 10.0)


# ---------------------------------------------------------------------------------------------------- 2. shapes
def weights_for(n, cuts, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        w = rng.random(n) + 1e-3
    elif kind == "one":  # all weight on one particle of the middle rank: every other shard empties
        w = np.zeros(n)
        w[(cuts[1] + cuts[2]) // 2] = 1.0
    else:  # zero weights at the slice borders
        w = rng.random(n) + 1e-3
        for c in cuts[1:-1]:
            w[max(c - 1, 0)] = 0.0
            w[min(c, n - 1)] = 0.0
        if w.sum() == 0.0:
            w[n // 2] = 1.0
    return w / w.sum()


@pytest.mark.parametrize("wkind", ["random", "one", "borders"])
@pytest.mark.parametrize("u0", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("M", [3, 255, 257, 4097])
def test_smallest_shapes(pool, M, u0, wkind):
    """max_samples = M and a leaf count beyond every limit: the new set has M samples.  W = 3 over an even split, so
    u0 = 0.1 / 0.5 / 0.9 starts the comb in rank 0 / the middle rank / the last rank of a uniform CDF."""
    W, n = 3, M
    cuts = [(n * r) // W for r in range(W + 1)]
    samples = cloud(n, "spread", seed=M)
    samples[:, 3] = weights_for(n, cuts, wkind, seed=M + 1)
    P, recs, st1 = check_rotation(pool, samples, cuts, M, 0, state_for_u0(u0), leaf=BIG_LEAF, min_samples=2,
                                  what=(M, u0, wkind))
    assert st1.sample_count == M and sum(P["counts"]) == M
    assert P["targets"][0] == int(u0 * 2.0 ** 48) / 2.0 ** 48
    seam = M - P["i_wrap"]  # where tooth 0 sits in the rotated set
    if wkind == "one":
        assert P["counts"] == [0, M, 0]
    if wkind in ("random", "borders") and M >= 255:  # (M = 3: one tooth per rank, no interior; "one": rank 1 owns all)
        owner = ipr.owner(P["targets"][0], P["edges"])
        assert owner == {0.1: 0, 0.5: 1, 0.9: 2}[u0]
        assert P["firsts"][owner] < seam < P["firsts"][owner] + P["counts"][owner] - 1  # i_wrap inside a rank


# ---------------------------------------------------------------------------------------------------- 3. W
def test_the_result_does_not_depend_on_the_world_size(pool):
    n = 5000
    samples = cloud(n, "spread", seed=11)
    rng = state_for_u0(0.63)
    one = sharded_resample(pool, samples, cuts_for(n, 1, "even"), n, 0, rng)
    eight = sharded_resample(pool, samples, cuts_for(n, 8, "even"), n, 0, rng)
    a, b = one[0]["set"], np.concatenate([r["set"] for r in eight])
    assert a.shape == b.shape and np.array_equal(a, b)
    assert all(r["form"] == "in_place" for r in one + eight)
    assert eight[0]["M"] == one[0]["M"] and eight[3]["rng"] == one[0]["rng"]
    assert (eight[5]["leaf"], eight[5]["bins"]) == (one[0]["leaf"], one[0]["bins"])


# ---------------------------------------------------------------------------------------------------- 5. cap
def test_imbalance_cap_takes_the_window_form(pool):
    """90 % of the weight in rank 2 of 4: its share of the teeth is beyond 2 ceil(M / 4), so every rank takes the window
    form -- today's result, split evenly; with max_share = W the same set stays in place."""
    n, W = 2000, 4
    samples = cloud(n, "spread", seed=13)
    cuts = cuts_for(n, W, "even")
    w = np.random.default_rng(14).random(n) + 1e-3
    w[cuts[2]:cuts[3]] *= 27.0
    samples[:, 3] = w / w.sum()
    rng = state_for_u0(0.21)
    capped = sharded_resample(pool, samples, cuts, n, 0, rng, max_share=2.0)
    window = sharded_resample(pool, samples, cuts, n, 0, rng, form="window")
    M = window[0]["M"]
    for k in range(W):
        assert capped[k]["form"] == "window" and capped[k]["windows"] == 1
        assert capped[k]["counts"] == window[k]["counts"] == [(M * (r + 1)) // W - (M * r) // W for r in range(W)]
        assert np.array_equal(capped[k]["set"], window[k]["set"])
        for key in ("M", "leaf", "bins", "rng", "conv", "miss"):
            assert capped[k][key] == window[k][key], key
    P, recs, _ = check_rotation(pool, samples, cuts, n, 0, rng, what="max_share = W")
    assert max(P["counts"]) > 2.0 * ((M + W - 1) // W)
    assert ipr.plan(rng, M, 0, [float(sum(samples[cuts[q]:cuts[q + 1], 3])) for q in range(W)], False)["form"] == ipr.WINDOW


# ---------------------------------------------------------------------------------------------------- 7. multinomial
def test_multinomial_ignores_the_form(pool):
    n, W = 3000, 3
    samples = cloud(n, "blob", seed=17)
    cuts = cuts_for(n, W, "uneven")
    a = sharded_resample(pool, samples, cuts, n, 0, 12345, resampler=0, form="in_place")
    b = sharded_resample(pool, samples, cuts, n, 0, 12345, resampler=0, form="window")
    for k in range(W):
        assert a[k]["form"] == b[k]["form"] == "window" and a[k]["windows"] == b[k]["windows"] >= 1
        assert np.array_equal(a[k]["set"], b[k]["set"])
        for key in ("M", "leaf", "bins", "rng", "conv", "miss", "counts"):
            assert a[k][key] == b[k][key], key


# ---------------------------------------------------------------------------------------------------- 4. + 6. cycles
def cycle_ranks(pool, samples, cuts, alpha, steps, kld=0, seed=21):
    """ShardedFilter (in place, max_share = W) on W engines with the map: steps(sf, b, od, data, rec) per rank."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    W, n = len(cuts) - 1, samples.shape[0]
    bs = []
    for r in range(W):
        pf = pool.filter(1 + r, n, alpha=alpha, with_map=True)
        pf.setResampleModel(1)
        pf.setKldCount(kld)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.setUniformPoseCheck(0.0, 0.5)
        pf.srand48(seed)
        load_slice(pf, samples[cuts[r]:cuts[r + 1]], n)
        bs.append(HipShardBackend(pool.engines[1 + r], pool.scanner(1 + r)[0], pf, torch.device("cuda", 0)))

    def body(rank, dist):
        b = bs[rank]
        sf = ShardedFilter(b, dist, rank=rank, world=W, exchange="collective", resample_form="in_place",
                           max_share=float(W))
        od = bpf.Odom(b.e)
        od.setModel(*ODOM)
        rec = {}
        steps(sf, b, od, pool.scanner(1 + rank)[1], rec)
        return rec

    return run_ranks(W, body)


def single_with_map(pool, samples, alpha, kld=0, seed=21):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    pf1 = pool.filter(0, samples.shape[0], alpha=alpha, with_map=True)
    pf1.setResampleModel(1)
    pf1.setKldCount(kld)
    pf1.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    pf1.setUniformPoseCheck(0.0, 0.5)
    pf1.srand48(seed)
    pf1.initWithSamples(samples)
    od = bpf.Odom(pool.engines[0])
    od.setModel(*ODOM)
    scn, data = pool.scanner(0)
    return pf1, od, scn, data


def test_recovery_random_poses_sit_at_rank_0s_head(pool, orc):
    """w_diff > 0 (two sensor updates, the second against a scan that fits nowhere, with fast decay rates): the
    random free-space poses are the single engine's, at rank 0's head, and the stream ends where the single engine's
    does."""
    import badger_amcl_amd as bpf
    sc = pool.scenario()
    n, W, alpha = 3000, 3, (0.5, 0.9)
    from badger_amcl_amd import synth
    samples = synth.converged_cloud(n, sc.pose, seed=31)
    cuts = cuts_for(n, W, "uneven")
    bad = bpf.PlanarData(np.full(sc.ranges.shape[0], 1.0), sc.angles, sc.range_max)

    def steps(sf, b, od, data, rec):
        sf.update_sensor(data)
        sf.update_sensor(bad)
        rec["rng0"] = b.pf.getRngState()
        sf.update_resample()
        st = sf.state()
        rec.update(set=read_set(b.pf)[0], M=st.sample_count, rng=b.pf.getRngState(), counts=list(sf.counts),
                   form=sf.form_used, miss=st.cdf_miss, w_slow=st.w_slow, w_fast=st.w_fast)

    recs = cycle_ranks(pool, samples, cuts, alpha, steps)
    pf1, od, scn, data = single_with_map(pool, samples, alpha)
    scn.updateSensor(pf1, data)
    scn.updateSensor(pf1, bad)
    rng0 = pf1.getRngState()
    pf1.updateResample()
    S, st1 = read_set(pf1)
    M = st1.sample_count
    n_random = int(st1.w_diff * M)
    assert st1.w_diff > 0.05 and n_random > 10
    _, i_wrap, _ = ipr.target_chain(rng0, M - n_random)
    want = ipr.rotate(S, n_random, i_wrap)
    got = np.concatenate([r["set"] for r in recs])
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    assert np.array_equal(recs[0]["set"][:n_random, :3], S[:n_random, :3]) and recs[0]["counts"][0] >= n_random
    for r in recs:
        assert r["form"] == "in_place" and r["rng0"] == rng0 and r["rng"] == pf1.getRngState() and r["M"] == M
        assert (r["w_slow"], r["w_fast"]) == (0.0, 0.0) == (st1.w_slow, st1.w_fast) and not r["miss"]


def test_two_cycles_on_the_uneven_slices(pool, orc):
    """Two rounds of motion, sensor update and in-place resample; the single engine's set is rotated between the
    rounds (get_samples, set_samples(..., -1)), which is what the ranks' slices hold.  Poses and counts exact, the
    normalised weights to 1e-9 relative.  Precondition, from the single engine's CDF: no target within 1e-9 of a CDF
    edge (the ranks' CDFs are the same sums in another order); seed 21 meets it."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    sc = pool.scenario()
    n, W = 3000, 3
    samples = synth.converged_cloud(n, sc.pose, seed=33)
    cuts = cuts_for(n, W, "uneven")

    def steps(sf, b, od, data, rec):
        rec["rounds"] = []
        for _ in range(2):
            sf.update_action(od, bpf.OdomData(*ODATA))
            moved = read_set(b.pf)[0]
            sf.update_sensor(data)
            scored = read_set(b.pf)[0]
            sf.update_resample()
            st = sf.state()
            best = sf.get_max_weight_pose()
            rec["rounds"].append(dict(moved=moved, scored=scored, set=read_set(b.pf)[0], M=st.sample_count,
                                      leaf=st.leaf_count, bins=st.bin_count, rng=b.pf.getRngState(),
                                      counts=list(sf.counts), form=sf.form_used, conv=st.converged, miss=st.cdf_miss,
                                      best=best))

    recs = cycle_ranks(pool, samples, cuts, (0.0, 0.0), steps)
    pf1, od, scn, data = single_with_map(pool, samples, (0.0, 0.0))
    for k in range(2):
        rr = [r["rounds"][k] for r in recs]
        od.updateAction(pf1, bpf.OdomData(*ODATA))
        assert np.array_equal(np.concatenate([r["moved"] for r in rr]), read_set(pf1)[0]), k
        scn.updateSensor(pf1, data)
        w1 = read_set(pf1)[0]
        w = np.concatenate([r["scored"] for r in rr])
        assert np.array_equal(w[:, :3], w1[:, :3])
        assert np.max(np.abs(w[:, 3] - w1[:, 3]) / w1[:, 3]) <= 1e-9
        rng0 = pf1.getRngState()
        pf1.updateResample()
        S, st1 = read_set(pf1)
        M = st1.sample_count
        targets, i_wrap, _ = ipr.target_chain(rng0, M)
        cdf = np.concatenate([[0.0], np.cumsum(w1[:, 3])])
        gap = np.min(np.abs(np.asarray(targets)[:, None] - cdf[None, :])) if M * cdf.size < 5e7 else None
        assert gap is not None and gap > 1e-9, gap  # the precondition
        want = ipr.rotate(S, 0, i_wrap)
        got = np.concatenate([r["set"] for r in rr])
        assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3]), k
        assert np.all(got[:, 3] == 1.0 / M)
        rng_after = pf1.getRngState()
        pf1.initWithSamples(want, -1)  # the rotated set: what the ranks hold
        pf1.setRngState(rng_after)
        st = pf1.getState()
        best1 = pf1.getMaxWeightPose()
        for r in rr:
            assert r["form"] == "in_place" and r["M"] == M and r["rng"] == rng_after and not r["miss"]
            assert sum(r["counts"]) == M and r["counts"] == rr[0]["counts"]
            assert (r["leaf"], r["bins"]) == (st.leaf_count, st.bin_count) and r["conv"] == st1.converged
            assert r["best"][0] == best1[0] and np.array_equal(np.asarray(r["best"][1]), np.asarray(best1[1]))
        assert [r["set"].shape[0] for r in rr] == rr[0]["counts"]


# ---------------------------------------------------------------------------------------------------- the stage calls
def test_stage_calls_refuse_what_they_cannot_do(pool):
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend
    n = 600
    pf = pool.filter(1, n)
    pf.setResampleModel(1)
    pf.initWithSamples(cloud(n, "blob", seed=19))
    b = HipShardBackend(pool.engines[1], None, pf, torch.device("cuda", 0))
    with pytest.raises(bpf.BpfError):
        b.set_resample_form(2, 2.0)
    with pytest.raises(bpf.BpfError):
        b.set_resample_form(1, 0.5)
    b.set_resample_form(1, 3.0)
    assert b.resample_form() == (1, 3.0)
    with pytest.raises(bpf.BpfError) as ei:
        b.slice()  # a set loaded by hand: nobody has told the engine where it sits
    assert ei.value.code == 2
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_xy_sums()  # no select
    assert ei.value.code == 2
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    sums = torch.ones(1, dtype=torch.float64, device="cuda")
    rng = pf.getRngState()
    b.begin_resample(rng, 50)
    b.build_cdf(flags)
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_select(rng + 1, 100, sums, False, 0, 1, flags)  # not the resample begun
    assert ei.value.code == 1
    pf.setResampleModel(0)
    with pytest.raises(bpf.BpfError) as ei:
        b.inplace_select(rng, 100, sums, False, 0, 1, flags)  # the multinomial resampler keeps the window
    assert ei.value.code == 1
    assert pf.getState().sample_count == n
    b.set_resample_form(0, 2.0)
