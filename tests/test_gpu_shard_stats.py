"""Cluster statistics of a SHARDED set on the GPU box (include/badger_pf.h, bpf_shard_stats_*): the global clusters,
the set's mean / cov and the heaviest cluster's pose on every rank's engine must be the same BITS as one engine
holding the concatenation of the slices returns -- exact integer sums leave no knife edge, so nothing here is compared
with a tolerance except against the oracle's serial double chain (the budgets of test_gpu_next_rows.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

from scenario import Scenario
from badger_amcl_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu

MAX_N = 100000


# ---------------------------------------------------------------------------------------------------- helpers
def read_stats(pf):
    """Everything the ordinary getters return, as one dict of arrays (compared with np.array_equal)."""
    n, mean, cov = pf.computeClusterStats()
    cl = [pf.getClusterStats(k) for k in range(n)]
    assert pf.getClusterStats(n) is None
    bw, bp = pf.getMaxWeightPose()
    return dict(n=np.array([n]), set_mean=np.array(mean), set_cov=np.array(cov),
                weight=np.array([c[0] for c in cl]), mean=np.array([c[1] for c in cl]).reshape(n, 3),
                count=np.array([c[2] for c in cl]), cov=np.array([c[3] for c in cl]).reshape(n, 5),
                best_w=np.array([bw]), best_pose=np.array(bp))


def assert_same_bits(got, want, what=""):
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


class Recorded:
    """The getters of pf.ParticleFilter over a read_stats() dict (for _assert_stats_equal of test_gpu_next_rows)."""

    def __init__(self, st):
        self.st = st

    def computeClusterStats(self):
        return int(self.st["n"][0]), self.st["set_mean"], self.st["set_cov"]

    def getClusterStats(self, k):
        st = self.st
        if k >= int(st["n"][0]):
            return None
        return st["weight"][k], st["mean"][k], st["count"][k], st["cov"][k]

    def getMaxWeightPose(self):
        return self.st["best_w"][0], self.st["best_pose"]


def assert_no_tie(want):
    """The one leave-out _assert_stats_equal permits (two heaviest clusters equal to rounding) must not be in use."""
    ws = np.sort(want["weight"])[::-1]
    assert ws.size < 2 or ws[0] - ws[1] > 1e-12 * ws[0]


def reference_stats(engine, samples, host=False):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    pf = bpf.ParticleFilter(engine, 100, max(MAX_N, samples.shape[0]), 0.0, 0.0, 85.0)
    pf.initWithSamples(np.ascontiguousarray(samples))
    engine.set_option(hpf.OPT_STATS_HOST, 1 if host else 0)
    try:
        return read_stats(pf)
    finally:
        engine.set_option(hpf.OPT_STATS_HOST, 0)


@pytest.fixture(scope="module")
def engines():
    import torch
    import badger_amcl_amd as bpf
    torch.cuda.set_device(0)  # torch's context first, as in the sharded workers; the engines run on its stream
    torch.zeros(1, device="cuda")
    pool = [bpf.Engine(0) for _ in range(17)]  # [0]: the single engine; [1 ..]: the ranks
    yield pool
    for e in pool:
        e.close()


def make_ranks(engines, samples, cuts):
    """One backend per slice [cuts[r], cuts[r + 1]) on device 0; an empty slice is an engine that adopted 0 samples."""
    import torch
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend
    n = samples.shape[0]
    out = []
    for r in range(len(cuts) - 1):
        e = engines[1 + r]
        lo, hi = cuts[r], cuts[r + 1]
        pf = bpf.ParticleFilter(e, 100, MAX_N, 0.0, 0.0, 85.0)
        if hi > lo:
            pf.initWithSamples(np.ascontiguousarray(samples[lo:hi]))
        else:
            e.check(e.lib.bpf_shard_adopt_dev(e.h, None, None, None, 0, n, 0, 0))
        assert pf.getState().sample_count == hi - lo
        out.append(HipShardBackend(e, None, pf, torch.device("cuda", 0)))
    return out


def run_stages(bs, samples, cuts, force_distributed=False):
    """The sequence of ShardedFilter._ensure_stats with the two exchanges done by torch ops on the device
    (concatenate, integer sum); returns the route taken."""
    import torch
    W, n = len(bs), samples.shape[0]
    counts = [cuts[r + 1] - cuts[r] for r in range(W)]
    route = None
    if n <= 4096 and not force_distributed:
        soa = torch.cat([b.stats_local_soa() for b in bs], dim=1).contiguous()  # exchange: all-gather of the slices
        assert soa.shape == (4, n)
        handled = [b.stats_gathered(soa, n) for b in bs]
        assert len(set(handled)) == 1
        route = {1: "gathered", 0: None, -1: "host"}[handled[0]]
    if route is None:
        lists = [b.stats_local_bins(cuts[r]) for r, b in enumerate(bs)]
        nbs = [int(l[0].shape[1]) for l in lists]
        if any(l[1] for l in lists):
            route = "host"
        else:
            pad = max(max(nbs), 1)
            all_bins = torch.zeros((W, 2, pad), dtype=torch.int64, device=bs[0].device)  # exchange 1
            for r, l in enumerate(lists):
                all_bins[r, :, :nbs[r]] = l[0]
            cs = [b.stats_label(all_bins, nbs, pad) for b in bs]
            assert len(set(cs)) == 1
            sums = [b.stats_local_sums() for b in bs]
            reduced = torch.stack(sums).sum(dim=0)  # exchange 2: lane-wise int64 sum of the limb words
            assert reduced.dtype == torch.int64 and reduced.numel() == 40 * cs[0]
            done = [b.stats_finish(reduced) for b in bs]
            assert len(set(done)) == 1  # sums beyond the fixed-point format: every rank finds out alike
            route = "host" if done[0] is False else "distributed"
    if route == "host":
        for b in bs:
            b.stats_host(samples)
    return route, counts


def three_blobs(orc):
    sc_ = Scenario(orc, size=400, n=3000, beams=61, cloud="converged")
    blobs = [synth.converged_cloud(1000, sc_.pose + off, seed=5 + i, sigma=(0.15, 0.15, 0.05))
             for i, off in enumerate([(0, 0, 0), (4.0, -2.0, 1.0), (-3.0, 3.5, -2.0)])]
    s = np.ascontiguousarray(np.concatenate(blobs))
    s[:, 3] = np.random.default_rng(9).uniform(0.5, 1.5, s.shape[0])
    s[:, 3] /= s[:, 3].sum()
    return s


_SETS = {}


def scored_set(engines, orc, name):
    """three_blobs: test_cluster_stats_of_loaded_multimodal_set's set, non-uniform weights; spread100k: 100 000 spread
    particles with scored weights; converged2k: 2 000 converged with scored weights."""
    if name not in _SETS:
        if name == "three_blobs":
            _SETS[name] = three_blobs(orc)
        else:
            size, n, cloud = (2000, 100000, "spread") if name == "spread100k" else (400, 2000, "converged")
            sc_ = Scenario(orc, size=size, n=n, beams=181, cloud=cloud)
            m, sc, pf, data = sc_.gpu_objects(engines[0], 181, "lf", min_samples=100, seed=21)
            sc.updateSensor(pf, data)
            _SETS[name] = pf.getCurrentSet().samples.copy()
    return _SETS[name]


def splits(n, W, kind):
    if kind == "even":
        return [(n * r) // W for r in range(W + 1)]
    if kind == "ragged":
        inner = np.sort(np.random.default_rng(W).integers(1, n, W - 1)) if W > 1 else np.array([], dtype=int)
        return [0] + [int(v) for v in inner] + [n]
    if kind == "empty":
        # every other shard empty, the first and the last among them when W allows
        cuts, at = [0], 0
        full = [r for r in range(W) if r % 2 == 1] or [0]
        for r in range(W):
            if r in full:
                at += n // len(full) if r != full[-1] else n - at
            cuts.append(at)
        cuts[-1] = n
        return cuts
    if kind == "cut_cluster":
        # the first cut falls in the middle of the set's first dense group of samples (index 500: inside blob 0 of
        # the three-blob set, inside the single cluster of the converged set), the rest evenly
        return [0] + [500 + ((n - 500) * r) // (W - 1) for r in range(W - 1)] + [n] if W > 1 else [0, n]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", ["even", "ragged", "empty", "cut_cluster"])
@pytest.mark.parametrize("W", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("name", ["three_blobs", "spread100k", "converged2k"])
def test_stage_functions_equal_one_engine_bit_for_bit(engines, orc, name, W, kind):
    """W engines on device 0, the test doing the exchanges: every rank's ordinary getters return the single engine's
    bits.  Sets of at most 4096 samples are run through BOTH forms (the gathered form is what ShardedFilter picks;
    the distributed form must agree with it)."""
    s = scored_set(engines, orc, name)
    n = s.shape[0]
    cuts = splits(n, W, kind)
    assert cuts[0] == 0 and cuts[-1] == n and all(b >= a for a, b in zip(cuts, cuts[1:])) and len(cuts) == W + 1
    if kind == "empty" and W > 1:
        assert any(b == a for a, b in zip(cuts, cuts[1:]))
    want = reference_stats(engines[0], s)
    assert want["n"][0] >= (3 if name == "three_blobs" else 1)
    for force in ([False, True] if n <= 4096 else [False]):
        bs = make_ranks(engines, s, cuts)
        route, _ = run_stages(bs, s, cuts, force_distributed=force)
        assert route == ("gathered" if n <= 4096 and not force else "distributed")
        for r, b in enumerate(bs):
            assert_same_bits(read_stats(b.pf), want, (name, W, kind, route, r))


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [4096, 4097])
def test_where_the_regimes_meet(engines, orc, n):
    """4096 samples in more than 1024 bins: the gathered form declines and the distributed form takes over; 4097
    samples go to the distributed form directly.  Both equal the single engine."""
    rng = np.random.default_rng(n)
    s = np.zeros((n, 4))
    s[:, 0] = rng.uniform(-40, 40, n)
    s[:, 1] = rng.uniform(-40, 40, n)
    s[:, 2] = rng.uniform(-np.pi, np.pi, n)
    s[:, 3] = rng.uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    want = reference_stats(engines[0], s)
    cuts = splits(n, 3, "ragged")
    bs = make_ranks(engines, s, cuts)
    if n == 4096:
        import torch
        soa = torch.cat([b.stats_local_soa() for b in bs], dim=1).contiguous()
        assert [b.stats_gathered(soa, n) for b in bs] == [0, 0, 0]  # declined: more than 1024 bins
    route, _ = run_stages(bs, s, cuts)
    assert route == "distributed"
    for b in bs:
        assert_same_bits(read_stats(b.pf), want, n)


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("why", ["key_out_of_range", "option"])
@pytest.mark.parametrize("name", ["three_blobs", "spread100k"])
def test_host_route_equals_the_single_engine_and_the_oracle(engines, orc, name, why):
    """A key outside the packing range on ONE rank (x = 5e6 m), or BPF_OPT_STATS_HOST = 1, sends every rank down the
    host route.  The result is, bit for bit, the BPF_OPT_STATS_HOST = 1 evaluation of one engine holding the set, and
    on the three-blob set -- the one test_cluster_stats_of_loaded_multimodal_set pins the single engine's host
    evaluation to the oracle with -- the oracle's serial evaluation bit for bit (the exact branch of
    _assert_stats_equal).  On the 100 000-sample spread set the single engine's own host evaluation is not the
    oracle's to the bit: measured on the GPU box, 14 of its 31 336 clusters differ by one ulp in mean[2] (the atan2 of
    the two circular sums; every weight, count, mean x / y and covariance is equal), with and without the far sample.
    The engine's host code calls libm's sin and cos, the oracle's compiler merged the pair into sincos, and the two
    differ in the last bit for a few arguments in 100 000.  That is a property of the host evaluation this change
    leaves as it is; there the oracle is held to the summation budgets instead (exact=False: counts and labels
    exact, 1e-12 / 1e-10)."""
    import badger_amcl_amd.pf as hpf
    from test_gpu_next_rows import _assert_stats_equal, _oracle_stats
    s = scored_set(engines, orc, name).copy()
    n = s.shape[0]
    if why == "key_out_of_range":
        s[n - 7, 0] = 5.0e6  # in the last rank's slice only
    cuts = splits(n, 3, "even")
    single = reference_stats(engines[0], s, host=True)
    bs = make_ranks(engines, s, cuts)
    if why == "option":
        for b in bs:
            b.e.set_option(hpf.OPT_STATS_HOST, 1)
    try:
        route, _ = run_stages(bs, s, cuts)
        assert route == "host"
        want = _oracle_stats(orc, s, n)
        for r, b in enumerate(bs):
            assert_same_bits(read_stats(b.pf), single, (name, why, r))
            if name == "three_blobs":
                _assert_stats_equal(b.pf, want, exact=True)
            else:
                assert_no_tie(want)
                _assert_stats_equal(b.pf, want, exact=False, set_atol=1e-7)
    finally:
        for b in bs:
            b.e.set_option(hpf.OPT_STATS_HOST, 0)


def test_stages_out_of_order_are_refused(engines, orc):
    s = scored_set(engines, orc, "three_blobs")
    b = make_ranks(engines, s, [0, s.shape[0]])[0]
    import ctypes as C
    import torch
    p, n = C.c_void_p(), C.c_size_t()
    assert b.e.lib.bpf_shard_stats_local_sums_dev(b.e.h, C.byref(p), C.byref(n)) == 2  # BPF_ERR_NOT_CONFIGURED
    bins, _ = b.stats_local_bins(0)
    assert b.e.lib.bpf_shard_stats_finish_dev(b.e.h, C.c_void_p(bins.data_ptr())) == 2
    # the slice changes between two stages: the stages in progress are void
    b.pf.fillWeights(1.0 / s.shape[0])
    cnt = (C.c_int * 1)(int(bins.shape[1]))
    out = C.c_int()
    assert b.e.lib.bpf_shard_stats_label_dev(b.e.h, C.c_void_p(bins.data_ptr()), cnt, 1, int(bins.shape[1]),
                                             C.byref(out)) == 2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 3, 5
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CYCLES = 2
ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion


def _scenario(cloud):
    from oracle import pyoracle as orc
    return orc, Scenario(orc, size=400, n=6000, beams=181, cloud=cloud)


def _worker(rank, world, port, out_dir, cloud, resampler, exchange):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    staged = exchange == "mailbox-staged"
    orc, sc = _scenario(cloud)
    n = sc.samples.shape[0]
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world
    e = bpf.Engine(0)
    spare = bpf.Engine(0)  # a single engine for the LOCAL evaluation of this rank's slice
    spare_pf = bpf.ParticleFilter(spare, 100, n, 0.0, 0.0, 85.0)
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    m, scn, pf, data = shard.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21)
    pf.setResampleModel(resampler)
    if staged:
        e.set_option(5, 0)  # BPF_OPT_FUSED_RESAMPLE: the mailbox step stage by stage
    b = HipShardBackend(e, scn, pf, torch.device("cuda", 0))
    b.kld_device_min = 512 if cloud == "spread" else 8192
    calls = []
    for name in ("stats_gathered", "stats_local_bins", "stats_label", "stats_local_sums", "stats_finish", "stats_host"):
        def wrap(fn=getattr(b, name), name=name):
            def f(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return f
        setattr(b, name, wrap())
    sf = ShardedFilter(b, dist, first_window=1024, exchange="mailbox" if staged else exchange)
    assert sf.mailbox == (exchange != "collective")
    od = bpf.Odom(e)
    od.setModel(*ODOM)

    def query(tag):
        """The global statistics, and a second query from the cache: no new stage calls."""
        before = len(calls)
        nc, mean, cov = sf.compute_cluster_stats()
        assert len(calls) > before, "a query after the set changed must evaluate"
        mark = len(calls)
        cl = [sf.get_cluster(k) for k in range(nc)]
        assert sf.get_cluster(nc) is None
        bw, bp = sf.get_max_weight_pose()
        nc2, mean2, cov2 = sf.compute_cluster_stats()
        assert len(calls) == mark, "cached: no new stage calls"
        assert nc2 == nc and np.array_equal(mean, mean2) and np.array_equal(cov, cov2, equal_nan=True)
        st = dict(n=np.array([nc]), set_mean=np.array(mean), set_cov=np.array(cov),
                  weight=np.array([c[0] for c in cl]), mean=np.array([c[1] for c in cl]).reshape(nc, 3),
                  count=np.array([c[2] for c in cl]), cov=np.array([c[3] for c in cl]).reshape(nc, 5),
                  best_w=np.array([bw]), best_pose=np.array(bp), route=sf.stats_route)
        # the engine's own getters return the installed GLOBAL values while the slice stands
        assert_same_bits(read_stats(pf), {k: v for k, v in st.items() if k != "route"}, tag)
        return st

    def local_is_fresh(tag, global_st):
        """After the slice changed the plain getter evaluates the NEW slice locally: equal to a single engine loaded
        with the slice, and (the slice being a part of the set) not the old global result."""
        cur = pf.getCurrentSet().samples
        got = read_stats(pf)
        if cur.shape[0]:
            spare_pf.initWithSamples(np.ascontiguousarray(cur))
            assert_same_bits(got, read_stats(spare_pf), tag)
        assert not np.array_equal(got["best_w"], global_st["best_w"]), tag

    recs = []
    last = query("initial")
    for cycle in range(CYCLES):
        sf.update_action(od, bpf.OdomData(*ODATA))
        sf.update_sensor(data)
        local_is_fresh(("sensor", cycle), last)
        w_after = pf.getCurrentSet().samples.copy()
        after_sensor = query(("sensor", cycle))
        sf.update_resample()
        st = sf.state()
        local_is_fresh(("resample", cycle), after_sensor)
        last = query(("resample", cycle))
        recs.append(dict(w=w_after, after_sensor=after_sensor, after_resample=last,
                         samples=pf.getCurrentSet().samples.copy(), M=st.sample_count))
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(recs, dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    spare.close()
    e.close()


FILTER_CASES = [(w, r, c, x) for w in (2, 3) for r in (0, 1) for c in ("converged", "spread")
                for x in ("mailbox", "collective")] + \
               [(2, 0, "converged", "mailbox-staged"), (3, 0, "spread", "mailbox-staged")]


@pytest.mark.parametrize("world,resampler,cloud,exchange", FILTER_CASES)
def test_sharded_filter_statistics(tmp_path, orc, world, resampler, cloud, exchange):
    """update_action -> update_sensor -> statistics -> update_resample -> statistics, two cycles.  After update_sensor
    the reference is one engine loaded with the set the shards really hold; after update_resample it is the unsharded
    filter's own cycle; both bit for bit, and the oracle within the budgets of test_gpu_next_rows.  The workers also
    hold test 5: the cache (no stage calls on a second query), its invalidation by every step (mailbox one-call,
    mailbox staged, collectives), and the plain getter's LOCAL evaluation once the slice has changed."""
    import torch.multiprocessing as mp
    from test_gpu_next_rows import _assert_stats_equal, _oracle_stats
    sys.path.insert(0, HERE)
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path), cloud, resampler, exchange), nprocs=world, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r), allow_pickle=True) for r in range(world)]

    import badger_amcl_amd as bpf
    _, sc = _scenario(cloud)
    n = sc.samples.shape[0]
    e, e2 = bpf.Engine(0), bpf.Engine(0)
    m, scn, pf, data = sc.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21)
    pf.setResampleModel(resampler)
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    keys = ["n", "set_mean", "set_cov", "weight", "mean", "count", "cov", "best_w", "best_pose"]
    for cycle in range(CYCLES):
        od.updateAction(pf, bpf.OdomData(*ODATA))
        scn.updateSensor(pf, data)
        rr = [recs[k][cycle] for k in range(world)]
        held = np.ascontiguousarray(np.concatenate([r["w"] for r in rr]))
        want = reference_stats(e2, held)
        want_orc = _oracle_stats(orc, held, n)
        assert_no_tie(want_orc)
        for r in rr:
            assert_same_bits({k: r["after_sensor"][k] for k in keys}, want, ("sensor", cycle))
            assert r["after_sensor"]["route"] == ("gathered" if held.shape[0] <= 4096 else "distributed")
            _assert_stats_equal(Recorded(r["after_sensor"]), want_orc, exact=False)
        pf.updateResample()
        M = pf.getState().sample_count
        want = read_stats(pf)
        want_orc = _oracle_stats(orc, pf.getCurrentSet().samples, n)
        assert_no_tie(want_orc)
        for r in rr:
            assert r["M"] == M
            assert_same_bits({k: r["after_resample"][k] for k in keys}, want, ("resample", cycle))
            assert r["after_resample"]["route"] == ("gathered" if M <= 4096 else "distributed")
            _assert_stats_equal(Recorded(r["after_resample"]), want_orc, exact=False)
    e.close()
    e2.close()
