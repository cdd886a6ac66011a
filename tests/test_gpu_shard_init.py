"""A sharded set initialised on its ranks (include/badger_pf.h, bpf_shard_init_with_*, bpf_shard_tree_*): W engines
together must hold, bit for bit, what ONE engine holds after bpf_pf_init_with_gaussian / bpf_pf_init_with_random_poses
with the same max_samples and rng state -- samples, weights, the rng state on every rank, the leaf and bin counts of
the GLOBAL set's histogram tree, w_slow / w_fast / converged -- and the cycle that follows must go on as the one
engine's does.

Three harnesses: the stage functions on W engines in one process with the exchange done by torch ops on the device
(any contiguous split); ShardedFilter on W engines in one process over a thread-based stand-in for torch.distributed
(every W up to 16 without 16 processes: the follow-on cycle through the stage functions); and two processes on the one
GPU over the mailbox and over gloo."""
import os
import socket
import sys
import threading

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kld_bins_ref  # noqa: E402
import pose_check_ref as ref  # noqa: E402
from scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu

ROT = ((0.8, -0.6, 0.0), (0.6, 0.8, 0.0), (0.0, 0.0, 1.0))
SIGMA = (0.15, 0.1, 0.05)
ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion
ROUTE_DEVICE, ROUTE_HOST, ROUTE_BINS, ROUTE_KEYS = 1, 2, 3, 4
WORLDS = [1, 2, 3, 8, 16]


# ---------------------------------------------------------------------------------------------------- helpers
_SCENARIOS = {}


def scenario(orc, size):
    """size 400: the map of the sharded tests; size 2000: the bench-size map (100 m x 100 m)."""
    if size not in _SCENARIOS:
        _SCENARIOS[size] = Scenario(orc, size=size, n=256, beams=181)
    return _SCENARIOS[size]


class Pool:
    """[0]: the single engine; [1 ..]: the ranks.  Every engine carries the map of the scenario asked for last."""

    def __init__(self):
        import badger_amcl_amd as bpf
        torch.cuda.set_device(0)  # torch's context first, as in the sharded workers; the engines run on its stream
        torch.zeros(1, device="cuda")
        self.engines = [bpf.Engine(0) for _ in range(17)]
        self.held = [None] * 17
        self.keep = [None] * 17

    def filter(self, k, orc, size, n, alpha=(0.0, 0.0), seed=17, gen3d=False):
        import badger_amcl_amd as bpf
        e = self.engines[k]
        sc_ = scenario(orc, size)
        if self.held[k] != (size, gen3d):
            m, scn, _, data = sc_.gpu_objects(e, 181, "lf")
            om = _attach_3d_map(e)[0] if gen3d else None
            self.keep[k] = (m, scn, data, om)
            self.held[k] = (size, gen3d)
        pf = bpf.ParticleFilter(e, 100, n, alpha[0], alpha[1], 85.0)
        pf.srand48(seed)
        return pf

    def scanner(self, k):
        return self.keep[k][1], self.keep[k][2]

    def close(self):
        self.keep = []
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


def _attach_3d_map(e):
    """a small 3-D map on a planar engine: the 3-D generator needs nothing else (test_gpu_pose_check.py)"""
    import badger_amcl_amd as bpf
    mn, mx = np.array([-40, -30, 0], dtype=np.int32), np.array([60, 50, 3], dtype=np.int32)
    cols = int((mx[0] - mn[0] + 1) * (mx[1] - mn[1] + 1))
    nz = int(mx[2] - mn[2] + 1)
    om = bpf.OctoMap(e, 0.05)
    om.setDistancesLUT(np.zeros(cols, dtype=np.uint32), np.zeros(nz, dtype=np.uint8), mn, mx, 0.3)
    return om, ref.FreeSpace.octo(list(mn), list(mx), 0.05)


def splits(n, W, kind):
    if kind == "even":
        return [(n * r) // W for r in range(W + 1)]
    if kind == "ragged":
        inner = np.sort(np.random.default_rng(W).integers(1, n, W - 1)) if W > 1 else np.array([], dtype=int)
        return [0] + [int(v) for v in inner] + [n]
    if kind == "empty":
        # shards of 0 samples (ranks 0, 4, ..) and of 1 sample (ranks 2, 6, ..) among full ones
        small = {r: (0 if r % 4 == 0 else 1) for r in range(W) if r % 4 in (0, 2)}
        full = [r for r in range(W) if r not in small]
        if not full:
            small.pop(W - 1)
            full = [W - 1]
        rest = n - sum(small.values())
        sizes = [small.get(r, 0) for r in range(W)]
        for i, r in enumerate(full):
            sizes[r] = (rest * (i + 1)) // len(full) - (rest * i) // len(full)
        return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
    raise ValueError(kind)


def read_set(pf):
    st = pf.getState()
    s = pf.getCurrentSet().samples if st.sample_count > 0 else np.zeros((0, 4))
    return s, st


def make_ranks(pool, orc, W, size, n, **kw):
    from badger_amcl_amd.sharded import HipShardBackend
    out = []
    for r in range(W):
        pf = pool.filter(1 + r, orc, size, n, **kw)
        scn, _ = pool.scanner(1 + r)
        out.append(HipShardBackend(pool.engines[1 + r], scn, pf, torch.device("cuda", 0)))
    return out


def global_tree(bs, cuts):
    """The exchange of the bin lists (or of the raw keys) by torch ops; returns every rank's (leaf, bins)."""
    W = len(bs)
    lists = [b.tree_local_bins(cuts[r]) for r, b in enumerate(bs)]
    nbs = [int(l[0].shape[1]) for l in lists]
    for r in range(W):
        assert nbs[r] <= cuts[r + 1] - cuts[r]
        if nbs[r] > 1 and not lists[r][1]:
            firsts = lists[r][0][1].cpu().numpy()
            assert np.all(np.diff(firsts) > 0) and firsts[0] == cuts[r] and firsts[-1] < cuts[r + 1]
    if any(l[1] for l in lists):
        keys = torch.cat([b.tree_local_keys() for b in bs], dim=1).t().contiguous().cpu().numpy()
        assert keys.shape == (cuts[-1], 3)
        return [b.tree_from_keys(keys) for b in bs]
    pad = max(max(nbs), 1)
    all_bins = torch.zeros((W, 2, pad), dtype=torch.int64, device=bs[0].device)
    for r, l in enumerate(lists):
        all_bins[r, :, :nbs[r]] = l[0]
    return [b.tree_merge(all_bins, nbs, pad) for b in bs]


def check_against_single(bs, cuts, pf1, counts, what):
    """Concatenated samples and weights, rng, counts, averages, converged: the single engine's bits."""
    want, st1 = read_set(pf1)
    n = want.shape[0]
    got = []
    for r, b in enumerate(bs):
        s, st = read_set(b.pf)
        assert st.sample_count == cuts[r + 1] - cuts[r], (what, r)
        assert b.pf.getRngState() == pf1.getRngState(), (what, r)
        assert (st.leaf_count, st.bin_count) == (st1.leaf_count, st1.bin_count) == counts[r], (what, r)
        assert (st.w_slow, st.w_fast, st.converged) == (st1.w_slow, st1.w_fast, st1.converged) == (0.0, 0.0, 0)
        got.append(s)
    got = np.concatenate(got)
    assert got.shape == want.shape and np.array_equal(got, want), what
    assert np.all(want[:, 3] == 1.0 / n)
    return want, st1


def oracle_counts(orc, samples, mode):
    t = orc.KDTree()
    for p in samples[:, :3]:
        t.insert_pose(p, 1.0)
    return (t.leaf_count(), t.node_count()) if mode == 0 else (t.node_count(), t.node_count())


def do_init(target, kind, mean):
    """target: (gaussian(mean, rot, sigma), random()) of one engine or of one rank."""
    if kind == "gaussian":
        return target[0](mean, ROT, SIGMA)
    return target[1]()


def init_everywhere(pool, orc, bs, cuts, pf1, kind, mean, check=None, gen3d=False, kld=0):
    import badger_amcl_amd.pf as hpf
    n = cuts[-1]
    for pf in [pf1] + [b.pf for b in bs]:
        pf.setKldCount(kld)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D if gen3d else hpf.RANDOM_POSE_FREE_SPACE_2D)
        if check is not None:
            pf.setUniformPoseCheck(*check)
    do_init((pf1.initWithGaussian, pf1.initWithRandomPoses), kind, mean)
    for r, b in enumerate(bs):
        lo, cnt = cuts[r], cuts[r + 1] - cuts[r]
        do_init((lambda m, ro, s: b.init_gaussian(m, ro, s, lo, cnt, n), lambda: b.init_random_poses(lo, cnt, n)),
                kind, mean)
        st = b.pf.getState()
        assert (st.sample_count, st.leaf_count, st.bin_count) == (cnt, -1, -1)  # the tree is marked as not built
        assert b.tree_last_route() == 0
    return global_tree(bs, cuts)


# ---------------------------------------------------------------------------------------------------- stage functions
@pytest.mark.parametrize("split", ["even", "ragged", "empty"])
@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("kind,kld", [("gaussian", 0), ("random", 0), ("random", 1)])
def test_init_stages_equal_one_engine(pool, orc, kind, kld, W, split):
    """6 000 samples.  Gaussian: converged, a handful of bins; random: spread over the free space of the 400 x 400
    map, fewer than 8 192 distinct keys either way: the host tree of the merged keys (kld 1: the bin count, no tree)."""
    n = 6000
    cuts = splits(n, W, split)
    assert cuts[0] == 0 and cuts[-1] == n and len(cuts) == W + 1 and all(b >= a for a, b in zip(cuts, cuts[1:]))
    if split == "empty" and W > 1:
        assert cuts[1] == 0 and (W < 3 or cuts[3] - cuts[2] == 1)
    pf1 = pool.filter(0, orc, 400, n)
    bs = make_ranks(pool, orc, W, 400, n)
    counts = init_everywhere(pool, orc, bs, cuts, pf1, kind, scenario(orc, 400).pose, kld=kld)
    want, st1 = check_against_single(bs, cuts, pf1, counts, (kind, kld, W, split))
    assert (st1.leaf_count, st1.bin_count) == oracle_counts(orc, want, kld)
    if kld == 1:
        assert st1.leaf_count == kld_bins_ref.set_count(want, kld_bins_ref.BINS, orc.KDTree)
    assert (st1.bin_count < 200) if kind == "gaussian" else (1000 < st1.bin_count < 8192)
    for b in bs:
        assert b.tree_last_route() == (ROUTE_BINS if kld else ROUTE_HOST)


@pytest.mark.parametrize("n,W,split", [(100000, 1, "even"), (100000, 2, "even"), (100000, 3, "ragged"),
                                       (100000, 8, "empty"), (100000, 16, "even"), (1000000, 3, "ragged")])
def test_free_space_init_on_the_bench_map_takes_the_device_tree(pool, orc, n, W, split):
    """Global localisation on the 2000 x 2000 map: more than 8 192 distinct keys, so the tree of the merged keys is
    grown on the device on every rank -- asserted, not assumed -- and equals the one engine's and the oracle's.
    Seed 17: the oracle's own tree of these sets is 40 levels deep at 100 000 samples (96 229 bins) and 50 at
    1 000 000 (697 153 bins), checked on the CPU with pyoracle.KDTree's counts beside a restatement that tracks the
    depth: far below the device tree's 256-level bound."""
    cuts = splits(n, W, split)
    pf1 = pool.filter(0, orc, 2000, n)
    bs = make_ranks(pool, orc, W, 2000, n)
    counts = init_everywhere(pool, orc, bs, cuts, pf1, "random", None)
    want, st1 = check_against_single(bs, cuts, pf1, counts, (n, W, split))
    assert st1.bin_count > 8192
    for b in bs:
        assert b.tree_last_route() == ROUTE_DEVICE
    assert (st1.leaf_count, st1.bin_count) == oracle_counts(orc, want, 0)
    # BINS mode on the same set: the count of the merged keys, no tree
    for pf in [pf1] + [b.pf for b in bs]:
        pf.srand48(17)
    counts = init_everywhere(pool, orc, bs, cuts, pf1, "random", None, kld=1)
    want2, st2 = check_against_single(bs, cuts, pf1, counts, (n, W, split, "bins"))
    assert np.array_equal(want2, want) and st2.leaf_count == st2.bin_count == st1.bin_count
    assert all(b.tree_last_route() == ROUTE_BINS for b in bs)


@pytest.mark.parametrize("gen3d", [False, True])
@pytest.mark.parametrize("check", [(0.0, 0.5), (10.0, 0.5)])
def test_pose_check_as_reference_and_3d_generator(pool, orc, check, gen3d):
    """K = 0 and K = 4 rejected trials per call, the 2-D and the 3-D free-space generator, against the single engine
    and the Python restatement of the generator (pose_check_ref.py)."""
    n, W = 5000, 3
    assert ref.retries(*check) in (0, 4)
    cuts = splits(n, W, "ragged")
    pf1 = pool.filter(0, orc, 400, n, gen3d=gen3d)
    bs = make_ranks(pool, orc, W, 400, n, gen3d=gen3d)
    rng0 = pf1.getRngState()
    counts = init_everywhere(pool, orc, bs, cuts, pf1, "random", None, check=check, gen3d=gen3d)
    want, st1 = check_against_single(bs, cuts, pf1, counts, (check, gen3d))
    sc_ = scenario(orc, 400)
    fs = ref.FreeSpace.octo([-40, -30, 0], [60, 50, 3], 0.05) if gen3d else ref.FreeSpace.planar(
        ref.free_cells_2d(sc_.cells, sc_.lut, sc_.map_factors[2]), sc_.size, sc_.size, sc_.origin, sc_.res)
    r = ref.Rng(rng0)
    assert np.array_equal(want[:, :3], np.array(ref.init_with_pose_fn(r, n, ref.FastGen(fs, *check))))
    assert pf1.getRngState() == r.s


@pytest.mark.parametrize("kld", [0, 1])
def test_key_outside_the_packing_range_takes_the_keys_route(pool, orc, kld):
    """x = 5e6 m: floor(x / 0.5 m) does not fit the packed key's 24 bits.  Every rank raises the flag, the raw keys
    cross, the host tree gives the single engine's counts."""
    n, W = 3000, 3
    cuts = splits(n, W, "ragged")
    pf1 = pool.filter(0, orc, 400, n)
    bs = make_ranks(pool, orc, W, 400, n)
    counts = init_everywhere(pool, orc, bs, cuts, pf1, "gaussian", (5.0e6, 1.0, 0.3), kld=kld)
    want, st1 = check_against_single(bs, cuts, pf1, counts, ("far", kld))
    assert (st1.leaf_count, st1.bin_count) == oracle_counts(orc, want, kld)
    assert all(b.tree_last_route() == ROUTE_KEYS for b in bs)


def test_refusals_leave_the_set_untouched(pool, orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = 2000
    b = make_ranks(pool, orc, 1, 400, n)[0]
    b.pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    b.init_random_poses(0, n, n)
    before, rng0 = b.pf.getCurrentSet().samples.copy(), b.pf.getRngState()
    # BPF_POSE_CHECK_SENSOR_MODEL: out of scope on the sharded path, as bpf_shard_begin_resample has it
    b.pf.setUniformPoseCheck(10.0, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)
    with pytest.raises(bpf.BpfError) as ei:
        b.init_random_poses(0, n, n)
    assert ei.value.code == 4
    b.pf.setUniformPoseCheck(0.0, 0.5)
    # global_count has to be the engine's max_samples; the range has to lie inside it
    for args in [(0, n - 1, n - 1), (0, n, n + 1), (1, n, n), (-1, 5, n)]:
        with pytest.raises(bpf.BpfError) as ei:
            b.init_random_poses(*args)
        assert ei.value.code == 1, args
        with pytest.raises(bpf.BpfError) as ei:
            b.init_gaussian((0, 0, 0), ROT, SIGMA, *args)
        assert ei.value.code == 1, args
    # the capacity refusal on the GLOBAL stream use (10, 0.999999: K ~ 2.3 M trials per call)
    b.pf.setUniformPoseCheck(10.0, 0.999999)
    with pytest.raises(bpf.BpfError) as ei:
        b.init_random_poses(0, 1, n)
    assert ei.value.code == 8
    assert np.array_equal(b.pf.getCurrentSet().samples, before) and b.pf.getRngState() == rng0
    b.pf.setUniformPoseCheck(0.0, 0.5)


# ---------------------------------------------------------------------------------------------------- follow-on
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


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("kind", ["gaussian", "random"])
def test_cycle_after_the_init_equals_one_engine(pool, orc, kind, W, resampler):
    """ShardedFilter.init_* on W engines, then one motion update, one likelihood-field sensor update and one resample
    through the stage functions.  Poses after the motion update, the resampled set, M, leaf / bin counts, the rng state
    and the converged flag: the single engine's bits.  The normalised weights are held to n 2^-53 relative: the W
    totals are added in rank order where one engine adds its tiles, and two orders of an n-term double sum differ by
    rounding only (the neighbouring sharded tests hold them to 1e-12 for the same reason).  The systematic resampler
    runs without any host-side key gather: the init left the leaf count."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import ShardedFilter
    n = 6000
    sc_ = scenario(orc, 400)
    pf1 = pool.filter(0, orc, 400, n, seed=21)
    bs = make_ranks(pool, orc, W, 400, n, seed=21)
    for pf in [pf1] + [b.pf for b in bs]:
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.setKldCount(0)
        pf.setUniformPoseCheck(0.0, 0.5)

    def forbidden():
        raise AssertionError("the per-particle key gather must not run after an init")

    def body(rank, dist):
        b = bs[rank]
        b.local_pose_keys = forbidden
        b.kld_device_min = 512 if kind == "random" else 8192
        sf = ShardedFilter(b, dist, rank=rank, world=W, first_window=1024, exchange="collective", init_follows=True)
        do_init((sf.init_with_gaussian, sf.init_with_random_poses), kind, sc_.pose)
        st = b.pf.getState()
        rec = dict(init=read_set(b.pf)[0], leaf0=sf.leaf_count, bins0=sf.bin_count, route=sf.tree_route,
                   eleaf0=st.leaf_count, rng0=b.pf.getRngState())
        od = bpf.Odom(b.e)
        od.setModel(*ODOM)
        sf.update_action(od, bpf.OdomData(*ODATA))
        rec["moved"] = read_set(b.pf)[0]
        sf.update_sensor(pool.scanner(1 + rank)[1])
        rec["scored"] = read_set(b.pf)[0]
        sf.update_resample()
        st = sf.state()
        rec.update(after=read_set(b.pf)[0], M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count,
                   rng=b.pf.getRngState(), conv=st.converged, miss=st.cdf_miss)
        return rec

    recs = run_ranks(W, body)
    do_init((pf1.initWithGaussian, pf1.initWithRandomPoses), kind, sc_.pose)
    s0, st0 = read_set(pf1)
    assert np.array_equal(np.concatenate([r["init"] for r in recs]), s0)
    for r in recs:
        assert (r["leaf0"], r["bins0"], r["eleaf0"]) == (st0.leaf_count, st0.bin_count, st0.leaf_count)
        assert r["rng0"] == pf1.getRngState() and r["route"] == "host"
    od = bpf.Odom(pool.engines[0])
    od.setModel(*ODOM)
    od.updateAction(pf1, bpf.OdomData(*ODATA))
    assert np.array_equal(np.concatenate([r["moved"] for r in recs]), read_set(pf1)[0])
    scn, data = pool.scanner(0)
    scn.updateSensor(pf1, data)
    w1 = read_set(pf1)[0]
    w = np.concatenate([r["scored"] for r in recs])
    assert np.array_equal(w[:, :3], w1[:, :3])
    rel = np.max(np.abs(w[:, 3] - w1[:, 3]) / w1[:, 3])
    print("normalised weights, W = %d: largest relative difference %.3g" % (W, rel))
    assert rel <= n * 2.0 ** -53
    pf1.updateResample()
    s2, st2 = read_set(pf1)
    assert np.array_equal(np.concatenate([r["after"] for r in recs])[:, :3], s2[:, :3])
    for k, r in enumerate(recs):
        assert (r["M"], r["leaf"], r["bins"], r["rng"], r["conv"]) == (
            st2.sample_count, st2.leaf_count, st2.bin_count, pf1.getRngState(), st2.converged)
        assert not r["miss"] and np.all(r["after"][:, 3] == 1.0 / st2.sample_count)
        assert r["after"].shape[0] == (st2.sample_count * (k + 1)) // W - (st2.sample_count * k) // W


# ---------------------------------------------------------------------------------------------------- two processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CYCLES = 2
N2 = 6000


def _scenario2(geometry=None):
    """geometry: None = the square 400 x 400 map, else a name of map_geometry.GEOMETRIES (a rectangle)."""
    from oracle import pyoracle as orc
    if geometry is None:
        return orc, Scenario(orc, size=400, n=256, beams=181)
    from map_geometry import GeoScenario
    return orc, GeoScenario.named(orc, geometry, n=256, beams=181)


def _worker(rank, world, port, out_dir, resampler, exchange, geometry=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    orc, sc = _scenario2(geometry)
    e = bpf.Engine(0)
    m, scn, _, data = sc.gpu_objects(e, 181, "lf")
    pf = bpf.ParticleFilter(e, 100, N2, 0.0, 0.0, 85.0)
    pf.srand48(21)
    pf.setResampleModel(resampler)
    b = HipShardBackend(e, scn, pf, torch.device("cuda", 0))
    b.kld_device_min = 512

    def forbidden():
        raise AssertionError("the per-particle key gather must not run after an init")

    b.local_pose_keys = forbidden
    sf = ShardedFilter(b, dist, first_window=1024, exchange=exchange, init_follows=True)
    assert sf.mailbox == (exchange == "mailbox")
    sf.set_random_pose_generator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    sf.init_with_random_poses()
    st = pf.getState()
    recs = [dict(samples=pf.getCurrentSet().samples.copy(), leaf=sf.leaf_count, bins=sf.bin_count,
                 eleaf=st.leaf_count, ebins=st.bin_count, rng=pf.getRngState(), route=sf.tree_route, counts=sf.counts)]
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    for cycle in range(CYCLES):
        sf.update_action(od, bpf.OdomData(*ODATA))
        sf.update_sensor(data)
        sf.update_resample()
        st = sf.state()
        bw, bp = sf.get_max_weight_pose()
        recs.append(dict(samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                         bins=st.bin_count, rng=pf.getRngState(), conv=st.converged, miss=st.cdf_miss,
                         best_w=bw, best_pose=np.array(bp)))
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(recs, dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


@pytest.mark.parametrize("exchange", ["mailbox", "collective"])
@pytest.mark.parametrize("resampler", [0, 1])
def test_two_processes_init_and_two_cycles_equal_single_engine(tmp_path, resampler, exchange):
    """ShardedFilter.init_with_random_poses() in two processes on the one GPU -- over the mailbox (the engine's one-call
    form does the exchanges) and over gloo (staged through the host) -- then two full cycles and get_max_weight_pose."""
    _two_processes_against_single_engine(tmp_path, resampler, exchange, None)


def test_two_processes_init_on_a_rectangular_map_equals_single_engine(tmp_path):
    """The same on G1 of map_geometry.py (333 x 150, so that the free-space list's i-outer order and the two half
    sizes of the conversion back to the world matter): the two ranks' random poses are the single engine's."""
    _two_processes_against_single_engine(tmp_path, 0, "mailbox", "G1")


def _two_processes_against_single_engine(tmp_path, resampler, exchange, geometry):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path), resampler, exchange, geometry), nprocs=2, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r), allow_pickle=True) for r in range(2)]
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    orc, sc = _scenario2(geometry)
    if geometry is not None:
        first = np.concatenate([recs[0][0]["samples"], recs[1][0]["samples"]])
        assert sc.transposed_blind_fraction(first) >= 0.2 and sc.in_map(first).all()
    e = bpf.Engine(0)
    try:
        m, scn, _, data = sc.gpu_objects(e, 181, "lf")
        pf = bpf.ParticleFilter(e, 100, N2, 0.0, 0.0, 85.0)
        pf.srand48(21)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.initWithRandomPoses()
        st = pf.getState()
        assert np.array_equal(np.concatenate([recs[0][0]["samples"], recs[1][0]["samples"]]),
                              pf.getCurrentSet().samples)
        for r in (recs[0][0], recs[1][0]):
            assert (r["leaf"], r["bins"], r["eleaf"], r["ebins"]) == (st.leaf_count, st.bin_count) * 2
            assert r["rng"] == pf.getRngState() and r["route"] == "host" and r["counts"] == [N2 // 2, N2 - N2 // 2]
        od = bpf.Odom(e)
        od.setModel(*ODOM)
        for cycle in range(CYCLES):
            od.updateAction(pf, bpf.OdomData(*ODATA))
            scn.updateSensor(pf, data)
            pf.updateResample()
            st = pf.getState()
            bw, bp = pf.getMaxWeightPose()
            rr = [recs[k][1 + cycle] for k in range(2)]
            for r in rr:
                assert (r["M"], r["leaf"], r["bins"], r["rng"], r["conv"]) == (
                    st.sample_count, st.leaf_count, st.bin_count, pf.getRngState(), st.converged)
                assert not r["miss"]
                assert r["best_w"] == bw and np.array_equal(r["best_pose"], np.array(bp))
            merged = np.concatenate([r["samples"] for r in rr])
            assert np.array_equal(merged[:, :3], pf.getCurrentSet().samples[:, :3])
            assert np.all(merged[:, 3] == 1.0 / st.sample_count)
    finally:
        e.close()
