"""Pose search over a sharded filter (bpf_shard_search_poses and its three siblings, LocalShardedFilter.search_*,
ShardedFilter.search_*, localize): W engines on device 0 in one process, connected as a local world, against ONE
engine that searches the whole range.  The contract is exactness: every rank's rows are the single engine's rows,
byte for byte; the pruned forms' counters equal the numpy replay with the floor the ranks share behind their seeds
(tests/shard_search_ref.py), field for field.  Maps, scans and spaces are those of tests/test_gpu_pose_search.py.

The floor measured on an MI355X (scored_candidates summed over the ranks, with the floor / as stand-alone range calls,
the map's own scan; the replay gives the same figures): G1 lf K = 64 B = 8 W = 3: 89 854 / 97 213 of 134 573 (FLOOR_CASE
below, the one case asserted to save evaluations); G2 gompertz K = 64 B = 2 W = 2: 66 988 / 72 099 of 140 870; G1 lf
K = 1 B = 8 W = 2: 23 646 / 23 646 (the lattice map repeats itself: both halves hold a pose that scores as well, so
neither rank's tau is news to the other); G2 lf K = 1 B = 8 W = 3 and G3 lf K = 1024 B = 64 W = 4: no difference.
"With the floor never more" is NOT asserted: the floor changes which window a survivor is decided in, and an earlier
window can mean a lower tau of the rank's own."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_pruned_ref as ppr  # noqa: E402
import pose_search_ref as psr  # noqa: E402
import shard_search_ref as ssr  # noqa: E402
from test_gpu_pose_search import MAX_BEAMS, ORACLE_SPACES, blind_scan, geometry, scanner_on, window  # noqa: E402
from test_gpu_pose_search_pruned import scan_of  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 64, 1024)
STAT_FIELDS = ("block_candidates", "seed_candidates", "pruned_block_candidates", "expanded_block_candidates",
               "scored_candidates", "windows")
# the case whose replay decides that the floor saves evaluations: (map, model, K, B, W)
FLOOR_CASE = ("G1", "lf", 64, 8, 3)


class Ranks:
    """One single engine and, per world size, W engines with a filter each (the GLOBAL bounds), connected as one
    local world.  Maps and scanners are put on the engines by the tests."""

    def __init__(self):
        import badger_amcl_amd as bpf
        self.single = bpf.Engine(0)
        self.worlds = {}

    def world(self, W):
        import badger_amcl_amd as bpf
        from badger_amcl_amd.local_world import LocalShardedFilter
        if W not in self.worlds:
            engines = [bpf.Engine(0) for _ in range(W)]
            pfs = []
            for e in engines:
                pf = bpf.ParticleFilter(e, 100, 1000, 0.0, 0.0, 85.0)
                pf.srand48(7)
                pfs.append(pf)
            self.worlds[W] = (engines, LocalShardedFilter(pfs, kld_count=0))
        return self.worlds[W]

    def planar(self, W, geo, model, max_beams=MAX_BEAMS, kw=None):
        """(single engine's scanner, the world's filter, what keeps the maps alive)"""
        engines, f = self.world(W)
        keep = [scanner_on(e, geo, model, max_beams, kw) for e in [self.single] + engines]
        return keep[0][1], f, keep

    def close(self):
        for engines, f in self.worlds.values():
            f.close()
            for e in engines:
                e.close()
        self.single.close()


@pytest.fixture(scope="module")
def ranks():
    r = Ranks()
    yield r
    r.close()


# ------------------------------------------------------------------------------------ 1. the single engine's rows
@pytest.mark.parametrize("model", ["lf", "gompertz"])
@pytest.mark.parametrize("name,W", [("G1", 2), ("G2", 3), ("G3", 4)])
def test_rows_equal_the_single_engine(ranks, orc, name, W, model):
    """exhaustive and pruned, K = 1, 64, 1024; LocalShardedFilter compares the ranks' rows with each other"""
    geo = geometry(orc, name)
    sc, f, keep = ranks.planar(W, geo, model)
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES[name]
    total, _ = sc.searchSpace(headings, stride)
    if name == "G1":
        # every rank's share spans more than one window, and rank 1's starts inside one
        assert total // W > window() and (total // W) % window() != 0
    else:
        assert total % W != 0  # an uneven split of the candidates
        assert name != "G3" or sc.searchBlocks(stride, 8) % W != 0  # ... and of the blocks
    before = f.exchange_counts()
    for k in KS:
        want = sc.searchPoses(data, headings, stride, k)
        assert want.shape[0] == k
        assert f.search_poses(data, headings, stride, k).tobytes() == want.tobytes(), (name, W, model, k)
        got, stats = f.search_poses_pruned(data, headings, stride, k, 8)
        assert got.tobytes() == want.tobytes(), (name, W, model, k)
        assert sum(st["candidates"] for st in stats) == total
        print("sharded pruned search %s %s W=%d K=%d: scored %s of %d"
              % (name, model, W, k, [st["scored_candidates"] for st in stats], total))
    assert all(a > b for a, b in zip(f.exchange_counts(), before))


def test_ranges_inside_the_space_are_split_inside_the_range(ranks, orc):
    geo = geometry(orc, "G2")
    sc, f, keep = ranks.planar(3, geo, "lf")
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES["G2"]
    total, _ = sc.searchSpace(headings, stride)
    first, count = 1001, 70001
    assert first + count < total and count % 3 != 0
    for k in (1, 64):
        assert f.search_poses(data, headings, stride, k, first, count).tobytes() == \
            sc.searchPoses(data, headings, stride, k, first, count).tobytes()
    nb = sc.searchBlocks(stride, 8)
    fb, bc = 2, nb - 7
    assert bc > 3 and bc % 3 != 0
    for k in (1, 64):
        got, stats = f.search_poses_pruned(data, headings, stride, k, 8, fb, bc)
        assert got.tobytes() == sc.searchPosesPruned(data, headings, stride, k, 8, fb, bc).tobytes()
        assert [st["block_candidates"] for st in stats] == [n * headings for _, n in ssr.split(fb, bc, 3)]


def test_an_empty_share(ranks, orc):
    """fewer units than ranks: a rank without a share scores nothing, contributes an empty list and takes part in
    every exchange"""
    geo = geometry(orc, "G3")
    sc, f, keep = ranks.planar(4, geo, "lf")
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES["G3"]
    assert 0 < sc.searchBlocks(stride, 64) < 4
    for k in (1, 64):
        got, stats = f.search_poses_pruned(data, headings, stride, k, 64)
        assert got.tobytes() == sc.searchPoses(data, headings, stride, k).tobytes()
        shares = [n for _, n in ssr.split(0, sc.searchBlocks(stride, 64), 4)]
        assert 0 in shares
        for st, n in zip(stats, shares):
            assert st["block_candidates"] == n * headings
            if n == 0:
                assert all(v == 0 for v in st.values())
    # the exhaustive form: a count below W, and a space of fewer candidates than ranks
    assert sc.searchSpace(headings, stride)[0] > 10
    assert f.search_poses(data, headings, stride, 8, 5, 3).tobytes() == \
        sc.searchPoses(data, headings, stride, 8, 5, 3).tobytes()
    assert f.search_poses(data, headings, stride, 8, 5, 0).shape[0] == 0
    free = ((geo.cells == -1) & (geo.lut.astype(np.float64) > geo.map_factors[2])).T  # [i, j]
    few = [s for s in range(max(geo.size_x, geo.size_y), 0, -1) if 0 < free[::s, ::s].sum() < 4][0]
    assert 0 < sc.searchSpace(1, few)[0] < 4
    want = sc.searchPoses(data, 1, few, 8)
    assert 0 < want.shape[0] < 4
    assert f.search_poses(data, 1, few, 8).tobytes() == want.tobytes()


def test_blind_scan_prunes_nothing_and_orders_by_candidate(ranks, orc):
    geo = geometry(orc, "G1")
    sc, f, keep = ranks.planar(2, geo, "lf")
    headings, stride = ORACLE_SPACES["G1"]
    total, _ = sc.searchSpace(headings, stride)
    for k in (1, 1024):
        want = sc.searchPoses(blind_scan(geo), headings, stride, k)
        got, stats = f.search_poses_pruned(blind_scan(geo), headings, stride, k, 8)
        assert got.tobytes() == want.tobytes()
        assert np.all(got["score"] == 1.0) and np.array_equal(got["candidate"], np.arange(k))
        assert all(st["pruned_block_candidates"] == 0 for st in stats)
        assert sum(st["scored_candidates"] for st in stats) == total
        assert f.search_poses(blind_scan(geo), headings, stride, k).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------ 2. the floor
def _replay_inputs(sc, geo, data, name, block):
    headings, stride = ORACLE_SPACES[name]
    sp = psr.Space.of(geo, headings, stride)
    blocks, start, member = ppr.block_list(sp.ij, block)
    s = sp.samples(0, sp.total)
    sc.applyModelToSampleSet(data, s)
    scores = s[:, 3].reshape(-1, headings)
    assert np.all(np.isfinite(scores))
    bounds = sc.searchBounds(data, headings, stride, block)
    return headings, stride, sp, start, member, scores, bounds


@pytest.mark.parametrize("name,model,k,block,W", [FLOOR_CASE, ("G1", "lf", 1, 8, 2), ("G2", "gompertz", 64, 2, 2),
                                                  ("G2", "lf", 1, 8, 3), ("G3", "lf", 1024, 64, 4)])
def test_stats_equal_the_replay_with_the_floor(ranks, orc, name, model, k, block, W):
    """every rank's counters against the numpy replay of its call with the floor formed from the ranks' seed stages;
    the stand-alone range calls against the replay without it"""
    geo = geometry(orc, name)
    sc, f, keep = ranks.planar(W, geo, model)
    data = scan_of(geo)
    headings, stride, sp, start, member, scores, bounds = _replay_inputs(sc, geo, data, name, block)
    nb = start.shape[0] - 1
    got, stats = f.search_poses_pruned(data, headings, stride, k, block)
    want = sc.searchPoses(data, headings, stride, k)
    assert got.tobytes() == want.tobytes()
    assert want["score"].tobytes() == scores.reshape(-1)[want["candidate"]].tobytes()  # what the replay's tau rests on
    with_floor, floor = ssr.replay_world(bounds, scores, start, member, headings, k, 0, nb, W, shared=True)
    alone, _ = ssr.replay_world(bounds, scores, start, member, headings, k, 0, nb, W, shared=False)
    if floor is not None:
        assert floor <= want["score"][k - 1]
    for r, (st, rep) in enumerate(zip(stats, with_floor)):
        for field in STAT_FIELDS:
            assert st[field] == rep[field], (r, field, st, {n: v for n, v in rep.items() if n != "best"})
    sums = {}
    for r, (lo, n) in enumerate(ssr.split(0, nb, W)):
        _, st = sc.searchPosesPruned(data, headings, stride, k, block, lo, n, stats=True)
        for field in STAT_FIELDS:
            assert st[field] == alone[r][field], (r, field)
        for field in ("scored_candidates", "windows"):
            sums[field] = sums.get(field, 0) + st[field]
    scored = sum(st["scored_candidates"] for st in stats)
    print("floor %s %s K=%d B=%d W=%d: scored with the floor %d (%s), stand-alone %d, total %d; windows %d / %d"
          % (name, model, k, block, W, scored, [st["scored_candidates"] for st in stats], sums["scored_candidates"],
             sp.total, sum(st["windows"] for st in stats), sums["windows"]))
    if (name, model, k, block, W) == FLOOR_CASE:
        # decided by the replay, then required of the device
        assert sum(r["scored_candidates"] for r in with_floor) < sum(r["scored_candidates"] for r in alone)
        assert scored < sums["scored_candidates"]


# ------------------------------------------------------------------------------------ 3. the cloud scanner
def test_cloud_searches(ranks, orc):
    import badger_amcl_amd as bpf
    import test_gpu_pose_search_cloud_pruned as tc
    lut, _, max_dist = tc.hall(orc)
    engines, f = ranks.world(2)
    keep = [tc.scanner_on(e, lut, max_dist) for e in [ranks.single] + engines]
    sc = keep[0][1]
    data = bpf.PointCloudData(np.array(tc.cloud(orc, "cast")))
    headings, stride = 6, 1
    total, _ = sc.searchSpace(headings, stride)
    assert total > 2048
    for k in (1, 64):
        want = sc.searchPoses(data, headings, stride, k)
        assert want.shape[0] == k
        assert f.cloud_search_poses(data, headings, stride, k).tobytes() == want.tobytes()
        assert f.cloud_search_poses(data, headings, stride, k, 7, total - 20).tobytes() == \
            sc.searchPoses(data, headings, stride, k, 7, total - 20).tobytes()
        got, stats = f.cloud_search_poses_pruned(data, headings, stride, k, 4)
        assert got.tobytes() == want.tobytes()
        assert sum(st["candidates"] for st in stats) == total
        for st in stats:
            assert st["block_candidates"] == (st["seed_candidates"] + st["pruned_block_candidates"] +
                                              st["expanded_block_candidates"])


# ------------------------------------------------------------------------------------ 4. nothing else moves
def _world_run(orc, with_search):
    import badger_amcl_amd as bpf
    from test_gpu_local_world import ODATA, World, _cycle_scenario
    w = World(_cycle_scenario(orc), 2)
    try:
        f, recs, hits = w.f, [], None
        for c in range(2):
            f.update_action(None, bpf.OdomData(*ODATA))
            f.update_sensor(w.data)
            if with_search and c == 0:
                other = bpf.PlanarData(np.full(w.data.range_count_, 1.0), w.data.angles_, w.data.range_max_)
                hits = (f.search_poses(other, 4, 3, 32), f.search_poses_pruned(other, 4, 3, 32, 8)[0])
            recs.append(dict(sets=f.local_sets(), rng=f.rng_states()))
            f.update_resample()
            st = [(s.sample_count, s.leaf_count, s.converged, s.w_slow, s.w_fast, s.total) for s in f.rank_states()]
            recs.append(dict(sets=f.local_sets(), rng=f.rng_states(), M=f.sample_count, leaf=f.leaf_count,
                             bins=f.bin_count, states=st))
        return recs, hits
    finally:
        w.close()


def test_a_sharded_search_leaves_the_filter_as_it_found_it(orc):
    a, hits = _world_run(orc, True)
    b, _ = _world_run(orc, False)
    assert hits[0].shape[0] == 32 and hits[0].tobytes() == hits[1].tobytes()
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb)
        for key in ra:
            if key == "sets":
                assert all(x.tobytes() == y.tobytes() for x, y in zip(ra[key], rb[key])), step
            else:
                assert ra[key] == rb[key], (step, key)


# ------------------------------------------------------------------------------------ 5. refusals
def test_refusals(ranks, orc):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import _lib
    geo = geometry(orc, "G2")
    data = scan_of(geo)
    rp, ap = data.pointers()
    W = 3

    def codes(f, pruned, headings=4, cell_stride=1, k=8, block=8, first=0, count=-1):
        hits = [np.zeros(1100, dtype=bpf.pf.POSE_HIT_DTYPE) for _ in range(W)]
        ns = [C.c_int(0) for _ in range(W)]

        def call(r, h, lib):
            hp = hits[r].ctypes.data_as(C.POINTER(_lib.PoseHit))
            if pruned:
                return lib.bpf_shard_search_poses_pruned(h, rp, ap, data.range_count_, data.range_max_, headings,
                                                         cell_stride, block, first, count, k, hp, C.byref(ns[r]), None)
            return lib.bpf_shard_search_poses(h, rp, ap, data.range_count_, data.range_max_, headings, cell_stride,
                                              first, count, k, hp, C.byref(ns[r]))
        before = f.exchange_counts()
        got = f.codes(call)
        assert f.exchange_counts() == before  # refused before the first exchange, on every rank
        return got

    for model in ("prob", "beam"):
        sc, f, keep = ranks.planar(W, geo, model)
        assert codes(f, True) == [4] * W
        assert codes(f, False, k=0) == [1] * W
    sc, f, keep = ranks.planar(W, geo, "lf")
    total, nb = sc.searchSpace(4, 1)[0], sc.searchBlocks(1, 8)
    for pruned in (False, True):
        units = nb if pruned else total
        for kw in (dict(k=0), dict(k=1025), dict(first=units + 1), dict(first=-1), dict(count=units + 1),
                   dict(first=1, count=units), dict(count=-2), dict(headings=0), dict(cell_stride=0)):
            assert codes(f, pruned, **kw) == [1] * W, (pruned, kw)
    assert codes(f, True, block=3) == [1] * W
    # and the world goes on
    assert f.search_poses(data, 4, 1, 8).tobytes() == sc.searchPoses(data, 4, 1, 8).tobytes()
    # an engine without a connected world
    e = bpf.Engine(0)
    try:
        m, sc1 = scanner_on(e, geo, "lf")
        hits = np.zeros(8, dtype=bpf.pf.POSE_HIT_DTYPE)
        n = C.c_int()
        hp = hits.ctypes.data_as(C.POINTER(_lib.PoseHit))
        assert e.lib.bpf_shard_search_poses(e.h, rp, ap, data.range_count_, data.range_max_, 4, 1, 0, -1, 8, hp,
                                            C.byref(n)) == 2
        assert e.lib.bpf_shard_search_poses_pruned(e.h, rp, ap, data.range_count_, data.range_max_, 4, 1, 8, 0, -1, 8,
                                                   hp, C.byref(n), None) == 2
        pts = np.zeros((4, 3), dtype=np.float32)
        pp = pts.ctypes.data_as(C.POINTER(C.c_float))
        assert e.lib.bpf_shard_cloud_search_poses(e.h, pp, 4, 4, 1, 0, -1, 8, hp, C.byref(n)) == 2
        assert e.lib.bpf_shard_cloud_search_poses_pruned(e.h, pp, 4, 4, 1, 8, 0, -1, 8, hp, C.byref(n), None) == 2
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 6. ShardedFilter, both routes
@pytest.mark.parametrize("route", ["collectives", "engine"])
def test_sharded_filter_routes(ranks, orc, route):
    """in-process ranks over the thread stand-in for torch.distributed; "engine": the engines are connected as a
    local world, so the one-call forms carry the search"""
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    from test_gpu_shard_init import run_ranks
    W = 2
    geo = geometry(orc, "G1")
    sc, f, keep = ranks.planar(W, geo, "lf")
    engines, _ = ranks.world(W)
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES["G1"]
    k, block = 64, 8
    nb = sc.searchBlocks(stride, block)
    if route == "collectives":
        for e in engines:
            e.lib.bpf_shard_shutdown(e.h)
    backends = [HipShardBackend(engines[r], keep[1 + r][1], f.pfs[r], torch.device("cuda", 0)) for r in range(W)]
    try:
        def body(rank, dist):
            sf = ShardedFilter(backends[rank], dist, rank=rank, world=W, exchange="collective", init_follows=True)
            assert sf._engine_exchange() == (route == "engine")
            rows = sf.search_poses(data, headings, stride, k)
            pruned, st = sf.search_poses_pruned(data, headings, stride, k, block)
            part = sf.search_poses(data, headings, stride, k, 11, 70000)
            return rows, pruned, st, part

        out = run_ranks(W, body)
    finally:
        for e in engines:
            e.set_stream(None)
        if route == "collectives":
            f.connect()
    want = sc.searchPoses(data, headings, stride, k)
    for r, (rows, pruned, st, part) in enumerate(out):
        assert rows.tobytes() == want.tobytes() and pruned.tobytes() == want.tobytes()
        assert part.tobytes() == sc.searchPoses(data, headings, stride, k, 11, 70000).tobytes()
        if route == "collectives":  # no shared tau on this route: the stand-alone range call's counters
            lo, n = ssr.split(0, nb, W)[r]
            _, alone = sc.searchPosesPruned(data, headings, stride, k, block, lo, n, stats=True)
            assert st == alone


# ------------------------------------------------------------------------------------ 7. localize
def test_localize_equals_one_engine(ranks, orc):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    W, n = 3, 1000
    geo = geometry(orc, "G1")
    sc, f, keep = ranks.planar(W, geo, "lf")
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES["G1"]
    k = 64
    refine = (2, geo.res / 2, 2, 0.02, 2)
    moments = (2, geo.res / 2, 2, 0.02, 0.5, (0.01, 0.01, 0.01), (1.0, 1.0, 1.0))
    mixture = (0.5, 0.5, 8, (0.1, 0.1, 0.05))
    pf1 = bpf.ParticleFilter(ranks.single, 100, n, 0.0, 0.0, 85.0)
    pf1.srand48(7)
    for pf in f.pfs:
        pf.srand48(7)
    hits = sc.searchPosesPruned(data, headings, stride, k, 8)
    refined = sc.refinePoses(data, hits, *refine)
    rows = sc.poseMoments(data, refined, *moments[:5])
    comps = hpf.mixtureApplyMoments(hpf.mixtureFromHits(refined, n, *mixture), rows, moments[5], moments[6])
    pf1.initWithMixture(comps)
    for pruned in (True, False):
        for pf in f.pfs:
            pf.srand48(7)
        got = f.localize([kp[1] for kp in keep[1:]], data, headings, stride, k, refine, moments, mixture,
                         pruned=pruned)
        assert got.tobytes() == comps.tobytes()
        assert np.concatenate(f.local_sets()).tobytes() == pf1.getCurrentSet().samples.tobytes()
        assert f.rng_states() == [pf1.getRngState()] * W
        assert f.sample_count == n and f.counts == [n * (r + 1) // W - n * r // W for r in range(W)]
