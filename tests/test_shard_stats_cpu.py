"""gloo worlds of 1, 2, 3 and 8 (no GPU): ShardedFilter.compute_cluster_stats / get_cluster / get_max_weight_pose
over the oracle backend with the statistics stages restated in plain Python (shard_stats_ref.py).  Holds the
orchestration: the choice of the regime by the GLOBAL count, the two exchanges of the distributed form (ragged bin
lists, the limb form of the sums), the host route taken by EVERY rank when one rank asks for it, the cache and its
invalidation by the filter's steps.  The integer sums are exact, so they are compared with == across worlds."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ODOM = (2, (0.05, 0.04, 0.03, 0.02, 0.0))
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_stats(orc, samples, max_clusters):
    """(the call of tests/test_gpu_next_rows.py)"""
    t = orc.KDTree()
    for k in range(samples.shape[0]):
        t.insert_pose(samples[k, :3], samples[k, 3])
    return t.cluster_stats(samples, max_clusters)


def _set(name):
    """mixture: the 1 200-sample set of test_sharded_cpu.py, weights made non-uniform; blobs: three blobs of 400 whose
    members straddle the shard boundaries; spread: 5 000 spread samples (above 4 096: the distributed form),
    spread4000: 4 000 of them;
    *_far: the same with one pose at x = 5e6 m (a key outside the packing range) near the end of the set."""
    from oracle import pyoracle as orc
    from scenario import Scenario
    from badger_amcl_amd import synth
    base = name.split("_")[0]
    if base == "mixture":
        sc = Scenario(orc, size=200, n=1200, beams=61, cloud="mixture")
        s = sc.samples.copy()
    elif base == "blobs":
        sc = Scenario(orc, size=200, n=1200, beams=61, cloud="converged")
        s = np.concatenate([synth.converged_cloud(400, sc.pose + off, seed=5 + i, sigma=(0.15, 0.15, 0.05))
                            for i, off in enumerate([(0, 0, 0), (4.0, -2.0, 1.0), (-3.0, 3.5, -2.0)])])
    else:
        sc = Scenario(orc, size=400, n=4000 if base == "spread4000" else 5000, beams=61, cloud="spread")
        s = sc.samples.copy()
    s = np.ascontiguousarray(s)
    s[:, 3] = np.random.default_rng(9).uniform(0.5, 1.5, s.shape[0])
    s[:, 3] /= s[:, 3].sum()
    if name.endswith("_far"):
        s[s.shape[0] - 3, 0] = 5.0e6
    return orc, sc, s


def _read(sf):
    n, mean, cov = sf.compute_cluster_stats()
    cl = [sf.get_cluster(k) for k in range(n)]
    assert sf.get_cluster(n) is None
    bw, bp = sf.get_max_weight_pose()
    return dict(n=n, set_mean=np.array(mean), set_cov=np.array(cov), weight=np.array([c[0] for c in cl]),
                mean=np.array([c[1] for c in cl]).reshape(n, 3), count=np.array([c[2] for c in cl]),
                cov=np.array([c[3] for c in cl]).reshape(n, 5), best_w=bw, best_pose=np.array(bp),
                route=sf.stats_route)


def _worker(rank, world, port, out_dir, name, cuts, cycle):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from badger_amcl_amd.sharded import ShardedFilter
    from shard_stats_ref import StatsOracleShardBackend
    orc, sc, s = _set(name)
    n = s.shape[0]
    planar = sc.oracle_planar(61, "lf") if cycle else None
    b = StatsOracleShardBackend(orc, sc.omap if cycle else None, planar, s[cuts[rank]:cuts[rank + 1]], 100, n, seed=9)
    sf = ShardedFilter(b, dist, first_window=256)
    rec = dict(first=_read(sf), sums=b.int_sums, calls=list(b.stage_calls))
    # cached: a second round of queries makes no stage call
    again = _read(sf)
    assert b.stage_calls == rec["calls"]
    assert again["n"] == rec["first"]["n"] and np.array_equal(again["set_cov"], rec["first"]["set_cov"], equal_nan=True)
    if cycle:
        # every step of the filter invalidates; the statistics then describe the set the shards hold NOW
        steps = []
        sf.update_action(ODOM, ODATA)
        sf.update_sensor((sc.ranges, sc.angles, sc.range_max))
        before = len(b.stage_calls)
        steps.append(dict(stats=_read(sf), samples=b.samples.copy(), sums=b.int_sums))
        assert len(b.stage_calls) > before
        sf.update_resample()
        before = len(b.stage_calls)
        steps.append(dict(stats=_read(sf), samples=b.samples.copy(), sums=b.int_sums))
        assert len(b.stage_calls) > before
        rec["steps"] = steps
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([rec], dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()


def _run(tmp_path, name, cuts, cycle=False):
    W = len(cuts) - 1
    out = os.path.join(str(tmp_path), "%s_%d_%s" % (name, W, "_".join(str(c) for c in cuts)))
    while os.path.exists(out):
        out += "_again"
    os.makedirs(out)
    sys.path.insert(0, HERE)
    mp.spawn(_worker, args=(W, _free_port(), out, name, tuple(cuts), cycle), nprocs=W, join=True)
    return [np.load(os.path.join(out, "rank%d.npy" % r), allow_pickle=True)[0] for r in range(W)]


def _close(a, b, rtol=1e-12, atol=1e-12):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol,
                       equal_nan=True)


def _check_against_oracle(got, want, set_atol=1e-12):
    """The budgets of _assert_stats_equal(exact=False) in tests/test_gpu_next_rows.py: labels and counts exact, 1e-12
    relative for weights and means, 1e-10 absolute for covariances."""
    assert got["n"] == want["n"]
    assert np.array_equal(got["count"], want["count"])
    assert _close(got["set_mean"], want["set_mean"], atol=set_atol)
    assert _close(got["set_cov"], want["set_cov"], atol=max(1e-10, set_atol))
    assert _close(got["weight"], want["weight"]) and _close(got["mean"], want["mean"])
    assert _close(got["cov"], want["cov"], atol=1e-10)
    if want["n"]:
        k = int(np.argmax(want["weight"]))
        ws = np.sort(want["weight"])[::-1]
        assert ws.size < 2 or ws[0] - ws[1] > 1e-12 * ws[0], "the chosen set must not tie its two heaviest clusters"
        assert _close(got["best_w"], want["weight"][k]) and _close(got["best_pose"], want["mean"][k])


def _same(a, b):
    for k in ("n", "set_mean", "set_cov", "weight", "mean", "count", "cov", "best_w", "best_pose", "route"):
        if isinstance(a[k], str):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


_WORLD1 = {}


def _world1(tmp_path, name):
    if name not in _WORLD1:
        _, _, s = _set(name)
        _WORLD1[name] = _run(tmp_path, name, [0, s.shape[0]])[0]
    return _WORLD1[name]


def _even(n, W):
    return [(n * r) // W for r in range(W + 1)]


CASES = [("mixture", _even(1200, 1)), ("mixture", _even(1200, 2)), ("mixture", _even(1200, 3)),
         ("mixture", _even(1200, 8)), ("mixture", [0, 1, 2, 3, 500, 501, 900, 1199, 1200]),
         ("mixture", [0, 0, 700, 700, 1200]),                 # empty shards (ranks 0 and 2)
         ("blobs", [0, 200, 1200]), ("blobs", [0, 390, 410, 1200]), ("blobs", _even(1200, 8)),
         ("spread", _even(5000, 1)), ("spread", _even(5000, 2)), ("spread", [0, 17, 4000, 5000]),
         ("spread", _even(5000, 8)), ("spread", [0, 0, 2500, 2500, 5000])]


@pytest.mark.parametrize("name,cuts", CASES, ids=["%s-%s" % (n, "_".join(str(v) for v in c)) for n, c in CASES])
def test_sharded_statistics_equal_one_filter(tmp_path, name, cuts):
    recs = _run(tmp_path, name, cuts)
    orc, _, s = _set(name)
    for r in recs[1:]:
        _same(r["first"], recs[0]["first"])          # every rank returns the same values
        assert r["sums"] == recs[0]["sums"]
    one = _world1(tmp_path, name)
    assert recs[0]["sums"] == one["sums"]            # exact integers: any world, any split
    _same(recs[0]["first"], one["first"])
    # both regimes: the blobs (a few dozen bins) are evaluated from the gathered set, the 5 000 spread samples where
    # they are; the 1 200-sample mixture is small enough to be gathered but may hold too many bins or clusters for the
    # single-block form -- whichever way it goes, every rank of every world goes the same way
    distributed = ["local_bins", "label", "local_sums", "finish"]
    if name == "blobs":
        assert recs[0]["calls"] == ["gathered"] and recs[0]["first"]["route"] == "gathered"
    elif name == "spread":
        assert recs[0]["calls"] == distributed and recs[0]["first"]["route"] == "distributed"
    else:
        assert recs[0]["calls"] in (["gathered"], ["gathered"] + distributed)
    assert all(r["calls"] == recs[0]["calls"] for r in recs) and one["calls"] == recs[0]["calls"]
    if name == "blobs":
        assert recs[0]["first"]["n"] >= 3
    _check_against_oracle(recs[0]["first"], _oracle_stats(orc, s, s.shape[0]))


def test_a_small_set_with_too_many_bins_goes_distributed(tmp_path):
    """4 000 samples spread over more than 1 024 bins: the gathered form declines on every rank alike, the distributed
    form follows in the same query."""
    recs = _run(tmp_path, "spread4000", [0, 1500, 4000])
    assert all(r["calls"] == ["gathered", "local_bins", "label", "local_sums", "finish"] for r in recs)
    assert recs[0]["first"]["route"] == "distributed"
    _same(recs[0]["first"], recs[1]["first"])
    orc, _, s = _set("spread4000")
    _check_against_oracle(recs[0]["first"], _oracle_stats(orc, s, s.shape[0]))


@pytest.mark.parametrize("name,cuts", [("mixture_far", [0, 400, 800, 1200]), ("spread_far", [0, 2000, 3500, 5000])])
def test_a_key_outside_the_packing_on_one_rank_sends_every_rank_down_the_host_route(tmp_path, name, cuts):
    recs = _run(tmp_path, name, cuts)
    orc, _, s = _set(name)
    want = _oracle_stats(orc, s, s.shape[0])
    for r in recs:
        assert r["calls"][-1] == "host" and r["first"]["route"] == "host"
        assert "label" not in r["calls"] and "finish" not in r["calls"]
        got = r["first"]
        assert got["n"] == want["n"] and np.array_equal(got["count"], want["count"])
        for k in ("set_mean", "set_cov", "weight", "mean", "cov"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k   # the oracle's, bit for bit
        j = int(np.argmax(want["weight"]))
        assert got["best_w"] == want["weight"][j] and np.array_equal(got["best_pose"], want["mean"][j])


@pytest.mark.parametrize("cuts", [[0, 600, 1200], [0, 100, 650, 1200]])
def test_statistics_follow_the_filter_steps(tmp_path, cuts):
    """update_action -> update_sensor -> statistics -> update_resample -> statistics: each query after a step
    evaluates again and equals the oracle on the set the shards hold then."""
    recs = _run(tmp_path, "mixture", cuts, cycle=True)
    orc, _, _ = _set("mixture")
    for step in range(2):
        held = np.ascontiguousarray(np.concatenate([r["steps"][step]["samples"] for r in recs]))
        for r in recs[1:]:
            _same(r["steps"][step]["stats"], recs[0]["steps"][step]["stats"])
            assert r["steps"][step]["sums"] == recs[0]["steps"][step]["sums"]
        _check_against_oracle(recs[0]["steps"][step]["stats"], _oracle_stats(orc, held, held.shape[0]))
