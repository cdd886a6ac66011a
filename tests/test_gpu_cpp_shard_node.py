"""A sharded filter as a C / C++ node runs it (tests/cpp/shard_node.cpp): bpf_shard_bootstrap, then nothing but one call
per step -- bpf_shard_update_sensor_planar (the prob model's beam skipping included), bpf_shard_update_sensor_cloud,
bpf_shard_update_resample, bpf_shard_compute_cluster_stats / bpf_shard_get_max_weight_pose -- with every exchange on
the engine's own transport.  The ranks share the one GPU of the box; one more process runs the filter unsharded.  One
half of the legs goes through the C calls, the other through badger_amcl_amd::ShardedParticleFilter (adapter.hpp).

A shard WITHOUT samples cannot take a sensor update (bpf_shard_score_planar refuses an empty set, as it always has), so
the split with an empty shard is queried as loaded; every other set is queried as loaded, after each sensor update
and after each resample."""
import os
import subprocess

import numpy as np
import pytest

import cpp_driver

NEW_ABI = ("bpf_shard_update_sensor_cloud", "bpf_shard_compute_cluster_stats", "bpf_shard_get_max_weight_pose",
           "bpf_shard_exchange_count")
WORLDS = [(2, 2), (3, 2), (1, 1)]  # (world, bootstrap flags): see test_gpu_cpp_shards.py for why these three
KEYS = ["n", "set_mean", "set_cov", "weight", "mean", "count", "cov", "best_w", "best_pose"]


def _compile(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_node")


def test_shard_node_compiles_and_the_new_entry_points_are_exported():
    """CPU: the driver (C calls and ShardedParticleFilter) builds against the header and links against the library;
    the one-call forms and the int64 all-gather of the RCCL object are exported."""
    import pathlib
    import tempfile
    from badger_amcl_amd import build
    so = build.build()
    with tempfile.TemporaryDirectory() as d:
        _compile(pathlib.Path(d))
    syms = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
    for name in NEW_ABI:
        assert (" T " + name + "\n") in syms, name
    syms = subprocess.run(["nm", "-D", build.OUT_RCCL], capture_output=True, text=True, check=True).stdout
    assert " T bpfc_allgather_i64\n" in syms


# ------------------------------------------------------------------------------------------------ running the program
def _planar_case(sc, model="lf", beamskip=None, **kw):
    return cpp_driver.planar_case(sc, kind=[0], model=[1 if model == "prob" else 0],
                                  beamskip=beamskip or [0, 0.5, 0.3, 0.9], **kw)


def _run(tmp_path, cfg, arrays, world, flags, api):
    """Runs the program; returns (per-rank lines, the unsharded process's lines, directory of the dumps)."""
    exe = _compile(tmp_path)
    d = tmp_path / "case"
    cfg = dict(dict(min_samples=[100], seed=[42], cycles=[2], stats=[0], stats_host=[0]), **cfg)
    cpp_driver.write_case(d, cfg, arrays)
    res = cpp_driver.run_driver(exe, [d, world, cpp_driver.free_port(), flags, api],
                                timeout=240)  # world + 1 <= 4 processes on the GPU
    assert res.returncode == 0, res.stdout + res.stderr
    # (only the program's own lines: RCCL prints a banner of its own into the same stream)
    ranks = [[l for l in open(d / ("rank%d.txt" % r)).read().splitlines() if l.startswith("rank %d " % r)]
             for r in range(world)]
    single = open(d / "single.txt").read().splitlines()
    for r in range(world):
        # before any exchange was set up the one-call forms return BPF_ERR_NOT_CONFIGURED
        assert ranks[r][0] == "rank %d unconfigured 2 2 2 2" % r
        assert ranks[r][1] == "rank %d mode %d" % (r, 1 if flags == 2 else 2)  # 1 = mailbox, 2 = RCCL
    return ranks, single, str(d)


def _fields(line, names):
    """'... key value ...' -> {key: int(value)} for the named keys"""
    t = line.split()
    return {k: int(t[t.index(k) + 1]) for k in names}


def _dump(d, who, cycle, step):
    return np.fromfile(os.path.join(d, "%s.c%d.%s.bin" % (who, cycle, step)), dtype=np.float64).reshape(-1, 4)


def _check_cycles(ranks, single, d, world, cycles, need_converged_from=None):
    """The comparisons of test_gpu_sharded.py / test_gpu_cpp_shards.py for every cycle: normalised weights at
    rtol 1e-12 (only the summation order of the total differs), M / leaf / bins / rng / converged equal on every rank and
    equal to the unsharded engine's, the resampled set equal up to ONE pose per cycle, every weight exactly 1 / M."""
    names = ["M", "leaf", "bins", "rng", "conv"]
    last_exch = [0] * world
    for c in range(cycles):
        one = [l for l in single if l.startswith("single cycle %d " % c)]
        assert len(one) == 1
        ref = _fields(one[0], names)
        if need_converged_from is not None and c >= need_converged_from:
            # the precondition of beam skipping: without it the compared update would be the plain prob model
            assert _fields(one[0], ["conv_before"])["conv_before"] == 1
        w_one = _dump(d, "single", c, "sensor")
        w_sh = np.concatenate([_dump(d, "rank%d" % r, c, "sensor") for r in range(world)])
        assert w_sh.shape == w_one.shape and np.array_equal(w_sh[:, :3], w_one[:, :3])
        assert np.allclose(w_sh[:, 3], w_one[:, 3], rtol=1e-12, atol=0)
        M = ref["M"]
        for r in range(world):
            got = [l for l in ranks[r] if l.startswith("rank %d cycle %d " % (r, c))]
            assert len(got) == 1
            f = _fields(got[0], names + ["local", "miss", "exch"])
            assert {k: f[k] for k in names} == ref, (r, c, f, ref)
            assert f["miss"] == 0 and f["local"] == (M * (r + 1)) // world - (M * r) // world
            assert f["exch"] > last_exch[r]  # every step exchanges
            last_exch[r] = f["exch"]
        new_one = _dump(d, "single", c, "resample")
        new_sh = np.concatenate([_dump(d, "rank%d" % r, c, "resample") for r in range(world)])
        assert new_sh.shape == new_one.shape == (M, 4)
        # (the shards' CDF slices are total_q / sum(totals): a draw within rounding of a slice edge may pick the
        # neighbouring particle -- one allowed per cycle, as in test_gpu_cpp_shards.py)
        assert np.flatnonzero(np.any(new_sh[:, :3] != new_one[:, :3], axis=1)).size <= 1
        assert np.all(new_sh[:, 3] == 1.0 / M)


# ------------------------------------------------------------------------------------------------ 1, 2: the updates
@pytest.mark.gpu
@pytest.mark.parametrize("world,flags", WORLDS)
def test_prob_model_with_beam_skipping_from_cpp(tmp_path, orc, world, flags):
    """test_gpu_sharded.py::test_two_ranks_prob_model_with_beam_skipping through ShardedParticleFilter: the first resample
    reports "converged", so the updates of cycles 1 and 2 run the counting pass, sum the counts over the engine's
    exchange and finish -- in mailbox mode too, where the mailbox form hands BPF_SHARD_NEED_BEAM_COUNTS back."""
    from scenario import Scenario
    from badger_amcl_amd import synth
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged", frac_max=0.0, frac_nan=0.0)
    sc.samples = synth.converged_cloud(3000, sc.pose, seed=12, sigma=(0.05, 0.05, 0.02))
    cfg, arrays = _planar_case(sc, model="prob", beamskip=[1, 0.5, 0.3, 0.9], max_samples=[3000], seed=[3], cycles=[3])
    ranks, single, d = _run(tmp_path, cfg, arrays, world, flags, api=1)
    _check_cycles(ranks, single, d, world, 3, need_converged_from=1)


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags", WORLDS)
def test_cloud3d_update_from_cpp(tmp_path, orc, world, flags):
    """test_gpu_sharded.py::test_two_ranks_cloud3d_equal_single_engine through the C calls: bpf_shard_update_sensor_cloud,
    and bpf_shard_update_resample accepts the totals it left."""
    from test_gpu_cloud import _setup
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, 3000, 8, 256, seed=6)
    cfg = dict(kind=[1], res=[0.05], max_dist=[max_dist], max_beams=[128], model_p=[0.5, 0.05, 0.1],
               map_factors=[0.95, 0.95, 0.3], tf_xyz=list(tf_xyz), tf_quat=list(tf_quat),
               min_cells=[int(v) for v in lut.min_cells], max_cells=[int(v) for v in lut.max_cells],
               max_samples=[3000], seed=[5], cycles=[2])
    arrays = dict(pose_indices=np.asarray(lut.pose_indices, dtype=np.uint32),
                  ratios=np.asarray(lut.distance_ratios, dtype=np.uint8), points=np.asarray(pts, dtype=np.float32),
                  samples=s)
    ranks, single, d = _run(tmp_path, cfg, arrays, world, flags, api=0)
    _check_cycles(ranks, single, d, world, 2)


# ------------------------------------------------------------------------------------------------ 3, 4: the global pose
def _parse_stats(line):
    t = line.split()
    assert t[2] == "stats" and t[5] == "route" and t[7] == "n" and t[9] == "mean" and t[13] == "cov" and t[19] == "best"
    n = int(t[8])
    fl = [float.fromhex(x) for x in t[10:13] + t[14:19] + t[20:24]]
    assert t[24] == "clusters" and len(t) == 25 + 10 * n
    cl = [t[25 + 10 * k: 35 + 10 * k] for k in range(n)]
    f = [[float.fromhex(x) for x in c[1:]] for c in cl]
    return dict(tag=(t[3], int(t[4])), route=int(t[6]), n=np.array([n]), set_mean=np.array(fl[0:3]),
                set_cov=np.array(fl[3:8]), best_w=np.array([fl[8]]), best_pose=np.array(fl[9:12]),
                count=np.array([int(c[0]) for c in cl]), weight=np.array([v[0] for v in f]),
                mean=np.array([v[1:4] for v in f]).reshape(n, 3), cov=np.array([v[4:9] for v in f]).reshape(n, 5))


def _expected_route(samples, clusters, host):
    """ShardedFilter._ensure_stats' choice, from the set alone: the host route on request; the gathered form up to
    4096 samples unless it declines (more than 1024 bins or 64 clusters, badger_pf.h); else the distributed form."""
    if host:
        return 3
    keys = np.stack([np.floor(samples[:, 0] / 0.5), np.floor(samples[:, 1] / 0.5),
                     np.floor(samples[:, 2] / (10 * np.pi / 180))], axis=1)
    bins = np.unique(keys, axis=0).shape[0]
    return 1 if samples.shape[0] <= 4096 and bins <= 1024 and clusters <= 64 else 2


def _expected_exchanges(route, n, clusters, world, flags, max_window):
    """Exchanges of one evaluation: the local counts; the slices when n <= 4096 (the gathered form is tried first);
    distributed: the bin counts with the flags, the bin lists, and the limb words (40 per cluster and rank) in rounds of
    6 * max_window / world words per rank over the mailbox, one all-reduce over RCCL; host: the slices."""
    tried_gathered = 1 if n <= 4096 else 0
    if route == 1:
        return 2
    if route == 3:
        return 3  # counts, then slices + slices (the gathered form asked for the host) or flags + slices
    per = (6 * max_window) // world
    rounds = 1 if flags == 1 else -(-40 * clusters // per)
    return 1 + tried_gathered + 2 + rounds


def _check_stats(ranks, d, world, orc, host, want_routes, flags, max_window):
    """Every stats line: the same on every rank; bit for bit ONE engine loaded with the concatenation of the dumped
    slices (weights included); the route the set calls for; the second query lazy; the number of exchanges of a query
    (counted where the count before it is printed: as loaded, and after a resample).  Returns the routes seen."""
    import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py
    import badger_amcl_amd as bpf
    from test_gpu_shard_stats import Recorded, assert_no_tie, assert_same_bits, reference_stats
    from test_gpu_next_rows import _assert_stats_equal, _oracle_stats
    lines = [[l for l in ranks[r] if l.split()[2] in ("stats", "lazy")] for r in range(world)]
    for r in range(1, world):
        assert [l.split(" ", 2)[2] for l in lines[r]] == [l.split(" ", 2)[2] for l in lines[0]], r
    e = bpf.Engine(0)
    seen, last_exch = [], -1
    try:
        it = iter(lines[0])
        for line in it:
            got = _parse_stats(line)
            step, cycle = got["tag"]
            whole = np.ascontiguousarray(np.concatenate(
                [np.fromfile(os.path.join(d, "rank%d.c%d.%s.bin" % (r, cycle, step)), dtype=np.float64).reshape(-1, 4)
                 for r in range(world)]))
            want = reference_stats(e, whole, host=host)
            assert_same_bits({k: got[k] for k in KEYS}, want, got["tag"])
            assert got["route"] == _expected_route(whole, int(want["n"][0]), host), got["tag"]
            seen.append(got["route"])
            if host:
                # the oracle's serial evaluation of the same concatenation: bit for bit on the loaded three-blob set
                # (the set test_host_route_equals_the_single_engine_and_the_oracle pins it with), within the
                # summation budgets of test_gpu_next_rows.py on the sets the filter makes of it (the engine's host
                # code and the oracle can differ in the last bit of a sin / cos, see that test's docstring)
                want_orc = _oracle_stats(orc, whole, whole.shape[0])
                assert_no_tie(want_orc)
                _assert_stats_equal(Recorded(got), want_orc, exact=(step == "loaded"))
            # the second query: the same bits, no exchange; and every new query exchanged again
            lazy = next(it).split()
            assert lazy[2:5] == ["lazy", step, str(cycle)] and lazy[5:7] == ["same", "1"]
            assert lazy[7] == "exch" and lazy[8] == lazy[9]
            assert int(lazy[8]) > last_exch
            last_exch = int(lazy[8])
            if step in ("loaded", "resample"):
                before = 0 if step == "loaded" else _fields(
                    [l for l in ranks[0] if l.startswith("rank 0 cycle %d " % cycle)][0], ["exch"])["exch"]
                assert last_exch - before == _expected_exchanges(got["route"], whole.shape[0], int(want["n"][0]), world,
                                                                 flags, max_window), got["tag"]
    finally:
        e.close()
    assert set(want_routes) <= set(seen), (want_routes, seen)
    return seen


def _stats_case(orc, name):
    """(scenario, cfg overrides, host route?, routes that must occur)"""
    from scenario import Scenario
    if name == "tracking":      # <= 4096 samples in one blob: the gathered form
        return Scenario(orc, size=400, n=2000, beams=91, cloud="converged"), {}, False, [1]
    if name == "large":         # more than 4096 samples: the distributed form (the resampled set is small again)
        return Scenario(orc, size=400, n=6000, beams=91, cloud="converged"), {}, False, [2]
    if name == "spread":        # <= 4096 samples in more than 1024 bins: the gathered form declines
        return Scenario(orc, size=400, n=4000, beams=91, cloud="spread"), {}, False, [2]
    if name == "host":          # BPF_OPT_STATS_HOST = 1 on every rank
        from test_gpu_shard_stats import three_blobs
        sc = Scenario(orc, size=400, n=3000, beams=91, cloud="converged")
        sc.samples = three_blobs(orc)
        return sc, dict(stats_host=[1]), True, [3]
    raise ValueError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags", WORLDS)
@pytest.mark.parametrize("name", ["tracking", "large", "spread", "host"])
def test_global_pose_from_cpp(tmp_path, orc, name, world, flags):
    """bpf_shard_compute_cluster_stats / bpf_shard_get_max_weight_pose on the set as loaded, after each sensor update
    and after each resample, two cycles."""
    sc, over, host, want_routes = _stats_case(orc, name)
    n = sc.samples.shape[0]
    cfg, arrays = _planar_case(sc, max_samples=[n], stats=[1], cycles=[2], **over)
    api = 1 if name in ("tracking", "spread") else 0
    ranks, single, d = _run(tmp_path, cfg, arrays, world, flags, api=api)
    _check_cycles(ranks, single, d, world, 2)
    seen = _check_stats(ranks, d, world, orc, host, want_routes, flags, n)
    assert len(seen) == 5  # loaded, 2 x (sensor, resample)


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags", [(2, 2), (3, 2)])
@pytest.mark.parametrize("n", [2000, 6000])
def test_global_pose_with_an_empty_shard(tmp_path, orc, n, world, flags):
    """One rank holds no samples (the first one; with three ranks the first and the last): the gathered form (2000)
    and the distributed form (6000) on the split as loaded, with its non-uniform weights.  (World size 1 has no second
    shard that could be the empty one, so the RCCL parametrisation is not among these.)"""
    from scenario import Scenario
    sc = Scenario(orc, size=400, n=n, beams=91, cloud="converged")
    cuts = [0, 0, n] if world == 2 else [0, 0, n, n]
    cfg, arrays = _planar_case(sc, max_samples=[n], stats=[1], cycles=[0], cuts=cuts)
    ranks, single, d = _run(tmp_path, cfg, arrays, world, flags, api=0)
    for r in range(world):
        got = np.fromfile(os.path.join(d, "rank%d.c0.loaded.bin" % r), dtype=np.float64)
        assert got.size == 4 * (cuts[r + 1] - cuts[r])
    seen = _check_stats(ranks, d, world, orc, False, [1 if n <= 4096 else 2], flags, n)
    assert len(seen) == 1
