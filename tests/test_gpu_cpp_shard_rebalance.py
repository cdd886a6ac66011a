"""Rebalancing the slices of a sharded filter through the one-call forms from C++ (tests/cpp/shard_rebalance.cpp):
LocalShardedParticleFilter at W = 8 on one device, forked ranks over the mailbox at W = 2 and 3, and W = 1 over RCCL
(BPF_BOOTSTRAP_FORCE_COLLECTIVE), each beside the unsharded filter.  Each run loads uneven slices, calls rebalance(),
then makes one sensor update and one in-place resample with BPF_SHARD_REBALANCE_AUTO at trigger_share = 1.  The
concatenation of the ranks' slices behind the rebalance is the unsharded program's loaded set, bit for bit, and behind
the resample its new set rotated by the model's i_wrap; the counts are the even split; the exchange count rises by 2
for a rebalance that moves samples (1 when none has to: W = 1) and by 5 for a resample that rebalances (4 when its
slices came out even: W = 1)."""
import os
import pathlib
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cpp_driver  # noqa: E402
import shard_in_place_ref as ipr  # noqa: E402
import shard_rebalance_ref as rbr  # noqa: E402

MODE_MAILBOX, MODE_RCCL, MODE_LOCAL = 1, 2, 3
FORCE_COLLECTIVE = 1
N = 3000
CUTS = {1: [0, N], 2: [0, 1, N], 3: [0, 1, 1250, N], 8: [0, 1, 2, 3, 1250, 1251, 2250, N - 1, N]}


def compile_driver(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_rebalance")


def test_driver_compiles_and_links(tmp_path):
    from badger_amcl_amd import build
    build.build()
    assert compile_driver(tmp_path).exists()


def _fields(line):
    t = line.split()
    return {t[k]: int(t[k + 1]) for k in range(1 if t[0] == "single" else 2, len(t) - 1, 2)}


def _run(tmp_path, orc, sc, mode, world, flags=0, window=None):
    n = sc.samples.shape[0]
    tree = orc.KDTree()
    for p in sc.samples[:, :3]:
        tree.insert_pose(p, 1.0)
    cfg, arrays = cpp_driver.planar_case(sc, min_samples=[100], max_samples=[n], seed=[21], kld=[0],
                                         leaf=[tree.leaf_count()], max_share=[2.0], cuts=CUTS[world])
    if window is not None:
        cfg["window"] = [window]
    d = pathlib.Path(tmp_path) / ("case_%d_%d" % (mode, world))
    cpp_driver.write_case(d, cfg, arrays)
    res = cpp_driver.run_driver(compile_driver(tmp_path), [d, mode, world, cpp_driver.free_port(), flags],
                                timeout=120)  # world + 1 <= 4 processes on the GPU
    assert res.returncode == 0, res.stdout + res.stderr
    if mode == 0:
        lines = res.stdout.splitlines()
        assert "next step ok form 1" in lines
    else:
        lines = cpp_driver.output_lines(d, world)
    if window is not None:
        return lines, d
    modes = [l for l in lines if l.startswith("mode ")]
    rebal = [_fields(l) for l in lines if l.startswith("rebalance ")]
    ranks = [_fields(l) for l in lines if l.startswith("rank ")]
    single = _fields([l for l in lines if l.startswith("single ")][0])

    def sets(tag):
        return [np.fromfile(str(d / ("rank%d.%s.bin" % (r, tag)))).reshape(-1, 4) for r in range(world)]
    loaded = np.fromfile(str(d / "single.loaded.bin")).reshape(-1, 4)
    one = np.fromfile(str(d / "single.resample.bin")).reshape(-1, 4)
    return modes, rebal, ranks, single, sets("rebalance"), sets("resample"), loaded, one


def _even(n, W):
    return [(n * (r + 1)) // W - (n * r) // W for r in range(W)]


def _check(orc, world, rebal, ranks, single, held, sets, loaded, one):
    # the stand-alone rebalance of the uneven load
    cuts = CUTS[world]
    T = rbr.plan([cuts[r + 1] - cuts[r] for r in range(world)])["moved"]
    assert (T > 0) == (world > 1) and len(rebal) == len(ranks) == world
    got = np.concatenate(held)
    assert loaded.shape == (N, 4) and got.shape == loaded.shape
    assert np.array_equal(got.view(np.uint64), loaded.view(np.uint64))
    assert [s.shape[0] for s in held] == _even(N, world)
    for r, f in enumerate(rebal):
        assert (f["moved"], f["local"], f["first"]) == (T, _even(N, world)[r], (N * r) // world), (r, f)
        assert f["exch1"] - f["exch0"] == (2 if T else 1), (r, f)
        assert (f["leaf"], f["bins"]) == (rebal[0]["leaf"], rebal[0]["bins"]) and f["leaf"] > 0, (r, f)
    # the resample with AUTO behind it
    M = single["M"]
    assert one.shape == (M, 4)
    _, i_wrap, _ = ipr.target_chain(single["rng0"], M)
    want = ipr.rotate(one, 0, i_wrap)
    got = np.concatenate(sets)
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    assert np.all(got[:, 3] == 1.0 / M)
    assert [s.shape[0] for s in sets] == _even(M, world)
    tree = orc.KDTree()
    for p in want[:, :3]:
        tree.insert_pose(p, 1.0)
    moved = ranks[0]["moved"]
    assert (moved > 0) == (world > 1)
    for r, f in enumerate(ranks):
        assert (f["M"], f["rng"], f["conv"], f["miss"]) == (M, single["rng"], single["conv"], 0), r
        assert f["windows"] == 0 and f["form"] == ipr.IN_PLACE and f["moved"] == moved, r
        assert (f["local"], f["first"]) == (sets[r].shape[0], (M * r) // world), r
        assert (f["leaf"], f["bins"]) == (f["eleaf"], f["ebins"]) == (tree.leaf_count(), tree.node_count()), r
        assert f["exch1"] - f["exch0"] == (5 if moved else 4), (r, f)


@pytest.mark.gpu
def test_local_world_of_eight_rebalances(tmp_path, orc):
    from scenario import Scenario
    sc = Scenario(orc, size=200, n=N, beams=60, cloud="converged")
    modes, *rest = _run(tmp_path, orc, sc, 0, 8)
    assert modes == ["mode %d" % MODE_LOCAL]
    _check(orc, 8, *rest)


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags,mode", [(2, 0, MODE_MAILBOX), (3, 0, MODE_MAILBOX),
                                              (1, FORCE_COLLECTIVE, MODE_RCCL)])
def test_forked_ranks_rebalance(tmp_path, orc, world, flags, mode):
    from scenario import Scenario
    sc = Scenario(orc, size=200, n=N, beams=60, cloud="converged")
    modes, *rest = _run(tmp_path, orc, sc, 1, world, flags)
    assert modes == ["mode %d" % mode] * world
    _check(orc, world, *rest)


@pytest.mark.gpu
def test_a_refused_rebalance_leaves_a_valid_set(tmp_path, orc):
    """Two forked ranks over a mailbox whose windows (256 columns, 1 536 words) are too small for the moved rows.  The
    stand-alone rebalance answers BPF_ERR_CAPACITY with the old, uneven slices current and nothing reported as moved.
    The AUTO resample commits its in-place resample and then fails in the rebalance behind it: the error comes back,
    bpf_shard_resample_committed says 1, the adapter's figures follow the new set, and the slices concatenate to the
    unsharded program's new set rotated -- resampled once, uneven, valid."""
    from scenario import Scenario
    CAPACITY, world = 8, 2
    sc = Scenario(orc, size=200, n=N, beams=60, cloud="converged")
    lines, d = _run(tmp_path, orc, sc, 1, world, window=256)
    assert [l for l in lines if l.startswith("mode ")] == ["mode %d" % MODE_MAILBOX] * world
    single = _fields([l for l in lines if l.startswith("single ")][0])
    loaded = np.fromfile(str(d / "single.loaded.bin")).reshape(-1, 4)
    one = np.fromfile(str(d / "single.resample.bin")).reshape(-1, 4)
    cuts = CUTS[world]
    held = [np.fromfile(str(d / ("rank%d.rebalance.bin" % r))).reshape(-1, 4) for r in range(world)]
    first = [_fields(l) for l in lines if l.startswith("norebalance ")]
    assert len(first) == world
    for r, f in enumerate(first):
        assert (f["threw"], f["status"], f["last"], f["moved"]) == (1, CAPACITY, 0, 0), (r, f)
        assert f["local"] == cuts[r + 1] - cuts[r] == held[r].shape[0], (r, f)
    assert np.array_equal(np.concatenate(held).view(np.uint64), loaded.view(np.uint64))
    M = single["M"]
    _, i_wrap, _ = ipr.target_chain(single["rng0"], M)
    want = ipr.rotate(one, 0, i_wrap)
    sets = [np.fromfile(str(d / ("rank%d.resample.bin" % r))).reshape(-1, 4) for r in range(world)]
    got = np.concatenate(sets)
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3]) and np.all(got[:, 3] == 1.0 / M)
    counts = [s.shape[0] for s in sets]
    assert 4 * rbr.plan(counts)["moved"] > 6 * 256  # what the mailbox refuses
    at = 0
    for r, f in enumerate([_fields(l) for l in lines if l.startswith("noauto ")]):
        assert (f["threw"], f["status"], f["committed"], f["last"], f["moved"]) == (1, CAPACITY, 1, 0, 0), (r, f)
        assert (f["local"], f["first"], f["M"], f["form"]) == (counts[r], at, M, ipr.IN_PLACE), (r, f)
        assert f["rng"] == single["rng"], (r, f)  # one resample's worth of the stream
        at += counts[r]
