"""The in-place multinomial resample through the one-call form from C++ (tests/cpp/shard_in_place_mn.cpp, the
adapter's setMultinomialForm): LocalShardedParticleFilter at W = 2 on one device and two forked ranks over the mailbox,
each beside the unsharded filter: one sensor update, one resample.  The concatenation of the ranks' slices is the
unsharded set sorted stably by the rank that holds each sample's source particle (the cloud's poses are pairwise
distinct, so a pose names its source), bit for bit; windows_out is 0; the exchange count rises by EXCHANGES."""
import os
import pathlib
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cpp_driver  # noqa: E402
import shard_in_place_mn_ref as mnr  # noqa: E402

EXCHANGES = 4  # the (count, flag) words, the bin lists, the limb words of the x / y sums, the count of updateConverged
MODE_MAILBOX, MODE_LOCAL = 1, 3


def compile_driver(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_in_place_mn")


def test_driver_compiles_and_links(tmp_path):
    from badger_amcl_amd import build
    build.build()
    assert compile_driver(tmp_path).exists()


def _fields(line):
    t = line.split()
    return {t[k]: int(t[k + 1]) for k in range(2 if t[0] == "rank" else 1, len(t) - 1, 2)}


def _run(tmp_path, sc, mode, world):
    n = sc.samples.shape[0]
    cfg, arrays = cpp_driver.planar_case(sc, min_samples=[100], max_samples=[n], seed=[21], kld=[0], leaf=[0],
                                         max_share=[float(world)])
    d = pathlib.Path(tmp_path) / ("case_%d_%d" % (mode, world))
    cpp_driver.write_case(d, cfg, arrays)
    res = cpp_driver.run_driver(compile_driver(tmp_path), [d, mode, world, cpp_driver.free_port(), 0],
                                timeout=120)  # world + 1 <= 3 processes on the GPU
    assert res.returncode == 0, res.stdout + res.stderr
    if mode == 0:
        lines = res.stdout.splitlines()
        assert "next step ok form 1" in lines
    else:
        lines = cpp_driver.output_lines(d, world)
    modes = [l for l in lines if l.startswith("mode ")]
    ranks = [_fields(l) for l in lines if l.startswith("rank ")]
    single = _fields([l for l in lines if l.startswith("single ")][0])
    sets = [np.fromfile(str(d / ("rank%d.resample.bin" % r))).reshape(-1, 4) for r in range(world)]
    one = np.fromfile(str(d / "single.resample.bin")).reshape(-1, 4)
    return modes, ranks, single, sets, one


def _check(orc, sc, world, ranks, single, sets, one):
    M, n = single["M"], sc.samples.shape[0]
    assert one.shape == (M, 4) and len(ranks) == world and M < n  # (the converged cloud stops early)
    assert len(set(map(tuple, sc.samples[:, :3]))) == n  # a pose names its source
    where = {tuple(p): i for i, p in enumerate(sc.samples[:, :3])}
    cuts = [(n * r) // world for r in range(world + 1)]
    owner = np.array(mnr.owner_of_sources([where[tuple(p)] for p in one[:, :3]], cuts))
    want = one[np.argsort(owner, kind="stable")]
    got = np.concatenate(sets)
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    assert np.all(got[:, 3] == 1.0 / M)
    first = 0
    for r, f in enumerate(ranks):
        assert (f["M"], f["rng"], f["conv"], f["miss"]) == (M, single["rng"], single["conv"], 0), r
        assert f["windows"] == 0 and f["form"] == mnr.IN_PLACE, r
        assert (f["local"], f["first"]) == (int(np.sum(owner == r)), first), r
        assert (f["leaf"], f["bins"]) == (f["eleaf"], f["ebins"]) == (single["leaf"], single["bins"]), r
        assert f["exch1"] - f["exch0"] == EXCHANGES, (r, f)
        first += f["local"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,expect", [(0, MODE_LOCAL), (1, MODE_MAILBOX)])
def test_two_ranks_one_resample(tmp_path, orc, mode, expect):
    from scenario import Scenario
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged")
    modes, ranks, single, sets, one = _run(tmp_path, sc, mode, 2)
    assert modes == ["mode %d" % expect] * (1 if mode == 0 else 2)
    _check(orc, sc, 2, ranks, single, sets, one)
