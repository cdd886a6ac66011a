"""The in-place systematic resample through the one-call form from C++ (tests/cpp/shard_in_place.cpp):
LocalShardedParticleFilter at W = 8 on one device, forked ranks over the mailbox at W = 2 and 3, and W = 1 over RCCL
(BPF_BOOTSTRAP_FORCE_COLLECTIVE), each beside the unsharded filter.  The concatenation of the ranks' slices is the
unsharded set rotated by the model's i_wrap, bit for bit; windows_out is 0; the exchange count rises by EXCHANGES per
resample whatever M is: the (count, flag) words and the bin lists of the new tree, the limb words of the x / y sums,
the count of updateConverged."""
import os
import pathlib
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cpp_driver  # noqa: E402
import shard_in_place_ref as ipr  # noqa: E402

EXCHANGES = 4  # recorded: per in-place resample, on the mailbox, RCCL and the local exchange alike
MODE_MAILBOX, MODE_RCCL, MODE_LOCAL = 1, 2, 3
FORCE_COLLECTIVE = 1


def compile_driver(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_in_place")


def test_driver_compiles_and_links(tmp_path):
    from badger_amcl_amd import build
    build.build()
    assert compile_driver(tmp_path).exists()


def _fields(line):
    t = line.split()
    return {t[k]: int(t[k + 1]) for k in range(2 if t[0] == "rank" else 1, len(t) - 1, 2)}


def _run(tmp_path, orc, sc, mode, world, flags=0, cuts=None):
    n = sc.samples.shape[0]
    tree = orc.KDTree()
    for p in sc.samples[:, :3]:
        tree.insert_pose(p, 1.0)
    cfg, arrays = cpp_driver.planar_case(sc, min_samples=[100], max_samples=[n], seed=[21], kld=[0],
                                         leaf=[tree.leaf_count()], max_share=[float(world)])
    if cuts is not None:
        cfg["cuts"] = cuts
    d = pathlib.Path(tmp_path) / ("case_%d_%d_%d" % (mode, world, len(list(pathlib.Path(tmp_path).glob("case_*")))))
    cpp_driver.write_case(d, cfg, arrays)
    res = cpp_driver.run_driver(compile_driver(tmp_path), [d, mode, world, cpp_driver.free_port(), flags],
                                timeout=120)  # world + 1 <= 4 processes on the GPU
    assert res.returncode == 0, res.stdout + res.stderr
    if mode == 0:
        lines = res.stdout.splitlines()
        modes = [l for l in lines if l.startswith("mode ")]
        assert "next step ok form 1" in lines
    else:
        lines = cpp_driver.output_lines(d, world)
        modes = [l for l in lines if l.startswith("mode ")]
    ranks = [_fields(l) for l in lines if l.startswith("rank ")]
    single = _fields([l for l in lines if l.startswith("single ")][0])
    sets = [np.fromfile(str(d / ("rank%d.resample.bin" % r))).reshape(-1, 4) for r in range(world)]
    one = np.fromfile(str(d / "single.resample.bin")).reshape(-1, 4)
    return modes, ranks, single, sets, one


def _check(orc, world, ranks, single, sets, one):
    M = single["M"]
    assert one.shape == (M, 4) and len(ranks) == world
    _, i_wrap, _ = ipr.target_chain(single["rng0"], M)
    want = ipr.rotate(one, 0, i_wrap)
    got = np.concatenate(sets)
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    assert np.all(got[:, 3] == 1.0 / M)
    tree = orc.KDTree()
    for p in want[:, :3]:
        tree.insert_pose(p, 1.0)
    first = 0
    for r, f in enumerate(ranks):
        assert (f["M"], f["rng"], f["conv"], f["miss"]) == (M, single["rng"], single["conv"], 0), r
        assert f["windows"] == 0 and f["form"] == ipr.IN_PLACE, r
        assert (f["local"], f["first"]) == (sets[r].shape[0], first), r
        assert (f["leaf"], f["bins"]) == (f["eleaf"], f["ebins"]) == (tree.leaf_count(), tree.node_count()), r
        assert f["exch1"] - f["exch0"] == EXCHANGES, (r, f)
        first += f["local"]
    return M


@pytest.mark.gpu
def test_local_world_of_eight_in_place(tmp_path, orc):
    """W = 8 on one device, a converged cloud of 3 000 and a spread one of 800 (max_samples = the cloud's size, so the
    second M is at most 800): M differs by more than a factor of two, the exchange count per resample does not."""
    from scenario import Scenario
    Ms = []
    for cloud, n in (("converged", 3000), ("spread", 800)):
        sc = Scenario(orc, size=200, n=n, beams=60, cloud=cloud)
        modes, ranks, single, sets, one = _run(tmp_path, orc, sc, 0, 8)
        assert modes == ["mode %d" % MODE_LOCAL]
        Ms.append(_check(orc, 8, ranks, single, sets, one))
    assert Ms[0] > 2 * Ms[1], Ms


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags,mode,cuts", [(2, 0, MODE_MAILBOX, None), (3, 0, MODE_MAILBOX, [0, 1, 1250, 3000]),
                                                   (1, FORCE_COLLECTIVE, MODE_RCCL, None)])
def test_forked_ranks_in_place(tmp_path, orc, world, flags, mode, cuts):
    from scenario import Scenario
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged")
    modes, ranks, single, sets, one = _run(tmp_path, orc, sc, 1, world, flags, cuts)
    assert modes == ["mode %d" % mode] * world
    _check(orc, world, ranks, single, sets, one)
