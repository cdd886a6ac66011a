"""A sharded filter STARTED from plain C++ processes (tests/cpp/shard_init.cpp): bpf_shard_bootstrap, then
badger_amcl_amd::ShardedParticleFilter::initWithGaussian / initWithRandomPoses (the one-call forms: the init, the
exchange of the bin lists over the engine's own exchange, the global set's tree), updateAction, updateSensor,
updateResample and getMaxWeightPose -- against an unsharded ParticleFilter in the same program.  Worlds 2 and 3 over the
mailbox, world 1 over RCCL."""
import re
import subprocess

import numpy as np
import pytest

import cpp_driver
from scenario import Scenario

N = 6000


def _compile(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_init", "-Wall", "-Werror")


def test_shard_init_driver_compiles():
    """CPU: the driver builds against the adapter's new members and the library exports the new entry points."""
    import pathlib
    import tempfile
    from badger_amcl_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as d:
        _compile(pathlib.Path(d))
    syms = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
    for name in ("bpf_shard_init_with_gaussian", "bpf_shard_init_with_random_poses", "bpf_shard_init_with_gaussian_all",
                 "bpf_shard_init_with_random_poses_all", "bpf_shard_global_leaf_count", "bpf_shard_tree_local_bins_dev",
                 "bpf_shard_tree_merge_dev", "bpf_shard_tree_local_keys_dev", "bpf_shard_tree_from_keys",
                 "bpf_shard_tree_last_route"):
        assert re.search(r"\bT %s\b" % name, syms), name


def _parse(path):
    out = {}
    for line in open(path).read().splitlines():
        tag, rest = line.split(" ", 1)
        toks = rest.split()
        if tag in ("init", "resample"):
            out[tag] = dict(zip(toks[0::2], toks[1::2]))
        else:
            out[tag] = toks
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,resampler", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("world,flags", [(2, 2), (3, 2), (1, 1)])
def test_cpp_ranks_init_and_run_a_cycle(tmp_path, orc, world, flags, kind, resampler):
    """flags 2 = BPF_BOOTSTRAP_MAILBOX_ONLY, flags 1 = BPF_BOOTSTRAP_FORCE_COLLECTIVE (a real RCCL communicator at
    world size 1).  kind 0: Gaussian around the scenario's pose (a handful of bins); kind 1: random free-space poses."""
    exe = _compile(tmp_path)
    sc = Scenario(orc, size=400, n=256, beams=91)
    cpp_driver.write_case(tmp_path, None, dict(cells=sc.cells.astype(np.int32), lut=sc.lut.astype(np.float32),
                                               ranges=sc.ranges, angles=sc.angles,
                                               mean=np.asarray(sc.pose, dtype=np.float64)))
    res = cpp_driver.run_driver(exe, [tmp_path, world, cpp_driver.free_port(), flags, kind, N, resampler, "400"],
                                timeout=240)
    assert res.returncode == 0, res.stdout + res.stderr
    one = _parse(str(tmp_path / "single.txt"))
    ranks = [_parse(str(tmp_path / ("rank%d.txt" % r))) for r in range(world)]

    def sets(stage):
        parts = [np.fromfile(str(tmp_path / ("rank%d.%s.bin" % (r, stage))), dtype=np.float64).reshape(-1, 4)
                 for r in range(world)]
        return parts, np.fromfile(str(tmp_path / ("single.%s.bin" % stage)), dtype=np.float64).reshape(-1, 4)

    for r, got in enumerate(ranks):
        assert got["unconfigured"] == ["2", "2"]  # BPF_ERR_NOT_CONFIGURED before the bootstrap
        mode, _, x0, x1, x2, _, leaf2, bins2, _, route = got["mode"]
        assert int(mode) == (1 if flags == 2 else 2)
        # the init's exchanges: the bin counts with the flags, then the bin lists; none on the repeated query
        assert int(x1) - int(x0) == 2 and int(x2) == int(x1)
        assert route == "2"  # BPF_SHARD_TREE_ROUTE_HOST: fewer than 8 192 distinct keys
        ini = got["init"]
        assert (leaf2, bins2) == (ini["leaf"], ini["bins"])
        assert int(ini["first"]) == (N * r) // world and int(ini["global"]) == N
        assert int(ini["local"]) == (N * (r + 1)) // world - (N * r) // world
        for k in ("leaf", "bins", "rng", "conv", "wslow", "wfast"):
            assert ini[k] == one["init"][k], (r, k)
        assert (ini["eleaf"], ini["ebins"]) == (ini["leaf"], ini["bins"])
    assert (int(one["init"]["bins"]) < 200) if kind == 0 else (int(one["init"]["bins"]) > 1000)
    for stage in ("init", "moved"):
        parts, whole = sets(stage)
        assert whole.shape[0] == N and np.array_equal(np.concatenate(parts), whole), stage
    parts, whole = sets("resample")
    M = int(one["resample"]["global"])
    assert whole.shape[0] == M
    merged = np.concatenate(parts)
    assert np.array_equal(merged[:, :3], whole[:, :3]) and np.all(merged[:, 3] == 1.0 / M)
    for r, got in enumerate(ranks):
        res_ = got["resample"]
        for k in ("global", "leaf", "bins", "rng", "conv"):
            assert res_[k] == one["resample"][k], (r, k)
        assert int(res_["first"]) == (M * r) // world and int(res_["local"]) == (M * (r + 1)) // world - (M * r) // world
        # the pose of the heaviest cluster of the GLOBAL set: the bits of one engine holding the concatenation
        assert got["pose"] == one["pose"], (r, got["pose"], one["pose"])
