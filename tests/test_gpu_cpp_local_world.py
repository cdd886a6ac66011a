"""badger_amcl_amd::LocalShardedParticleFilter (include/badger_amcl_amd/adapter.hpp) at world size 8 beside the same
filter unsharded, in ONE program (tests/cpp/local_world.cpp): three cycles of motion, sensor, resample with the
comparisons of tests/test_gpu_cpp_shard_node.py::_check_cycles, and the global pose, cluster 0 and the particle cloud
bit for bit those of one engine holding the concatenation of the ranks' slices."""
import os

import pytest

import cpp_driver
from test_local_world_cpu import compile_local_world

W, CYCLES = 8, 3


@pytest.mark.gpu
def test_local_sharded_particle_filter_beside_an_unsharded_filter(tmp_path, orc):
    from scenario import Scenario
    from test_gpu_cpp_shard_node import _check_cycles, _planar_case
    # the scenario, seed and even split that tests/test_gpu_local_world.py took through the CPU backend at W = 8
    sc = Scenario(orc, size=200, n=3000, beams=60, cloud="converged")
    cfg, arrays = _planar_case(sc, max_samples=[3000], seed=[21], cycles=[CYCLES], world=[W], resampler=[0],
                               min_samples=[100])
    exe = compile_local_world(tmp_path)
    d = tmp_path / "case"
    cpp_driver.write_case(d, cfg, arrays)
    res = cpp_driver.run_driver(exe, [d], timeout=120, env=dict(os.environ))  # (one process: no IPC environment)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "before mode 0" and lines[1] == "local mode 3 world %d" % W and lines[-1] == "after mode 0"
    ranks = [[l for l in lines if l.startswith("rank %d " % r)] for r in range(W)]
    single = [l for l in lines if l.startswith("single ")]
    _check_cycles(ranks, single, str(d), W, CYCLES)
    poses = [l for l in lines if l.startswith("pose ")]
    assert len(poses) == 4 * CYCLES
    for a, b in zip(poses[0::2], poses[1::2]):
        ta, tb = a.split(), b.split()
        assert ta[:3] == tb[:3] and ta[3] == "local" and tb[3] == "concat"
        assert ta[4:] == tb[4:], (a, b)  # hex floats: the same bits
        assert ta[10] == "1"  # there is a cluster 0
    lazy = [l.split() for l in lines if l.startswith("lazy ")]
    assert len(lazy) == 2 * CYCLES
    for t in lazy:
        # the first query exchanged, the second did not; the strided particle cloud is the one engine's
        assert t[3:9] == ["first", "1", "second", "0", "cloud", "1"] and int(t[10]) > 0
