"""The in-process sharded filter (bpf_shard_connect_local) as far as a box without a GPU can check it: the three entry
points are exported and bound, and the C++ driver of tests/test_gpu_cpp_local_world.py builds against the header
(badger_amcl_amd::LocalShardedParticleFilter) and links against the library."""
import os
import pathlib
import subprocess
import tempfile

import cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL_ABI = ("bpf_shard_connect_local", "bpf_shard_exchange_mode", "bpf_shard_local_selftest")


def compile_local_world(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "local_world")


def test_the_three_entry_points_are_exported_and_bound():
    from badger_amcl_amd import _lib, build
    so = build.build()
    syms = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
    for name in LOCAL_ABI:
        assert (" T " + name + "\n") in syms, name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in LOCAL_ABI:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "badger_pf.h")).read()
    assert "BPF_SHARD_EXCHANGE_LOCAL = 3" in header


def test_local_world_driver_compiles_and_links():
    from badger_amcl_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as d:
        assert compile_local_world(d).exists()


def test_local_sharded_filter_carries_the_sharded_filters_method_names():
    """Every public method of ShardedFilter that is not about its own transports (mailbox / torch.distributed)."""
    from badger_amcl_amd.local_world import LocalShardedFilter
    from badger_amcl_amd.sharded import ShardedFilter
    own_transport = {"use_collectives", "try_mailbox"}
    names = {n for n in vars(ShardedFilter) if not n.startswith("_") and callable(getattr(ShardedFilter, n))}
    missing = sorted(n for n in names - own_transport if not hasattr(LocalShardedFilter, n))
    assert missing == []
