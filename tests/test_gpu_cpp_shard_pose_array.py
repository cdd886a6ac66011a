"""The particle cloud of a sharded filter from C / C++ (tests/cpp/shard_pose_array.cpp): bpf_shard_bootstrap, then
bpf_shard_get_pose_array -- through the C call and through badger_amcl_amd::ShardedParticleFilter::getPoseArray -- with
every exchange on the engine's own transport.  The ranks share the one GPU of the box; one more process holds the whole
set on one engine and calls bpf_pf_get_pose_array.  Every received array is that one, bit for bit."""
import subprocess

import numpy as np
import pytest

import cpp_driver

NEW_ABI = ("bpf_pf_get_pose_array", "bpf_shard_pose_rows_dev", "bpf_pose_array_from_rows_dev",
           "bpf_shard_get_pose_array")
WORLDS = [(2, 2), (3, 2), (1, 1)]  # (world, bootstrap flags): see test_gpu_cpp_shards.py for why these three
N = 3001
QUERIES = {"root0": (0, 0, 1), "all": (-1, 3, 7)}  # kQueries of the driver: (root, first, stride)


def _compile(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "shard_pose_array")


def test_driver_compiles_and_the_new_entry_points_are_exported():
    """CPU: the driver (C calls and both classes' getPoseArray) builds against the headers and links against the
    library, which exports the four new entry points."""
    import pathlib
    import tempfile
    from badger_amcl_amd import build
    so = build.build()
    with tempfile.TemporaryDirectory() as d:
        _compile(pathlib.Path(d))
    syms = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
    for name in NEW_ABI:
        assert (" T " + name + "\n") in syms, name


def _samples():
    rng = np.random.default_rng(77)
    s = np.zeros((N, 4))
    s[:, 0] = rng.normal(3.0, 0.4, N)
    s[:, 1] = rng.normal(-2.0, 0.4, N)
    s[:, 2] = rng.uniform(-4 * np.pi, 4 * np.pi, N)
    s[:8, 2] = [0.0, -0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 7.5, -9.0]
    s[:, 3] = rng.uniform(0.5, 1.5, N)
    s[:, 3] /= s[:, 3].sum()
    s[11, 0] = -0.0
    return s


def _fields(line, names):
    t = line.split()
    return {k: int(t[t.index(k) + 1]) for k in names}


@pytest.mark.gpu
@pytest.mark.parametrize("world,flags,cuts", [(w, f, None) for w, f in WORLDS] + [(3, 2, (0, 0, 1700, N))],
                         ids=["w2-mailbox", "w3-mailbox", "w1-rccl", "w3-mailbox-empty-shard"])
def test_pose_array_from_cpp(tmp_path, world, flags, cuts):
    exe = _compile(tmp_path)
    d = tmp_path / "case"
    s = _samples()
    cpp_driver.write_case(d, None, dict(samples=s))
    res = cpp_driver.run_driver(exe, [d, world, cpp_driver.free_port(), flags] + list(cuts or ()),
                                timeout=120)  # world + 1 <= 4 processes
    assert res.returncode == 0, res.stdout + res.stderr
    ranks = [[l for l in open(d / ("rank%d.txt" % r)).read().splitlines() if l.startswith("rank %d " % r)]
             for r in range(world)]
    want = {}
    for q, (root, first, stride) in QUERIES.items():
        want[q] = np.fromfile(str(d / ("single.%s.bin" % q)), dtype=np.uint64).reshape(-1, 7)
        assert want[q].shape[0] == len(range(first, N, stride))
        # the single engine's array is the selection of the set: x, y bit for bit, three +0.0
        assert np.array_equal(want[q][:, :2], np.ascontiguousarray(s[first::stride, :2]).view(np.uint64))
        assert not want[q][:, 2:5].any()
    for r in range(world):
        lines = ranks[r]
        assert lines[0] == "rank %d unconfigured 2" % r  # BPF_ERR_NOT_CONFIGURED before the bootstrap
        assert lines[1] == "rank %d mode %d" % (r, 1 if flags == 2 else 2)  # 1 = mailbox, 2 = RCCL
        for q, (root, first, stride) in QUERIES.items():
            for api in ("c", "a"):
                line = [l for l in lines if l.startswith("rank %d query %s api %s " % (r, q, api))]
                assert len(line) == 1
                receives = root < 0 or root == r
                f = _fields(line[0], ["count", "exch"])
                # the counts, then one gather of the rows; count_out is set on every rank (the class hands a
                # non-receiving rank an empty vector)
                assert f["exch"] == 2
                assert f["count"] == (want[q].shape[0] if receives or api == "c" else 0)
                path = d / ("rank%d.%s.%s.bin" % (r, api, q))
                assert path.exists() == receives
                if receives:
                    got = np.fromfile(str(path), dtype=np.uint64).reshape(-1, 7)
                    assert got.shape == want[q].shape and np.array_equal(got, want[q]), (r, q, api)
        lazy = [l for l in lines if l.startswith("rank %d lazy " % r)]
        assert len(lazy) == 1 and _fields(lazy[0], ["same", "query_exch", "pose_exch"]) == dict(
            same=1, query_exch=2, pose_exch=0)
        short = [l for l in lines if l.startswith("rank %d short " % r)]
        assert len(short) == 1 and _fields(short[0], ["rc", "count", "touched"]) == dict(
            rc=8 if r == 0 else 0, count=N, touched=0)  # BPF_ERR_CAPACITY on the receiving rank only
        assert [l for l in lines if l.startswith("rank %d refused " % r)] == \
            ["rank %d refused 1 1 1 empty 0 count 0 exch 1" % r]
