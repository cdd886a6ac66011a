"""The rebalance plan of a sharded set with no GPU: the Python restatement (shard_rebalance_ref.py) against a brute-force
enumeration of every global index, the numpy emulation of pack and assemble (the concatenation is unchanged, the new
counts are the even split), and the engine's own header (badger_amcl_amd/csrc/shard_rebalance_plan.hpp) compiled into a
stand-alone program under the address and undefined-behaviour sanitizers, run as a plain executable."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import shard_rebalance_ref as rbr  # noqa: E402

NAMED = [
    [1, 1, 1, 497, 1, 399, 299, 1],       # a rank that keeps nothing, and a new slice with four owners
    [1, 1198, 1],                         # head AND tail outgoing
    [0, 1200, 0],
    [0, 0, 2, 298, 0, 300, 1, 598, 1],
    [1200],
    [150] * 8,                            # nothing moves
    [5, 0, 0, 0, 0, 0, 0, 0],             # fewer samples than ranks
    [0, 0, 0, 0, 0, 0, 0, 3],
]


def random_vectors(n, seed=5):
    rng = np.random.default_rng(seed)
    for k in range(n):
        W = 1 + k % 16
        c = rng.integers(0, 8 if k % 3 == 0 else 120, W)
        if k % 3 == 2:
            c[rng.random(W) < 0.35] = 0
        yield [int(v) for v in c]


def check_vector(counts):
    pl = rbr.plan(counts)
    W, G = len(counts), sum(counts)
    out, srcs, out_lists = rbr.brute_force(counts)
    assert pl["out"] == out and pl["moved"] == sum(out), counts
    assert [pl["Q"][r + 1] - pl["Q"][r] for r in range(W)] == rbr.even_split(G, W), counts
    for r in range(W):
        got = [rbr.source(pl, r, g) for g in range(pl["Q"][r], pl["Q"][r + 1])]
        assert got == srcs[r], (counts, r)
        # the pack order: head span, then tail span, in ascending global index
        head, kn = pl["keep_lo"][r] - pl["P"][r], pl["keep_n"][r]
        assert [pl["P"][r] + (i if i < head else i + kn) for i in range(pl["out"][r])] == out_lists[r], (counts, r)
    # pack and assemble on values that tell every sample and every field apart
    whole = np.arange(4 * G, dtype=np.float64).reshape(G, 4) + 0.25
    slices = [whole[pl["P"][r]:pl["P"][r + 1]] for r in range(W)]
    new, pl2 = rbr.rebalance(slices)
    assert pl2 == pl
    assert [s.shape[0] for s in new] == rbr.even_split(G, W), counts
    assert np.array_equal(np.concatenate(new) if G else np.zeros((0, 4)), whole), counts
    return pl


@pytest.mark.parametrize("counts", NAMED, ids=[",".join(map(str, c)) for c in NAMED])
def test_named_vectors_against_enumeration(counts):
    check_vector(counts)


def test_what_the_named_vectors_are_there_for():
    pl = rbr.plan(NAMED[0])
    assert 0 in [pl["keep_n"][r] for r in range(8) if NAMED[0][r] > 0]
    owners = [{rbr.owner(pl, g) for g in range(pl["Q"][r], pl["Q"][r + 1])} for r in range(8)]
    assert max(len(f) for f in owners) >= 4  # rank 0's new slice: its own sample and those of three other ranks
    pl = rbr.plan(NAMED[1])
    head, tail = pl["keep_lo"][1] - pl["P"][1], pl["P"][2] - pl["keep_lo"][1] - pl["keep_n"][1]
    assert head > 0 and tail > 0 and head + tail == pl["out"][1]
    assert rbr.plan(NAMED[5])["moved"] == 0 and rbr.plan(NAMED[4])["moved"] == 0
    assert rbr.plan([1, 69999])["moved"] == 34999


def test_random_vectors_against_enumeration():
    n = 0
    for counts in random_vectors(3000):
        check_vector(counts)
        n += 1
    assert n == 3000


def test_the_plan_refuses_bad_counts():
    with pytest.raises(ValueError):
        rbr.plan([1] * 17)
    with pytest.raises(ValueError):
        rbr.plan([3, -1])


def test_engine_header_under_sanitizers(tmp_path):
    """shard_rebalance_plan.hpp has no HIP include: a host program of its own compiles it, runs the same vectors
    against its own enumeration, and the sanitizers watch: their runtimes are linked in statically, the program inherits the
    environment as it is, nothing is preloaded by the test and nothing is loaded into python."""
    exe = tmp_path / "shard_rebalance_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "badger_amcl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "shard_rebalance_plan.cpp"), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout, res.stdout


def test_the_binding_declares_the_rebalance_calls():
    from badger_amcl_amd import _lib
    for name in ("bpf_shard_set_rebalance", "bpf_shard_get_rebalance", "bpf_shard_rebalance", "bpf_shard_rebalance_plan",
                 "bpf_shard_rebalance_export_dev", "bpf_shard_rebalance_import_dev", "bpf_shard_rebalance_last"):
        assert name in _lib.SIGNATURES
