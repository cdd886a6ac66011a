#!/usr/bin/env python3
"""Wall time of one bpf_shard_get_max_weight_pose (the global cluster statistics evaluated afresh, every exchange on the
engine's own transport) from the C++ driver tests/cpp/shard_node.cpp with ranks that SHARE ONE GPU, on the sets of
tools/time_shard_stats.py -- whose `--worlds W --only NAME` times ShardedFilter.get_max_weight_pose on the same set.
Ranks on one GPU bound the launch and host cost, NOT the exchange: nothing here says what xGMI does.
Run on the GPU box: python tools/time_shard_node_pose.py [--world 2] [--reps 30] [--warmup 5] [--only NAME]; prints one
JSON line (median / minimum ms per call, rank 0)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from time_shard_stats import SETS, make_set
    from badger_amcl_amd import build
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="one set: " + ", ".join(SETS))
    a = ap.parse_args()
    build.build()
    libdir = os.path.join(ROOT, "badger_amcl_amd")
    out = {"world": a.world, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "shard_node")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "shard_node.cpp"), "-o", exe, "-L", libdir,
                               "-lbadger_pf_hip", "-Wl,-rpath," + libdir])
        for name in ([a.only] if a.only else ["converged_2k", "spread_100k"]):
            s = make_set(name)
            d = os.path.join(tmp, name)
            os.mkdir(d)
            with open(os.path.join(d, "cfg.txt"), "w") as f:
                f.write("kind 2\nmin_samples 100\nmax_samples %d\nseed 42\ncycles 0\nstats 0\nstats_host 0\n"
                        "time_pose %d %d\n" % (s.shape[0], a.reps, a.warmup))
            np.ascontiguousarray(s).tofile(os.path.join(d, "samples.bin"))
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                port = so.getsockname()[1]
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
            flags = 2 if a.world > 1 else 1  # mailbox between the ranks of one GPU; RCCL at world size 1
            subprocess.run([exe, d, str(a.world), str(port), str(flags), "0"], check=True, env=env, timeout=600)
            line = [l for l in open(os.path.join(d, "rank0.txt")).read().splitlines() if " time_pose " in l][0].split()
            out[name] = {"median_ms": float(line[line.index("median_ms") + 1]),
                         "min_ms": float(line[line.index("min_ms") + 1])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
