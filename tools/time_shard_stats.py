#!/usr/bin/env python3
"""Wall time of one ShardedFilter.get_max_weight_pose (the global cluster statistics, evaluated afresh) with 1, 2 and
3 ranks that SHARE ONE GPU (gloo, exchanges staged through the host), for a 2 000-sample converged set (the gathered
form), and 100 000 and 1 000 000 spread samples (the distributed form), beside

  single   bpf_pf_get_max_weight_pose of ONE engine holding the whole set (evaluated afresh each rep);
  gather   the only route a sharded caller had before: every rank's bpf_pf_get_samples, concatenation over the
           process group, bpf_pf_set_samples into a spare engine on rank 0, bpf_pf_get_max_weight_pose there.

Ranks on one GPU bound the launch and host cost of the stages, NOT the exchange: nothing here says what xGMI does.
Medians over --reps timed repetitions after --warmup untimed ones; the weights are random (no map is needed), the
statistics are checked against the single engine's before anything is timed.
Run on the GPU box: python tools/time_shard_stats.py [--worlds 1,2,3] [--reps R] [--only NAME] [--out FILE]
[--single-only | --in-process]; prints one JSON line.  --single-only uses nothing this tool's commit added, so the
same file times the single engine on an older checkout."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"converged_2k": 2000, "spread_100k": 100_000, "spread_1m": 1_000_000}


def make_set(name):
    from badger_amcl_amd import synth
    n = SETS[name]
    if name.startswith("converged"):
        s = synth.converged_cloud(n, synth.true_pose(2000))
    else:
        s = synth.spread_cloud(n, 2000, seed=43, margin=0.5)
    s = np.ascontiguousarray(s, dtype=np.float64)
    s[:, 3] = np.random.default_rng(7).uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    return s


def median_ms(ts):
    return statistics.median(ts) * 1e3


def time_single(names, reps, warmup):
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    out = {}
    for name in names:
        s = make_set(name)
        pf = bpf.ParticleFilter(e, 100, s.shape[0], 0.0, 0.0, 85.0)
        pf.initWithSamples(s)
        pf.snapshot()
        ts = []
        for rep in range(warmup + reps):
            pf.restore()  # same set, statistics cache dropped
            e.synchronize()
            t0 = time.perf_counter()
            w, pose = pf.getMaxWeightPose()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts.append(dt)
        out[name] = dict(ms=median_ms(ts), min_ms=min(ts) * 1e3, clusters=pf.computeClusterStats()[0], weight=w)
    e.close()
    return out


def _worker(rank, world, port, names, reps, warmup, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    e = bpf.Engine(0)
    spare = bpf.Engine(0)
    out = {}
    for name in names:
        s = make_set(name)
        n = s.shape[0]
        lo, hi = (n * rank) // world, (n * (rank + 1)) // world
        pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
        pf.initWithSamples(np.ascontiguousarray(s[lo:hi]))
        sf = ShardedFilter(HipShardBackend(e, None, pf, torch.device("cuda", 0)), dist, exchange="collective")
        spare_pf = bpf.ParticleFilter(spare, 100, n, 0.0, 0.0, 85.0)
        spare_pf.initWithSamples(s)
        want = spare_pf.getMaxWeightPose()
        got = sf.get_max_weight_pose()
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (name, got, want)
        ts, tg = [], []
        for rep in range(warmup + reps):
            sf.restore(sf.counts, sf.leaf_count)  # drops the cache; the set stays
            dist.barrier()
            t0 = time.perf_counter()
            sf.get_max_weight_pose()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts.append(dt)
        for rep in range(warmup + reps):
            dist.barrier()
            t0 = time.perf_counter()
            mine = torch.from_numpy(pf.getCurrentSet().samples)
            pad = torch.zeros((max(sf.counts), 4), dtype=torch.float64)
            pad[:mine.shape[0]] = mine
            parts = [torch.empty_like(pad) for _ in range(world)]
            dist.all_gather(parts, pad)
            if rank == 0:
                whole = np.ascontiguousarray(torch.cat([p[:c] for p, c in zip(parts, sf.counts)]).numpy())
                spare_pf.initWithSamples(whole)
                spare_pf.getMaxWeightPose()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                tg.append(dt)
        out[name] = dict(sharded_ms=median_ms(ts), sharded_min_ms=min(ts) * 1e3, gather_ms=median_ms(tg),
                         gather_min_ms=min(tg) * 1e3, route=sf.stats_route)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()
    spare.close()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="1,2,3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="one set: " + ", ".join(SETS))
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--in-process", action="store_true",
                    help="world size 1 in this very process (for a rocprofv3 --kernel-trace --stats run, which follows "
                         "the program it started and not the ranks it spawns); the single engine is not timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = [k for k in SETS if not args.only or k == args.only]
    out = {"note": "ranks share one GPU: launch and host cost of the stages, not the exchange", "reps": args.reps,
           "warmup": args.warmup, "statistic": "median (and min) wall ms per call"}
    if args.in_process:
        path = os.path.join("/tmp", "time_shard_stats_%d_inline.json" % os.getpid())
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        _worker(0, 1, port, names, args.reps, args.warmup, path)
        with open(path) as f:
            out["world_1"] = json.load(f)
        os.remove(path)
    elif not args.single_only:
        import torch.multiprocessing as mp
        for world in [int(w) for w in args.worlds.split(",")]:
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            path = os.path.join("/tmp", "time_shard_stats_%d_%d.json" % (os.getpid(), world))
            mp.spawn(_worker, args=(world, port, names, args.reps, args.warmup, path), nprocs=world, join=True)
            with open(path) as f:
                out["world_%d" % world] = json.load(f)
            os.remove(path)
    if not args.in_process:
        out["single"] = time_single(names, args.reps, args.warmup)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
