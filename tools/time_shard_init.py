#!/usr/bin/env python3
"""Wall time of starting a filter: the single engine's bpf_pf_init_with_gaussian / bpf_pf_init_with_random_poses
(the yardstick), ShardedFilter.init_with_* with 1, 2 and 3 ranks that SHARE ONE GPU over the mailbox and over gloo,
and -- for the same sets, gloo -- the leaf count of the global set's tree by the two routes:

  bins   ShardedFilter._global_tree: the ranks' bin lists cross (16 B per occupied bin), merged on the device;
  keys   ShardedFilter._global_leaf_count, the only route before: three int64 per PARTICLE all-gathered to the CPU and
         inserted into the host tree one by one.

Sets: 100 000 samples from a Gaussian (converged: a handful of bins), 100 000 and 1 000 000 random free-space poses on
the 2000 x 2000 map (global localisation).  Ranks on one GPU bound the launch and host cost, NOT the exchange.
Host clock around a device synchronise; medians over --reps after --warmup untimed runs of every shape; the variants
alternate within one process.  Every sharded init is checked against the single engine's leaf / bin counts and rng
state before anything is timed.
Run on the GPU box: python tools/time_shard_init.py [--worlds 1,2,3] [--reps R] [--only NAME] [--out FILE]
[--single-only | --in-process EXCHANGE]; prints one JSON line.  --single-only uses nothing this tool's commit added, so
the same file times the single engine on an older checkout."""
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

SETS = {"gaussian_100k": 100_000, "random_100k": 100_000, "random_1m": 1_000_000}
MAP_SIZE = 2000
ROT = (0.8, -0.6, 0.0, 0.6, 0.8, 0.0, 0.0, 0.0, 1.0)
SIGMA = (0.15, 0.1, 0.05)


def setup_engine(e):
    """The bench-size map with the device-built distance LUT, and the free-space generator's radius."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    cells, origin = synth.make_map(MAP_SIZE, 0.05)
    m = bpf.OccupancyMap(e, 0.05)
    m.setCells(cells)
    m.setOrigin(origin)
    m.updateDistancesLUTExact(2.0)
    sc = bpf.PlanarScanner(e)
    sc.init(2, m)
    sc.setModelLikelihoodField(0.95, 0.05, 0.2, 2.0)
    sc.setMapFactors(*synth.MAP_FACTORS)
    return m, sc


def make_filter(e, n):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
    pf.srand48(17)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
    return pf


def run_init(name, gaussian, random):
    from badger_amcl_amd import synth
    if name.startswith("gaussian"):
        return gaussian(synth.true_pose(MAP_SIZE), ROT, SIGMA)
    return random()


def stats(ts):
    return dict(ms=statistics.median(ts) * 1e3, min_ms=min(ts) * 1e3)


def time_single(names, reps, warmup):
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    keep = setup_engine(e)
    out = {}
    for name in names:
        pf = make_filter(e, SETS[name])
        ts = []
        for rep in range(warmup + reps):
            pf.srand48(17)
            e.synchronize()
            t0 = time.perf_counter()
            run_init(name, pf.initWithGaussian, pf.initWithRandomPoses)
            e.synchronize()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts.append(dt)
        st = pf.getState()
        out[name] = dict(stats(ts), leaf=st.leaf_count, bins=st.bin_count, rng=pf.getRngState())
    del keep
    e.close()
    return out


def _worker(rank, world, port, names, reps, warmup, exchange, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    e, spare = bpf.Engine(0), bpf.Engine(0)
    keep = (setup_engine(e), setup_engine(spare))
    out = {}
    for name in names:
        n = SETS[name]
        pf, one = make_filter(e, n), make_filter(spare, n)
        sf = ShardedFilter(HipShardBackend(e, keep[0][1], pf, torch.device("cuda", 0)), dist, exchange=exchange,
                           init_follows=True)
        run_init(name, one.initWithGaussian, one.initWithRandomPoses)
        run_init(name, sf.init_with_gaussian, sf.init_with_random_poses)
        st = one.getState()
        assert (sf.leaf_count, sf.bin_count, pf.getRngState()) == (st.leaf_count, st.bin_count, one.getRngState()), name
        ts, tb, tk = [], [], []
        for rep in range(warmup + reps):
            pf.srand48(17)
            dist.barrier()
            e.synchronize()
            t0 = time.perf_counter()
            run_init(name, sf.init_with_gaussian, sf.init_with_random_poses)
            e.synchronize()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts.append(dt)
        rec = dict(init=stats(ts), route=sf.tree_route, leaf=sf.leaf_count, bins=sf.bin_count)
        if exchange == "collective":
            # the leaf count alone, both routes on the set just initialised, alternating
            want = (sf.leaf_count, sf.bin_count)
            for rep in range(warmup + reps):
                for route, acc in (("bins", tb), ("keys", tk)):
                    dist.barrier()
                    e.synchronize()
                    t0 = time.perf_counter()
                    if route == "bins":
                        got = sf._global_tree()
                    else:
                        sf.leaf_count = 0
                        sf._global_leaf_count()
                        got = (sf.leaf_count, sf.bin_count)
                    e.synchronize()
                    dt = time.perf_counter() - t0
                    assert got == want, (name, route, got, want)
                    if rep >= warmup:
                        acc.append(dt)
            rec.update(leaf_count_bins=stats(tb), leaf_count_keys=stats(tk))
        out[name] = rec
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()
    del keep
    spare.close()
    e.close()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="1,2,3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="one set: " + ", ".join(SETS))
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--in-process", default=None, metavar="EXCHANGE",
                    help="world size 1 in this very process, mailbox or collective (for a rocprofv3 --kernel-trace "
                         "--stats run, which follows the program it started and not the ranks it spawns)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = [k for k in SETS if not args.only or k == args.only]
    out = {"note": "ranks share one GPU: launch and host cost, not the exchange", "reps": args.reps,
           "warmup": args.warmup, "statistic": "median (and min) wall ms per call, host clock around a device synchronise"}
    if args.in_process:
        path = os.path.join("/tmp", "time_shard_init_%d_inline.json" % os.getpid())
        _worker(0, 1, _port(), names, args.reps, args.warmup, args.in_process, path)
        with open(path) as f:
            out["world_1_" + args.in_process] = json.load(f)
        os.remove(path)
    elif not args.single_only:
        import torch.multiprocessing as mp
        for world in [int(w) for w in args.worlds.split(",")]:
            for exchange in ("mailbox", "collective"):
                path = os.path.join("/tmp", "time_shard_init_%d_%d_%s.json" % (os.getpid(), world, exchange))
                mp.spawn(_worker, args=(world, _port(), names, args.reps, args.warmup, exchange, path), nprocs=world,
                         join=True)
                with open(path) as f:
                    out["world_%d_%s" % (world, exchange)] = json.load(f)
                os.remove(path)
    if not args.in_process:
        # twice: the spread between two identical runs is what "unchanged" can mean
        out["single"] = time_single(names, args.reps, args.warmup)
        out["single_again"] = time_single(names, args.reps, args.warmup)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
