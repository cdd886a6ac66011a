#!/usr/bin/env python3
"""The particle-cloud message (Node::publishParticleCloud, node.cpp:335-357): wall time of one call that leaves the
PoseArray entries in host memory, and how far the device's sin / cos are from the host's.

  accuracy  largest |difference| of the quaternion columns between bpf_pf_get_pose_array and
            bpf_wire_samples_to_pose_array (host libm) over the edge headings 0, -0, +-pi, +-pi/2, 7.5, -9 and
            1 000 000 random headings in [-4 pi, 4 pi]: max_abs_dev_vs_host_libm (the bound of
            tests/test_gpu_pose_array.py is twice this figure)
  single    8 000, 100 000 and 1 000 000 particles on one engine, pageable and registered output:
              parent   bpf_pf_get_samples + bpf_wire_samples_to_pose_array, both calls timed together (the route a
                       caller had before; entry points this change leaves untouched, timed in the same session)
              new      bpf_pf_get_pose_array at stride 1
              new_100  bpf_pf_get_pose_array at stride 100
  sharded   ShardedFilter.get_pose_array(root=0) of 100 000 particles with 1, 2 and 3 ranks that SHARE ONE GPU, over
            the mailbox (the engine's one-call form) and over gloo: this bounds launch and host cost only and says
            nothing about xGMI.

Every timed call ends with the data in host memory (the calls synchronise).  Per figure: --warmup untimed calls of
the same shape, then the median (and the minimum) of --reps.  Run on the GPU box:
python tools/time_pose_array.py [--reps 30] [--warmup 5] [--worlds 1,2,3] [--out profiles/pose_array.json]"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [8000, 100000, 1000000]
EDGE_HEADINGS = [0.0, -0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 7.5, -9.0]
N_SHARDED = 100000
DP = C.POINTER(C.c_double)


def make_set(n, seed=5):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    s[:, 0] = rng.uniform(-50, 50, n)
    s[:, 1] = rng.uniform(-50, 50, n)
    s[:, 2] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    s[:, 3] = 1.0 / n
    return s


def timed(fn, reps, warmup):
    ts = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if rep >= warmup:
            ts.append(dt)
    return dict(ms=statistics.median(ts) * 1e3, min_ms=min(ts) * 1e3)


def accuracy(e):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import wire
    s = make_set(1000000 + len(EDGE_HEADINGS), seed=11)
    s[:len(EDGE_HEADINGS), 2] = EDGE_HEADINGS
    pf = bpf.ParticleFilter(e, 1, s.shape[0], 0.0, 0.0, 85.0)
    pf.initWithSamples(s)
    got = pf.getPoseArray()
    want = wire.samples_to_pose_array(pf.getCurrentSet().samples)
    assert np.array_equal(got[:, :5].copy().view(np.uint64), want[:, :5].copy().view(np.uint64))
    dev = np.abs(got[:, 5:] - want[:, 5:])
    return dict(max_abs_dev_vs_host_libm=float(dev.max()), headings=int(s.shape[0]),
                differing_values=int(np.count_nonzero(dev)), ulp_of_one=float(np.finfo(np.float64).eps))


def single(e, reps, warmup):
    import badger_amcl_amd as bpf
    lib = e.lib
    out = {}
    for n in SIZES:
        pf = bpf.ParticleFilter(e, 1, n, 0.0, 0.0, 85.0)
        pf.initWithSamples(make_set(n))
        rec = {}
        for kind in ("pageable", "registered"):
            samples, poses = np.zeros((n, 4)), np.zeros((n, 7))
            if kind == "registered":
                e.registerHostBuffer(samples)
                e.registerHostBuffer(poses)
            cnt = C.c_int()
            sp, pp = samples.ctypes.data_as(DP), poses.ctypes.data_as(DP)

            def parent():
                e.check(lib.bpf_pf_get_samples(e.h, sp, n, C.byref(cnt)))
                assert lib.bpf_wire_samples_to_pose_array(sp, n, pp) == 0

            def new(stride):
                e.check(lib.bpf_pf_get_pose_array(e.h, 0, stride, pp, n, C.byref(cnt)))

            rec[kind] = dict(parent=timed(parent, reps, warmup), new=timed(lambda: new(1), reps, warmup),
                             new_100=timed(lambda: new(100), reps, warmup))
            rec[kind]["parent_over_new"] = rec[kind]["parent"]["ms"] / rec[kind]["new"]["ms"]
            if kind == "registered":
                e.unregisterHostBuffer(samples)
                e.unregisterHostBuffer(poses)
        out[str(n)] = rec
    return out


def _worker(rank, world, port, exchange, reps, warmup, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    e = bpf.Engine(0)
    s = make_set(N_SHARDED)
    n = s.shape[0]
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world
    pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
    pf.initWithSamples(np.ascontiguousarray(s[lo:hi]))
    sf = ShardedFilter(HipShardBackend(e, None, pf, torch.device("cuda", 0)), dist, exchange=exchange)
    got = sf.get_pose_array(root=0)
    if rank == 0:
        assert got.shape == (n, 7) and np.array_equal(got[:, :2], s[:, :2])
    ts = []
    for rep in range(warmup + reps):
        dist.barrier()
        t0 = time.perf_counter()
        sf.get_pose_array(root=0)
        dt = time.perf_counter() - t0
        if rep >= warmup:
            ts.append(dt)
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(dict(ms=statistics.median(ts) * 1e3, min_ms=min(ts) * 1e3, mailbox=bool(sf.mailbox)), f)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


def sharded(worlds, reps, warmup):
    import torch.multiprocessing as mp
    out = {"note": "ranks share ONE GPU: launch and host cost only, nothing about xGMI", "particles": N_SHARDED}
    for world in worlds:
        for exchange in ("mailbox", "collective"):
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            path = os.path.join("/tmp", "time_pose_array_%d_%d_%s.json" % (os.getpid(), world, exchange))
            mp.spawn(_worker, args=(world, port, exchange, reps, warmup, path), nprocs=world, join=True)
            with open(path) as f:
                out["world_%d_%s" % (world, exchange)] = json.load(f)
            os.remove(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worlds", default="1,2,3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"statistic": "median (and min) wall ms per call, data in host memory on return", "reps": args.reps,
           "warmup": args.warmup}
    worlds = [int(w) for w in args.worlds.split(",") if w]
    if worlds:
        out["sharded"] = sharded(worlds, args.reps, args.warmup)  # before this process opens the GPU itself
    import torch  # noqa: F401 -- before the engine library, as everywhere
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    out["accuracy"] = accuracy(e)
    out["max_abs_dev_vs_host_libm"] = out["accuracy"]["max_abs_dev_vs_host_libm"]
    out["single"] = single(e, args.reps, args.warmup)
    e.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
