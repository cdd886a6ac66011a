#!/usr/bin/env python3
"""Evaluation counts of the pruned pose search over a sharded filter (LocalShardedFilter.search_poses_pruned) beside
the single engine's call and beside the ranks' stand-alone range calls (what the collectives route of ShardedFilter
runs: no shared tau), on the bench's 2000 x 2000 map against its 1081-beam scan.

W engines on ONE device in one process (a local world): the wall time printed is W ranks sharing one GPU, not a
speed-up -- nothing here runs between two GPUs.  What a multi-GPU run would be bound by is the largest rank's window
count, printed per line.

Configurations: max_beams 1081, (headings, cell_stride) (72, 2) and (36, 1), K = 1 and 1024, B = 8, W = 2, 4, 8;
likelihood-field model, map and scan of tools/time_pose_search.py.  Host clock around the whole collective call,
--reps timed runs after one untimed run, the median reported.  Every result is compared with the single engine's rows
as bytes.  Run on the GPU box: python tools/time_pose_search_sharded.py [--reps R] [--worlds 2,4,8] [--out FILE];
prints one JSON line per configuration."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_pose_search import setup  # noqa: E402
from time_pose_search_pruned import timed  # noqa: E402

MAX_BEAMS, BLOCK = 1081, 8
SPACES = ((72, 2), (36, 1))
KS = (1, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    worlds = [int(v) for v in args.worlds.split(",")]
    single = bpf.Engine(0)
    m1, sc, cells, origin, data = setup(single, MAX_BEAMS)
    engines = [bpf.Engine(0) for _ in range(max(worlds))]
    keep, pfs = [], []
    for e in engines:
        keep.append(setup(e, MAX_BEAMS)[:2])
        pfs.append(bpf.ParticleFilter(e, 100, 1000, 0.0, 0.0, 85.0))
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for headings, stride in SPACES:
        nb = sc.searchBlocks(stride, BLOCK)
        for k in KS:
            (want, st1), t1, _ = timed(lambda: sc.searchPosesPruned(data, headings, stride, k, BLOCK, stats=True),
                                       args.reps)
            emit(dict(mode="single", headings=headings, cell_stride=stride, k=k, block=BLOCK, blocks=nb,
                      seconds_median=t1, **st1))
            for W in worlds:
                f = LocalShardedFilter(pfs[:W], kld_count=0)
                try:
                    (rows, stats), dt, _ = timed(
                        lambda: f.search_poses_pruned(data, headings, stride, k, BLOCK), args.reps)
                finally:
                    f.close()
                alone = []
                for r in range(W):
                    lo, hi = (nb * r) // W, (nb * (r + 1)) // W
                    hits, st = sc.searchPosesPruned(data, headings, stride, k, BLOCK, lo, hi - lo, stats=True)
                    alone.append(st)
                emit(dict(mode="sharded", headings=headings, cell_stride=stride, k=k, block=BLOCK, world=W,
                          same_rows=rows.tobytes() == want.tobytes(), seconds_median_one_device=dt,
                          scored_floor=[st["scored_candidates"] for st in stats],
                          scored_alone=[st["scored_candidates"] for st in alone],
                          windows_floor=[st["windows"] for st in stats], windows_alone=[st["windows"] for st in alone],
                          scored_floor_sum=sum(st["scored_candidates"] for st in stats),
                          scored_alone_sum=sum(st["scored_candidates"] for st in alone),
                          windows_floor_sum=sum(st["windows"] for st in stats),
                          windows_alone_sum=sum(st["windows"] for st in alone),
                          windows_floor_max=max(st["windows"] for st in stats),
                          windows_alone_max=max(st["windows"] for st in alone),
                          list_bytes_per_rank=16 * (k + 1) * W, floor_bytes_per_rank=8 * W))
    for e in engines + [single]:
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
