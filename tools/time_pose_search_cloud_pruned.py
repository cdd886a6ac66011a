#!/usr/bin/env python3
"""Wall time of the pruned cloud pose search (PointCloudScanner.searchPosesPruned) beside the exhaustive one
(PointCloudScanner.searchPoses) in the same process, on the 400 x 300-column hall and the clouds of
tools/time_pose_search_cloud.py, with the pruned call's stats.  The exhaustive path is untouched by the pruned one, so
its time is the parent commit's.

Configurations: clouds of 2 048 and 65 536 points, (headings, cell_stride) (72, 1) and (72, 2), K = 1 and 1024, B = 4,
8, 16, 32; the plain cloud model, a yaw-only mounting, resolution 0.05.  Host clock around the whole call; --reps timed
runs after one untimed run of every configuration (which also builds the cached pooled volume and block list), the
median reported.  Every pruned result is compared with the exhaustive rows as bytes.
Run on the GPU box: python tools/time_pose_search_cloud_pruned.py [--reps R] [--only POINTS,H,S] [--blocks 4,8]
[--ks 1,1024] [--out FILE]; prints one JSON line per configuration.  --once POINTS,H,S,K,B runs that pruned call
alone, twice (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_pose_search_cloud import CONFIGS, HALL_HI, HALL_LO, MAX_DIST, RES, setup  # noqa: E402

KS = (1, 1024)
BLOCKS = (4, 8, 16, 32)


def timed(job, reps):
    out = job()  # untimed: allocations, the cached list and volume, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = job()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="POINTS,H,S: that configuration alone")
    ap.add_argument("--blocks", default=",".join(str(b) for b in BLOCKS))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--once", default=None, help="POINTS,H,S,K,B: that pruned call alone, twice")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    lut = synth.box_room_lut(RES, MAX_DIST, lo=HALL_LO, hi=HALL_HI)
    if args.once:
        points, headings, stride, k, block = (int(v) for v in args.once.split(","))
        e = bpf.Engine(0)
        om, sc, data = setup(e, lut, points)
        for _ in range(2):
            hits, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
        print(json.dumps(dict(mode="once", points=points, headings=headings, cell_stride=stride, k=k, block=block,
                              best_candidate=int(hits["candidate"][0]), **st)))
        e.close()
        return
    configs = CONFIGS
    if args.only:
        configs = [tuple(int(v) for v in args.only.split(","))]
    ks = [int(v) for v in args.ks.split(",")]
    blocks = [int(v) for v in args.blocks.split(",")]
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for points in sorted({c[0] for c in configs}):
        e = bpf.Engine(0)
        om, sc, data = setup(e, lut, points)
        for _, headings, stride in [c for c in configs if c[0] == points]:
            total, _ = sc.searchSpace(headings, stride)
            for k in ks:
                want, t_ex, all_ex = timed(lambda: sc.searchPoses(data, headings, stride, k), args.reps)
                emit(dict(mode="exhaustive", points=points, headings=headings, cell_stride=stride, k=k,
                          candidates=total, ms=round(t_ex * 1e3, 3), all_ms=[round(t * 1e3, 3) for t in all_ex]))
                for block in blocks:
                    (got, st), t_pr, all_pr = timed(
                        lambda: sc.searchPosesPruned(data, headings, stride, k, block, stats=True), args.reps)
                    emit(dict(mode="pruned", points=points, headings=headings, cell_stride=stride, k=k, block=block,
                              ms=round(t_pr * 1e3, 3), all_ms=[round(t * 1e3, 3) for t in all_pr],
                              speedup=round(t_ex / t_pr, 3), rows_equal=bool(got.tobytes() == want.tobytes()),
                              scored_share=round(st["scored_candidates"] / max(st["candidates"], 1), 4), **st))
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(line.get("rows_equal", True) for line in lines):
        sys.exit("a pruned result differs from the exhaustive rows")


if __name__ == "__main__":
    main()
