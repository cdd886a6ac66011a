#!/usr/bin/env python3
"""Wall time of the pruned pose search (PlanarScanner.searchPosesPruned) beside the exhaustive one
(PlanarScanner.searchPoses) in the same session, on the bench's 2000 x 2000 map against its 1081-beam scan, with the
pruned call's stats.  The exhaustive path is untouched by the pruned one, so its time is the parent commit's.

Configurations: max_beams 60 and 1081, (headings, cell_stride) (72, 2) and (36, 1), K = 1 and 1024, B = 4, 8, 16, 32;
likelihood-field model, the device-built distance LUT, map and scan of tools/time_pose_search.py.  Host clock around
the whole call; --reps timed runs after one untimed run of every configuration (which also builds the cached pooled
image and block list), the median reported.  Every pruned result is compared with the exhaustive rows as bytes.
Run on the GPU box: python tools/time_pose_search_pruned.py [--reps R] [--only BEAMS,H,S] [--blocks 4,8] [--ks 1,1024]
[--out FILE]; prints one JSON line per configuration.  --once BEAMS,H,S,K,B runs that pruned call alone, twice (for a
kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_pose_search import CONFIGS, integrated_beams, setup  # noqa: E402

KS = (1, 1024)
BLOCKS = (4, 8, 16, 32)


def timed(job, reps):
    out = job()  # untimed: allocations, cached lists and images, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = job()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="BEAMS,H,S: that configuration alone")
    ap.add_argument("--blocks", default=",".join(str(b) for b in BLOCKS))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--once", default=None, help="BEAMS,H,S,K,B: that pruned call alone, twice")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    if args.once:
        max_beams, headings, stride, k, block = (int(v) for v in args.once.split(","))
        e = bpf.Engine(0)
        m, sc, cells, origin, data = setup(e, max_beams)
        for _ in range(2):
            hits, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
        print(json.dumps(dict(mode="once", max_beams=max_beams, headings=headings, cell_stride=stride, k=k,
                              block=block, best_candidate=int(hits["candidate"][0]), **st)))
        e.close()
        return
    configs = CONFIGS
    if args.only:
        configs = [tuple(int(v) for v in args.only.split(","))]
    blocks = [int(v) for v in args.blocks.split(",")]
    ks = [int(v) for v in args.ks.split(",")]
    lines = []
    for max_beams in sorted({c[0] for c in configs}):
        e = bpf.Engine(0)
        m, sc, cells, origin, data = setup(e, max_beams)
        beams = integrated_beams(data.ranges_, max_beams)
        for _, headings, stride in [c for c in configs if c[0] == max_beams]:
            total, n_cells = sc.searchSpace(headings, stride)
            for k in ks:
                want, t_ex, t_ex_all = timed(lambda: sc.searchPoses(data, headings, stride, k), args.reps)
                line = dict(mode="exhaustive", max_beams=max_beams, headings=headings, cell_stride=stride, k=k,
                            candidates=int(total), beams_integrated=beams, seconds_median=t_ex, seconds_all=t_ex_all)
                print(json.dumps(line), flush=True)
                lines.append(line)
                for block in blocks:
                    try:
                        (hits, st), dt, all_t = timed(
                            lambda: sc.searchPosesPruned(data, headings, stride, k, block, stats=True), args.reps)
                    except bpf.BpfError as err:
                        line = dict(mode="pruned", max_beams=max_beams, headings=headings, cell_stride=stride, k=k,
                                    block=block, error=str(err))
                        print(json.dumps(line), flush=True)
                        lines.append(line)
                        continue
                    line = dict(mode="pruned", max_beams=max_beams, headings=headings, cell_stride=stride, k=k,
                                block=block, beams_integrated=beams, seconds_median=dt, seconds_all=all_t,
                                speedup=t_ex / dt, scored_ratio=st["scored_candidates"] / max(st["candidates"], 1),
                                same_rows=hits.tobytes() == want.tobytes(), **st)
                    print(json.dumps(line), flush=True)
                    lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
