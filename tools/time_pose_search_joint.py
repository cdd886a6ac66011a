#!/usr/bin/env python3
"""Wall time of a joint pose search (PlanarScanner.searchPosesJoint, bpf_planar_search_poses_joint) on the bench's
2000 x 2000 map: every free cell with cell_stride 2 at 72 headings, likelihood-field model, K = 1024, at max_beams 1081
and 60, against S = 3 and S = 6 scans of 1081 beams cast along a short drive from the bench's true pose (scan s at
pose (+) D_s, D_s = s * (0.25 m, 0.02 m, 0.05 rad): the offsets the search is given).

Each line compares the joint call with the SUM of S single-scan PlanarScanner.searchPoses calls on the same scans in the
same process: that path is not touched by the joint form, so it is the parent's time for scoring the same scans.  Per
window the joint form adds S composition launches and drops S - 1 selections and S - 1 candidate launches; the planar
scans are staged per scoring call against a ring of four slots, so with S >= 4 the host may wait there.

Host clock around a call (each returns after its only wait for the rows); --reps timed runs after one untimed run, the
median reported.  The joint list is printed as a CRC so that runs can be compared.
Run on the GPU box: python tools/time_pose_search_joint.py [--reps R] [--only BEAMS,S] [--single] [--out FILE]; prints
one JSON line per configuration.  --single: two joint calls per configuration (the first allocates) and nothing else,
for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/time_pose_search_joint.py --single --only 1081,6)."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_pose_search import BEAMS, K, MAP_SIZE, RANGE_MAX, integrated_beams  # noqa: E402

HEADINGS, STRIDE = 72, 2
CONFIGS = [(1081, 3), (1081, 6), (60, 3), (60, 6)]
STEP = (0.25, 0.02, 0.05)  # the drive between two scans, in the frame of the pose before


def pose_add(pose, d):
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.array([pose[0] + d[0] * c - d[1] * s, pose[1] + d[0] * s + d[1] * c, pose[2] + d[2]])


def setup(e, max_beams, n_scans):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    cells, origin = synth.make_map(MAP_SIZE, 0.05)
    pose = np.asarray(synth.true_pose(MAP_SIZE), dtype=np.float64)
    m = bpf.OccupancyMap(e, 0.05)
    m.setCells(cells)
    m.setOrigin(origin)
    m.updateDistancesLUTExact(2.0)
    sc = bpf.PlanarScanner(e)
    sc.init(max_beams, m)
    p = synth.LF_DEFAULTS
    sc.setModelLikelihoodField(p["z_hit"], p["z_rand"], p["sigma_hit"], 2.0)
    sc.setMapFactors(*synth.MAP_FACTORS)
    sc.setPlanarScannerPose(synth.SCANNER_POSE)
    offsets = np.array([[s * v for v in STEP] for s in range(n_scans)], dtype=np.float64)
    datas = []
    for s in range(n_scans):
        ranges, angles = synth.cast_scan(cells, origin, 0.05, pose_add(pose, offsets[s]), BEAMS, seed=5 + s)
        datas.append(bpf.PlanarData(ranges, angles, RANGE_MAX))
    return m, sc, datas, offsets


def timed(job, reps):
    job()  # untimed: allocations, the free list, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        job()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="BEAMS,S: that configuration alone")
    ap.add_argument("--single", action="store_true", help="two joint calls per configuration, nothing else")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    configs = CONFIGS
    if args.only:
        configs = [tuple(int(v) for v in args.only.split(","))]
    lines = []
    for max_beams, n_scans in configs:
        e = bpf.Engine(0)
        m, sc, datas, offsets = setup(e, max_beams, n_scans)
        total, n_cells = sc.searchSpace(HEADINGS, STRIDE)
        if args.single:
            times = []
            for _ in range(2):  # (the first call allocates and loads code objects)
                t0 = time.perf_counter()
                hits = sc.searchPosesJoint(datas, offsets, HEADINGS, STRIDE, K)
                times.append(time.perf_counter() - t0)
            line = dict(mode="single", max_beams=max_beams, n_scans=n_scans, candidates=int(total), calls=2,
                        seconds_first_call=times[0], seconds_second_call=times[1],
                        best_candidate=int(hits["candidate"][0]))
        else:
            joint, joint_all = timed(lambda: sc.searchPosesJoint(datas, offsets, HEADINGS, STRIDE, K), args.reps)
            singles, singles_all = [], []
            for d in datas:
                t, all_t = timed(lambda: sc.searchPoses(d, HEADINGS, STRIDE, K), args.reps)
                singles.append(t)
                singles_all.append(all_t)
            hits = sc.searchPosesJoint(datas, offsets, HEADINGS, STRIDE, K)
            first = sc.searchPoses(datas[0], HEADINGS, STRIDE, K)
            beams = sum(integrated_beams(d.ranges_, max_beams) for d in datas)
            line = dict(mode="joint", max_beams=max_beams, n_scans=n_scans, headings=HEADINGS, cell_stride=STRIDE, k=K,
                        free_cells=int(n_cells), candidates=int(total), beams_integrated=beams,
                        joint_seconds_median=joint, joint_seconds_all=joint_all,
                        singles_seconds_sum=sum(singles), singles_seconds_median=singles,
                        singles_seconds_all=singles_all, joint_over_singles=joint / sum(singles),
                        evals_per_s=total * beams / joint, best_candidate=int(hits["candidate"][0]),
                        best_score=float(hits["score"][0]), single_scan_best_candidate=int(first["candidate"][0]),
                        top_k_crc="%08x" % zlib.crc32(np.ascontiguousarray(hits["candidate"]).tobytes()))
        print(json.dumps(line), flush=True)
        lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
