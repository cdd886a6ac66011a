#!/usr/bin/env python3
"""Wall time of an exhaustive pose search with the cloud scanner: a 400 x 300-column hall (synth.box_room_lut with its
corners scaled), a synth.grid_cloud of the hall, every column (every cell_stride-th in i and j) at H headings, the best
K = 1024 candidates.  Two modes that do the same job:

  --search    PointCloudScanner.searchPoses (bpf_cloud_search_poses): the cloud staged once, candidates generated,
              scored and selected on the device window after window, one wait at the end;
  --explicit  what a caller could do before that call existed: the candidate poses built in numpy window by window,
              pushed through the registered host-buffer seam PointCloudScanner.applyModelToSampleSet, every weight
              kept, np.argpartition at the end.  It uses nothing this tool's commit added, so the same file times an
              older build of the library (BPF_LIB=<path to libbadger_pf_hip.so>): symbols that build lacks are left
              unbound.

Configurations: clouds of 2 048 and 65 536 points, (headings, cell_stride) (72, 1) and (72, 2); the plain cloud model,
a yaw-only mounting (the planar dense kernel, resolution 0.05: its exact-reciprocal BORDER form).  Host clock around the
whole job; --reps timed runs after one untimed run of every configuration, the median reported.  evals = candidates x
points.  The top-K candidate list is printed as a CRC so that runs of one mode can be compared; between the modes it
differs wherever several candidates share the K-th score (np.argpartition keeps an arbitrary subset of them, the
search the lowest candidates).
Run on the GPU box: python tools/time_pose_search_cloud.py --search|--explicit [--reps R] [--only POINTS,H,S]
[--out FILE]; prints one JSON line per configuration."""
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

RES, MAX_DIST, K = 0.05, 0.3, 1024
HALL_LO, HALL_HI = (-197, -147, -2), (197, 147, 20)  # + 3 cells of padding: columns [-200, 200) x [-150, 150)
CLOUDS = {2048: (2, 1024), 65536: (64, 1024)}         # points: (rows, cols) of grid_cloud
CONFIGS = [(2048, 72, 1), (2048, 72, 2), (65536, 72, 1), (65536, 72, 2)]
TF_XYZ = (0.2, -0.1, 0.5)
TF_QUAT = (0.0, 0.0, float(np.sin(0.15)), float(np.cos(0.15)))
EXPLICIT_WINDOW = 1 << 20


def bind_what_the_library_has():
    """--explicit on an older build: drop the bindings of symbols it does not export"""
    import ctypes
    from badger_amcl_amd import _lib
    lib = ctypes.CDLL(_lib.SO)
    for name in list(_lib.SIGNATURES):
        if not hasattr(lib, name):
            del _lib.SIGNATURES[name]


def setup(e, lut, points):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    pose_indices, ratios, mn, mx = lut
    om = bpf.OctoMap(e, RES)
    om.setDistancesLUT(pose_indices, ratios, mn, mx, MAX_DIST)
    sc = bpf.PointCloudScanner(e)
    sc.init(points, om)
    sc.setPointCloudModel(0.5, 0.05, 0.1)
    sc.setMapFactors(0.95, 0.95, 0.3)
    sc.setPointCloudScannerToFootprintTF(TF_XYZ, TF_QUAT)
    rows, cols = CLOUDS[points]
    lo = (HALL_LO[0] * RES, HALL_LO[1] * RES, -0.1)
    hi = (HALL_HI[0] * RES, HALL_HI[1] * RES, 1.0)
    pts = synth.grid_cloud(rows, cols, origin=(0.3, 0.2, 0.6), room_lo=lo, room_hi=hi)
    assert pts.shape[0] == points
    return om, sc, bpf.PointCloudData(pts)


def columns(mn, mx, stride):
    """(i0, n_i, j0, n_j) of the columns min <= c < max that the stride divides"""
    i0 = -((-int(mn[0])) // stride) * stride
    j0 = -((-int(mn[1])) // stride) * stride
    n_i = (int(mx[0]) - 1 - i0) // stride + 1 if i0 < int(mx[0]) else 0
    n_j = (int(mx[1]) - 1 - j0) // stride + 1 if j0 < int(mx[1]) else 0
    return i0, n_i, j0, n_j


def explicit_search(sc, data, cols, stride, headings, buf, weights):
    """the candidates' poses in numpy, scored through the registered seam window by window; top K by argpartition"""
    i0, n_i, j0, n_j = cols
    total = n_i * n_j * headings
    for a in range(0, total, EXPLICIT_WINDOW):
        b = min(a + EXPLICIT_WINDOW, total)
        c = np.arange(a, b, dtype=np.int64)
        f, h = c // headings, c % headings
        s = buf[:b - a]
        s[:, 0] = (i0 + (f // n_j) * stride).astype(np.float64) * RES
        s[:, 1] = (j0 + (f % n_j) * stride).astype(np.float64) * RES
        s[:, 2] = (2.0 * np.pi * h.astype(np.float64)) / float(headings) - np.pi
        s[:, 3] = 1.0
        sc.applyModelToSampleSet(data, s)
        weights[a:b] = s[:, 3]
    w = weights[:total]
    top = np.argpartition(-w, K)[:K] if total > K else np.arange(total)
    top = top[np.lexsort((top, -w[top]))]
    return top, w[top]


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--search", action="store_true")
    mode.add_argument("--explicit", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="POINTS,H,S: that configuration alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.explicit:
        bind_what_the_library_has()
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    configs = CONFIGS
    if args.only:
        configs = [tuple(int(v) for v in args.only.split(","))]
    lut = synth.box_room_lut(RES, MAX_DIST, lo=HALL_LO, hi=HALL_HI)
    lines = []
    for points in sorted({c[0] for c in configs}):
        e = bpf.Engine(0)
        om, sc, data = setup(e, lut, points)
        buf = weights = None
        if args.explicit:
            buf = np.empty((EXPLICIT_WINDOW, 4), dtype=np.float64)
            e.registerHostBuffer(buf)
        for _, headings, stride in [c for c in configs if c[0] == points]:
            cols = columns(lut[2], lut[3], stride)
            total, n_cols = cols[1] * cols[3] * headings, cols[1] * cols[3]
            if args.search:
                assert sc.searchSpace(headings, stride) == (total, n_cols)

                def job():
                    hits = sc.searchPoses(data, headings, stride, K)
                    return hits["candidate"], hits["score"]
            else:
                weights = np.empty(total, dtype=np.float64)

                def job():
                    return explicit_search(sc, data, cols, stride, headings, buf, weights)
            top, scores = job()  # untimed: allocations, code objects
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                top, scores = job()
                times.append(time.perf_counter() - t0)
            dt = statistics.median(times)
            line = dict(mode="search" if args.search else "explicit", points=points, headings=headings,
                        cell_stride=stride, k=K, columns=int(n_cols), candidates=int(total), seconds_median=dt,
                        seconds_all=times, candidates_per_s=total / dt, evals_per_s=total * points / dt,
                        best_score=float(scores[0]), best_candidate=int(top[0]), cloud_form=e.cloud_last_form(),
                        top_k_crc="%08x" % zlib.crc32(np.ascontiguousarray(top, dtype=np.int64).tobytes()),
                        library=os.environ.get("BPF_LIB", "in-tree"))
            print(json.dumps(line), flush=True)
            lines.append(line)
        if args.explicit:
            e.unregisterHostBuffer(buf)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
