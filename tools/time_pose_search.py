#!/usr/bin/env python3
"""Wall time of an exhaustive pose search on the bench's 2000 x 2000 map against a 1081-beam scan: every free cell
(every cell_stride-th in i and j) at H headings, the best K = 1024 candidates.  Two modes that do the same job:

  --search    PlanarScanner.searchPoses (bpf_planar_search_poses): candidates generated, scored and selected on the
              device, one wait at the end;
  --explicit  what a caller could do before that call existed: the candidate poses built in numpy window by window,
              pushed through the registered host-buffer seam PlanarScanner.applyModelToSampleSet, every weight kept,
              np.argpartition at the end.  It uses nothing this tool's commit added, so the same file times an older
              build of the library (BPF_LIB=<path to libbadger_pf_hip.so>): symbols that build lacks are left unbound.

Configurations: max_beams 60 and 1081, (headings, cell_stride) (72, 2) and (36, 1); likelihood-field model, the
device-built distance LUT (the same cells are free for both modes: the free list is taken from the LUT read back).
Host clock around the whole job (the search call returns after its only wait; the explicit mode ends with host work);
--reps timed runs after one untimed run of every configuration, the median reported.  evals = candidates x the beams
the model integrates (the decimated beams below range_max).  The top-K candidate list is printed as a CRC so
that runs of one mode can be compared; between the modes it differs wherever several candidates share the K-th score
(np.argpartition keeps an arbitrary subset of them, the search the lowest candidates).
Run on the GPU box: python tools/time_pose_search.py --search|--explicit [--reps R] [--only BEAMS,H,S] [--out FILE];
prints one JSON line per configuration."""
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

MAP_SIZE, BEAMS, RANGE_MAX, K = 2000, 1081, 30.0, 1024
CONFIGS = [(60, 72, 2), (60, 36, 1), (1081, 72, 2), (1081, 36, 1)]
EXPLICIT_WINDOW = 1 << 20


def bind_what_the_library_has():
    """--explicit on an older build: drop the bindings of symbols it does not export"""
    import ctypes
    from badger_amcl_amd import _lib
    lib = ctypes.CDLL(_lib.SO)
    for name in list(_lib.SIGNATURES):
        if not hasattr(lib, name):
            del _lib.SIGNATURES[name]


def setup(e, max_beams):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    cells, origin = synth.make_map(MAP_SIZE, 0.05)
    pose = synth.true_pose(MAP_SIZE)
    ranges, angles = synth.cast_scan(cells, origin, 0.05, pose, BEAMS, seed=5)
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
    return m, sc, cells, origin, bpf.PlanarData(ranges, angles, RANGE_MAX)


def integrated_beams(ranges, max_beams):
    step = max((len(ranges) - 1) // (max_beams - 1), 1)
    r = ranges[::step]
    return int(np.sum(r < RANGE_MAX))


def free_list(m, cells, stride):
    from badger_amcl_amd import synth
    lut = m.getDistancesLUT()
    mask = (cells == -1) & (lut.astype(np.float64) > synth.MAP_FACTORS[2])
    ij = np.argwhere(mask.T)  # i outer, j inner
    return ij[(ij[:, 0] % stride == 0) & (ij[:, 1] % stride == 0)]


def explicit_search(e, sc, data, ij, origin, headings, buf, weights):
    """the candidates' poses in numpy, scored through the registered seam window by window; top K by argpartition"""
    total = ij.shape[0] * headings
    ox, oy = float(np.float32(origin[0])), float(np.float32(origin[1]))
    for a in range(0, total, EXPLICIT_WINDOW):
        b = min(a + EXPLICIT_WINDOW, total)
        c = np.arange(a, b, dtype=np.int64)
        f, h = c // headings, c % headings
        s = buf[:b - a]
        s[:, 0] = ox + (ij[f, 0] - MAP_SIZE // 2).astype(np.float64) * 0.05
        s[:, 1] = oy + (ij[f, 1] - MAP_SIZE // 2).astype(np.float64) * 0.05
        s[:, 2] = (2.0 * np.pi * h.astype(np.float64)) / float(headings) - np.pi
        s[:, 3] = 1.0
        sc.applyModelToSampleSet(data, s, 0)
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
    ap.add_argument("--only", default=None, help="BEAMS,H,S: that configuration alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.explicit:
        bind_what_the_library_has()
    import badger_amcl_amd as bpf
    configs = CONFIGS
    if args.only:
        configs = [tuple(int(v) for v in args.only.split(","))]
    lines = []
    for max_beams in sorted({c[0] for c in configs}):
        e = bpf.Engine(0)
        m, sc, cells, origin, data = setup(e, max_beams)
        beams = integrated_beams(data.ranges_, max_beams)
        buf = weights = None
        if args.explicit:
            buf = np.empty((EXPLICIT_WINDOW, 4), dtype=np.float64)
            e.registerHostBuffer(buf)
        for _, headings, stride in [c for c in configs if c[0] == max_beams]:
            if args.search:
                total, n_cells = sc.searchSpace(headings, stride)

                def job():
                    hits = sc.searchPoses(data, headings, stride, K)
                    return hits["candidate"], hits["score"]
            else:
                ij = free_list(m, cells, stride)
                total, n_cells = ij.shape[0] * headings, ij.shape[0]
                weights = np.empty(total, dtype=np.float64)

                def job():
                    return explicit_search(e, sc, data, ij, origin, headings, buf, weights)
            top, scores = job()  # untimed: allocations, the free list, code objects
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                top, scores = job()
                times.append(time.perf_counter() - t0)
            dt = statistics.median(times)
            line = dict(mode="search" if args.search else "explicit", max_beams=max_beams, headings=headings,
                        cell_stride=stride, k=K, free_cells=int(n_cells), candidates=int(total),
                        beams_integrated=beams, seconds_median=dt, seconds_all=times,
                        candidates_per_s=total / dt, evals_per_s=total * beams / dt, best_score=float(scores[0]),
                        best_candidate=int(top[0]),
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
