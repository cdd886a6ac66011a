#!/usr/bin/env python3
"""Wall time of refining the hits of a coarse pose search on the bench's 2000 x 2000 map against its 1081-beam scan,
and what the refinement buys.  The coarse search is (headings, cell_stride) = (36, 4), K = 1024; the lattice descent
is (xy_radius, theta_radius, levels) = (2, 2, 5) with xy_step one cell (the lattice spans +-2 cells, half the stride)
and theta_step a quarter of the heading step (+-5 degrees), so that the last level moves by res / 16 and 0.16 degrees.
Two modes that do the same descent:

  --refine    PlanarScanner.refinePoses (bpf_planar_refine_poses): lattice poses generated, scored and the argmax taken
              on the device, every level enqueued behind the one before, one wait at the end.  Also reports the best
              pose of coarse search + refinement beside the best of the fine search (72, 2), with the candidates each
              evaluated (--no-fine skips the fine search);
  --explicit  the same descent done by the caller: per level the 1024 x 125 lattice poses built in numpy, pushed
              through the registered host-buffer seam PlanarScanner.applyModelToSampleSet, the argmax under the order
              rule in numpy.  It uses nothing this tool's commit added, so the same file times an older build of the
              library (BPF_LIB=<path to libbadger_pf_hip.so>): symbols that build lacks are left unbound.

Configurations: max_beams 60 and 1081; likelihood-field model, the device-built distance LUT.  Host clock around the
whole refinement (the call returns after its only wait; the explicit mode ends with host work); --reps timed runs
after one untimed run, the median and every run reported.  --hits FILE: the coarse search's hits are read from FILE
when it exists and written to it otherwise, so that a profiler run holds the refinement's launches only.
Run on the GPU box: python tools/time_pose_refine.py --refine|--explicit [--reps R] [--only BEAMS] [--hits FILE]
[--out FILE]; prints one JSON line per configuration."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_pose_search as tps  # noqa: E402  (the map, the scan and the scanner of that tool)

COARSE, FINE, K = (36, 4), (72, 2), 1024
R, A, L = 2, 2, 5
XY_STEP = 0.05
THETA_STEP = (2.0 * math.pi / COARSE[0]) / 4.0


def lattice_offsets():
    side, turns = 2 * R + 1, 2 * A + 1
    m = np.arange(side * side * turns)
    ab, t = m // turns, m % turns
    return (ab // side - R).astype(np.float64), (ab % side - R).astype(np.float64), (t - A).astype(np.float64)


def explicit_refine(sc, data, poses, buf):
    """the descent of bpf_planar_refine_poses by the caller: (final poses, scores, trace)"""
    da, db, dt = lattice_offsets()
    M = da.shape[0]
    mc = (M - 1) // 2
    c = np.array(poses, dtype=np.float64)
    n = c.shape[0]
    rows = np.arange(n)
    trace = np.empty((n, L), dtype=np.int32)
    score = None
    for level in range(L):
        d, q = math.ldexp(XY_STEP, -level), math.ldexp(THETA_STEP, -level)
        s = buf[:n * M].reshape(n, M, 4)
        s[:, :, 0] = c[:, None, 0] + (da * d)[None, :]
        s[:, :, 1] = c[:, None, 1] + (db * d)[None, :]
        s[:, :, 2] = c[:, None, 2] + (dt * q)[None, :]
        s[:, :, 3] = 1.0
        sc.applyModelToSampleSet(data, buf[:n * M], 0)
        w = s[:, :, 3]
        key = np.where(np.isnan(w), -np.inf, w)
        best = key == key.max(axis=1)[:, None]
        m = np.where(best[:, mc], mc, np.argmax(best, axis=1))
        go = m != mc
        c = np.where(go[:, None], s[rows, m, :3], c)
        score = w[rows, m].copy()
        trace[:, level] = m
    return c, score, trace


def crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--refine", action="store_true")
    mode.add_argument("--explicit", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="max_beams: that configuration alone")
    ap.add_argument("--hits", default=None, help="file the coarse hits are read from (written to when missing)")
    ap.add_argument("--no-fine", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.explicit:
        tps.bind_what_the_library_has()
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    lines = []
    for max_beams in [args.only] if args.only else [60, 1081]:
        e = bpf.Engine(0)
        m, sc, cells, origin, data = tps.setup(e, max_beams)
        beams = tps.integrated_beams(data.ranges_, max_beams)
        hits_file = args.hits and "%s.%d.npy" % (args.hits, max_beams)
        line = dict(mode="refine" if args.refine else "explicit", max_beams=max_beams, beams_integrated=beams,
                    coarse=COARSE, lattice=(R, A, L), xy_step=XY_STEP, theta_step=THETA_STEP,
                    true_pose=[float(v) for v in synth.true_pose(tps.MAP_SIZE)],
                    library=os.environ.get("BPF_LIB", "in-tree"))
        if hits_file and os.path.exists(hits_file):
            hits = np.load(hits_file)
        else:
            sc.searchPoses(data, COARSE[0], COARSE[1], K)  # untimed
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                hits = sc.searchPoses(data, COARSE[0], COARSE[1], K)
                times.append(time.perf_counter() - t0)
            line.update(coarse_candidates=int(sc.searchSpace(*COARSE)[0]), coarse_seconds_median=statistics.median(times),
                        coarse_seconds_all=times)
            if hits_file:
                np.save(hits_file, hits)
        poses = np.ascontiguousarray(hits["pose"])
        n = poses.shape[0]
        M = (2 * R + 1) ** 2 * (2 * A + 1)
        if args.refine:
            def job():
                rows, trace = sc.refinePoses(data, poses, R, XY_STEP, A, THETA_STEP, L, trace=True)
                return np.ascontiguousarray(rows["pose"]), rows["score"], trace
        else:
            buf = np.empty((n * M, 4), dtype=np.float64)
            e.registerHostBuffer(buf)

            def job():
                return explicit_refine(sc, data, poses, buf)
        final, score, trace = job()  # untimed: allocations, code objects
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            final, score, trace = job()
            times.append(time.perf_counter() - t0)
        dt = statistics.median(times)
        evaluated = n * M * L
        best = int(np.lexsort((np.arange(n), -np.where(np.isnan(score), -np.inf, score)))[0])
        line.update(poses=n, lattice_points=M, refine_candidates=evaluated, seconds_median=dt, seconds_all=times,
                    candidates_per_s=evaluated / dt, evals_per_s=evaluated * beams / dt,
                    coarse_best_score=float(hits["score"][0]), coarse_best_pose=hits["pose"][0].tolist(),
                    refined_best_score=float(score[best]), refined_best_pose=final[best].tolist(),
                    refined_best_row=best, moved_share=float((trace != (M - 1) // 2).mean()),
                    poses_crc=crc(final), trace_crc=crc(trace.astype(np.int32)))
        if args.refine and not args.no_fine:
            fine = sc.searchPoses(data, FINE[0], FINE[1], K)
            line.update(fine=FINE, fine_candidates=int(sc.searchSpace(*FINE)[0]), fine_best_score=float(fine["score"][0]),
                        fine_best_pose=fine["pose"][0].tolist())
        if args.explicit:
            e.unregisterHostBuffer(buf)
        print(json.dumps(line), flush=True)
        lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
