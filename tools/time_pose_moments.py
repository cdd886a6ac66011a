#!/usr/bin/env python3
"""Wall time of the pose moments of the hits of a coarse pose search on the bench's 2000 x 2000 map against its
1081-beam scan.  The coarse search and the lattice are those of tools/time_pose_refine.py: (headings, cell_stride) =
(36, 4), K = 1024 hits; (xy_radius, theta_radius) = (2, 2), so M = 125 points per hit, xy_step one cell, theta_step a
quarter of the heading step; baseline 0.5.  Three jobs over the same 1024 x 125 lattice poses, each timed alone:

  moments   PlanarScanner.poseMoments (bpf_planar_pose_moments): lattice poses generated and scored and the moments
            reduced on the device, the groups enqueued back to back, one wait for the rows;
  refine1   PlanarScanner.refinePoses with levels = 1: the same lattices generated and scored on the device, reduced to
            an argmax -- the yardstick for what the moment kernel adds;
  explicit  the caller's way through the existing interface: the lattice poses built in numpy, pushed through the
            registered host-buffer seam PlanarScanner.applyModelToSampleSet, the moments formed in numpy.

Configurations: max_beams 61 and 1081; likelihood-field model, the device-built distance LUT.  Host clock around each
whole job; --reps timed runs after one untimed run; the median with the fastest and slowest run reported.
Run on the GPU box: python tools/time_pose_moments.py [--reps R] [--only BEAMS] [--out FILE]; prints one JSON line per
configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_pose_refine as tpr  # noqa: E402  (the search, the lattice and its steps)
import time_pose_search as tps  # noqa: E402  (the map, the scan and the scanner)

R, A = tpr.R, tpr.A
BASELINE = 0.5


def explicit_moments(sc, data, poses, buf):
    """the moments by the caller: (mean[n, 3], cov[n, 3, 3]) from the seam's scores of the explicit lattice poses"""
    da, db, dt = tpr.lattice_offsets()
    M = da.shape[0]
    n = poses.shape[0]
    s = buf[:n * M].reshape(n, M, 4)
    s[:, :, 0] = poses[:, None, 0] + (da * tpr.XY_STEP)[None, :]
    s[:, :, 1] = poses[:, None, 1] + (db * tpr.XY_STEP)[None, :]
    s[:, :, 2] = poses[:, None, 2] + (dt * tpr.THETA_STEP)[None, :]
    s[:, :, 3] = 1.0
    sc.applyModelToSampleSet(data, buf[:n * M], 0)
    score = np.where(np.isnan(s[:, :, 3]), -np.inf, s[:, :, 3])
    thr = BASELINE * score.max(axis=1)
    w = np.maximum(score - thr[:, None], 0.0)
    off = np.stack([da, db, dt])  # [3, M]
    W = w.sum(axis=1)
    m = (w @ off.T) / W[:, None]
    second = np.einsum("nm,um,vm->nuv", w, off, off) / W[:, None, None]
    step = np.array([tpr.XY_STEP, tpr.XY_STEP, tpr.THETA_STEP])
    cov = (second - m[:, :, None] * m[:, None, :]) * step[:, None] * step[None, :]
    return poses + m * step, cov


def timed(job, reps):
    job()  # untimed: allocations, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = job()
        times.append(time.perf_counter() - t0)
    return out, dict(median=statistics.median(times), min=min(times), max=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", type=int, default=None, help="max_beams: that configuration alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    lines = []
    for max_beams in [args.only] if args.only else [61, 1081]:
        e = bpf.Engine(0)
        m, sc, cells, origin, data = tps.setup(e, max_beams)
        beams = tps.integrated_beams(data.ranges_, max_beams)
        hits = sc.searchPoses(data, tpr.COARSE[0], tpr.COARSE[1], tpr.K)
        poses = np.ascontiguousarray(hits["pose"])
        n = poses.shape[0]
        M = (2 * R + 1) ** 2 * (2 * A + 1)
        rows, t_moments = timed(lambda: sc.poseMoments(data, poses, R, tpr.XY_STEP, A, tpr.THETA_STEP, BASELINE),
                                args.reps)
        _, t_scores = timed(lambda: sc.poseMoments(data, poses, R, tpr.XY_STEP, A, tpr.THETA_STEP, BASELINE,
                                                   scores=True), args.reps)
        _, t_refine = timed(lambda: sc.refinePoses(data, poses, R, tpr.XY_STEP, A, tpr.THETA_STEP, 1), args.reps)
        buf = np.empty((n * M, 4), dtype=np.float64)
        e.registerHostBuffer(buf)
        (mean, cov), t_explicit = timed(lambda: explicit_moments(sc, data, poses, buf), args.reps)
        e.unregisterHostBuffer(buf)
        valid = (rows["flags"] & 1) != 0
        dev_cov = rows["cov"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
        line = dict(max_beams=max_beams, beams_integrated=beams, poses=n, lattice=(R, A), lattice_points=M,
                    xy_step=tpr.XY_STEP, theta_step=tpr.THETA_STEP, baseline=BASELINE, reps=args.reps,
                    seconds_moments=t_moments, seconds_moments_with_scores=t_scores, seconds_refine_one_level=t_refine,
                    seconds_explicit=t_explicit, valid_rows=int(valid.sum()),
                    face_rows=int(((rows["flags"] & 14) != 0).sum()),
                    explicit_mean_deviation=float(np.abs(mean[valid] - rows["mean"][valid]).max()),
                    explicit_cov_deviation=float(np.abs(cov[valid] - dev_cov[valid]).max()),
                    sigma_xy_median=float(np.median(np.sqrt(np.maximum(rows["cov"][valid][:, [0, 3]], 0.0)))),
                    sigma_theta_median=float(np.median(np.sqrt(np.maximum(rows["cov"][valid][:, 5], 0.0)))))
        print(json.dumps(line), flush=True)
        lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
