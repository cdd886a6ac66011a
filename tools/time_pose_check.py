#!/usr/bin/env python3
"""Wall time of random pose injection with Node::uniformPoseGenerator's score check in AS_REFERENCE form
(bpf_pf_set_uniform_pose_check: K rejected trials per call) on the 2000 x 2000 bench map with the LF model and a
1081-beam scan: initWithPoseFn at 100 k, and a 100 k recovery resample at w_diff 0.5 for both resamplers, for
(g0, m) = (0, -) (check inactive, K = 0), (10, 0.5) (K = 4) and (10, 0.99) (K = 230), and in SENSOR_MODEL form
(g0 = the 90th percentile of random poses' scores, m = 0.5).
w_diff 0.5: after the sensor update the tool writes w_slow = 1, w_fast = 0.5 into the engine's scalar block
(bpf_shard_scalars_dev) before the timed resample.
Run on the GPU box: python tools/time_pose_check.py [--reps R]; prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import badger_amcl_amd as bpf  # noqa: E402
from badger_amcl_amd.sharded import _DevArray  # noqa: E402
import badger_amcl_amd.pf as hpf  # noqa: E402
from badger_amcl_amd import synth  # noqa: E402

CHECKS = {"k0": (0.0, 0.5), "k4": (10.0, 0.5), "k230": (10.0, 0.99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=100000)
    args = ap.parse_args()
    size, beams, n = 2000, 1081, args.n
    e = bpf.Engine(0)
    cells, origin = synth.make_map(size)
    pose = synth.true_pose(size)
    ranges, angles = synth.cast_scan(cells, origin, 0.05, pose, beams, seed=5)
    m = bpf.OccupancyMap(e, 0.05)
    m.setCells(cells)
    m.setOrigin(origin)
    m.updateDistancesLUT(2.0)
    sc = bpf.PlanarScanner(e)
    sc.init(beams, m)
    p = synth.LF_DEFAULTS
    sc.setModelLikelihoodField(p["z_hit"], p["z_rand"], p["sigma_hit"], 2.0)
    sc.setMapFactors(*synth.MAP_FACTORS)
    sc.setPlanarScannerPose(synth.SCANNER_POSE)
    data = bpf.PlanarData(ranges, angles, 30.0)
    samples = synth.spread_cloud(n, size, seed=43, margin=0.5)
    out = {"n": n, "beams": beams, "map": size, "reps": args.reps}
    pf = bpf.ParticleFilter(e, 100, n, 0.001, 0.1, 85.0)
    ptr = C.c_void_p()
    e.check(e.lib.bpf_shard_scalars_dev(e.h, C.byref(ptr)))
    scalars = torch.as_tensor(_DevArray(ptr.value, (16,), "<f8"), device="cuda")

    def set_w_diff_half():
        pf.getState()  # the engine's stream is idle
        scalars[1:3] = torch.tensor([1.0, 0.5], dtype=torch.float64)
        torch.cuda.synchronize()
    pf.srand48(42)
    pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)

    def measure(name):
        pf.initWithRandomPoses()  # warm-up (free-space list, buffers)
        pf.getState()
        t = 0.0
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pf.initWithRandomPoses()
            pf.getState()
            t += time.perf_counter() - t0
        out["init_%s_ms" % name] = t / args.reps * 1e3
        for resampler, rname in ((0, "multinomial"), (1, "systematic")):
            pf.setResampleModel(resampler)
            t, wd, M = 0.0, 0.0, 0
            for rep in range(args.reps + 1):
                pf.initWithSamples(samples)
                sc.updateSensor(pf, data)
                set_w_diff_half()
                t0 = time.perf_counter()
                pf.updateResample()
                st = pf.getState()
                if rep:  # the first one warms up
                    t += time.perf_counter() - t0
                wd, M = st.w_diff, st.sample_count
            out["resample_%s_%s_ms" % (rname, name)] = t / args.reps * 1e3
            out["resample_%s_%s_w_diff" % (rname, name)] = wd
            out["resample_%s_%s_M" % (rname, name)] = M

    for name, (g0, mult) in CHECKS.items():
        pf.setUniformPoseCheck(g0, mult)
        out["K_" + name] = hpf.uniform_pose_retries(g0, mult)
        measure(name)
    # SENSOR_MODEL: the threshold at the 90th percentile of the scores of random free-space poses against the scan,
    # multiplier 0.5
    pf.setUniformPoseCheck(0.0, 0.5)
    pf.initWithRandomPoses()
    cand = pf.getCurrentSet().samples.copy()
    cand[:, 3] = 1.0
    sc.applyModelToSampleSet(data, cand, 0)
    g0 = float(np.quantile(cand[:, 3], 0.9))
    out["sensor_g0"] = g0
    sc.updateSensor(pf, data)  # the scan the scores use
    pf.setUniformPoseCheck(g0, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)
    measure("sensor")
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
