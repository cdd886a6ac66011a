"""Times what the imbalance cap of the in-place systematic resample costs against rebalancing behind it
(include/badger_pf.h, bpf_shard_set_rebalance), back to back, on ONE GPU:

  step   restore, sensor update, resample of ONE filter of 100 k particles x 1081 beams on the 2000 x 2000 map
         (bench.py's headline workload, systematic resampler), split evenly over W = 1, 2, 4 ranks in this process
         (badger_amcl_amd.local_world.LocalShardedFilter).  The set is a spread cloud whose first quarter sits tightly
         around the true pose: the sensor update puts nearly all the weight, and so nearly all the teeth, on rank 0.
  cap    resample_form="in_place", rebalance="off": what the filter did before -- where the largest slice would exceed
         max_share * ceil(M / W) (2.0: only W > 2 can trip it) the resample falls back to the window form
  auto   resample_form="in_place", rebalance="auto" (trigger_share 1.5): always in place, then the slices go back to
         the even split

Medians over --repeats runs, with the spread of the runs beside them, written to profiles/shard_rebalance.json.  With
every rank on one GPU the numbers bound the launch and host cost of the two protocols only.  What crosses -- 32 B per
moved sample into every rank for the rebalance, 48 B per new sample into every rank for the window -- costs nothing
here: nothing has run between two GPUs, and that figure stays unmeasured.

usage: python tools/time_shard_rebalance.py [--out profiles/shard_rebalance.json] [--repeats 5] [--steps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_world(W, wl, samples, lut, rebalance):
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    from badger_amcl_amd.local_world import LocalShardedFilter
    n = samples.shape[0]
    engines, keep, pfs = [], [], []
    for r in range(W):
        e = bpf.Engine(0)
        m = bpf.OccupancyMap(e, 0.05)
        m.setCells(wl["cells"])
        m.setOrigin(wl["origin"])
        m.setDistancesLUT(lut, 2.0)
        sc = bpf.PlanarScanner(e)
        sc.init(wl["beams"], m)
        p = synth.LF_DEFAULTS
        sc.setModelLikelihoodField(p["z_hit"], p["z_rand"], p["sigma_hit"], 2.0)
        sc.setMapFactors(*synth.MAP_FACTORS)
        sc.setPlanarScannerPose(synth.SCANNER_POSE)
        pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
        pf.setResampleModel(1)  # systematic
        pf.srand48(42)
        engines.append(e)
        keep.append((m, sc))
        pfs.append(pf)
    f = LocalShardedFilter(pfs, resample_form="in_place", rebalance=rebalance)
    cuts = [(n * r) // W for r in range(W + 1)]
    f.load([samples[cuts[r]:cuts[r + 1]] for r in range(W)])
    f.for_each_rank(lambda r, pf: pf.snapshot())
    f.loaded = (list(f.counts), f.leaf_count)  # what every step starts from: both settings resample to the same M
    return engines, keep, f


def time_steps(f, data, steps):
    counts, leaf = f.loaded

    def step():
        f.for_each_rank(lambda r, pf: pf.restore())
        f.restore(counts, leaf)
        f.update_sensor(data)
        f.update_resample()
    for _ in range(5):
        step()
    for e in f.engines:
        e.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    for e in f.engines:
        e.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_rebalance.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--worlds", default="1,2,4")
    args = ap.parse_args()
    import torch  # noqa: F401 -- before the engine library
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
    size, beams, n = 2000, 1081, 100000
    cells, origin = synth.make_map(size)
    pose = synth.true_pose(size)
    ranges, angles = synth.cast_scan(cells, origin, 0.05, pose, beams, seed=5)
    wl = dict(cells=cells, origin=origin, ranges=ranges, angles=angles, beams=beams)
    e0 = bpf.Engine(0)
    m0 = bpf.OccupancyMap(e0, 0.05)
    m0.setCells(cells)
    m0.setOrigin(origin)
    m0.updateDistancesLUT(2.0)
    lut = m0.getDistancesLUT()
    e0.close()
    data = bpf.PlanarData(ranges, angles, 30.0)
    samples = synth.spread_cloud(n, size, 0.05, seed=43)
    samples[:n // 4] = synth.converged_cloud(n // 4, pose, seed=42, sigma=(0.05, 0.05, 0.02))
    samples[:, 3] = 1.0 / n
    samples = np.ascontiguousarray(samples)
    rows = []
    for W in [int(w) for w in args.worlds.split(",")]:
        row = {"world": W, "cloud": "spread, first quarter converged", "particles_total": n}
        # the two settings in turn within every repeat: same box, same minute
        worlds = {name: make_world(W, wl, samples, lut, mode) for name, mode in (("cap", "off"), ("auto", "auto"))}
        ms = {name: [] for name in worlds}
        for _ in range(args.repeats):
            for name, (_, _, f) in worlds.items():
                ms[name].append(time_steps(f, data, args.steps))
        for name, (engines, keep, f) in worlds.items():
            row[name + "_step_ms"] = statistics.median(ms[name])
            row[name + "_step_ms_min_max"] = [min(ms[name]), max(ms[name])]
            row[name + "_resampled_to"] = f.sample_count
            row[name + "_form_used"] = f.form_used
            row[name + "_largest_slice"] = max(f.counts)
            row[name + "_rebalanced"] = f.rebalanced
            f.close()
            for e in engines:
                e.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {
        "what": "in-place sharded systematic resample on a lopsided set: the imbalance cap (max_share 2.0, falls back to "
                "the window form) against BPF_SHARD_REBALANCE_AUTO (trigger_share 1.5), every rank on ONE MI355X in one "
                "process (badger_amcl_amd.local_world.LocalShardedFilter); step: restore + sensor update + resample, %d "
                "steps per run, medians of %d runs, the two settings alternating within every repeat; 2-D likelihood "
                "field, 1081 beams, 2000x2000 map, 100 k particles in all" % (args.steps, args.repeats),
        "caveats": ["ranks sharing one GPU bound launch and host cost only and say nothing about xGMI",
                    "what crosses is a byte count (rebalance: 32 B per moved sample into every rank; window: 48 B per new "
                    "sample into every rank); between two GPUs it is unmeasured",
                    "no target was fixed in advance: the cap's behaviour in the same run is the comparison",
                    "driven through Python threads, one fan-out and join per call"],
        "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
