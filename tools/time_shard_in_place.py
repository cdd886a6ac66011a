"""Times the two forms of the sharded resample -- the draw window and the resample in place (include/badger_pf.h,
bpf_shard_set_resample_form for the systematic resampler, bpf_shard_set_multinomial_form for the multinomial one:
--resampler) -- back to back, on ONE GPU:

  step   restore, sensor update, resample of ONE filter of 100 k particles x 1081 beams on the 2000 x 2000 map
         (bench.py's headline workload with the resampler asked for), split evenly over W = 1, 2, 4 ranks in this process
         (badger_amcl_amd.local_world.LocalShardedFilter), for a converged and a spread cloud

Medians over --repeats runs, with the spread of the runs beside them, written to profiles/shard_in_place.json
(--resampler multinomial: profiles/shard_in_place_multinomial.json).  With
every rank on one GPU the numbers bound the launch and host cost of the two protocols only.  What the in-place form is
for -- 48 B per new sample into every rank that no longer cross -- costs nothing here: nothing has run between two
GPUs, and that figure stays unmeasured.

usage: python tools/time_shard_in_place.py [--resampler systematic|multinomial] [--out FILE] [--repeats 5] [--steps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_world(W, wl, samples, lut, form, resampler="systematic"):
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
        pf.setResampleModel(1 if resampler == "systematic" else 0)
        pf.srand48(42)
        engines.append(e)
        keep.append((m, sc))
        pfs.append(pf)
    f = LocalShardedFilter(pfs, **{"resample_form" if resampler == "systematic" else "multinomial_form": form})
    cuts = [(n * r) // W for r in range(W + 1)]
    f.load([samples[cuts[r]:cuts[r + 1]] for r in range(W)])
    f.for_each_rank(lambda r, pf: pf.snapshot())
    f.loaded = (list(f.counts), f.leaf_count)  # what every step starts from: both forms resample to the same M
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
    ap.add_argument("--resampler", choices=("systematic", "multinomial"), default="systematic")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--worlds", default="1,2,4")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "shard_in_place.json" if args.resampler == "systematic"
                                else "shard_in_place_multinomial.json")
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
    clouds = {"converged": synth.converged_cloud(n, pose, seed=42), "spread": synth.spread_cloud(n, size, 0.05, seed=43)}
    rows = []
    for W in [int(w) for w in args.worlds.split(",")]:
        for cloud, samples in clouds.items():
            row = {"world": W, "cloud": cloud, "particles_total": n}
            # the two forms in turn within every repeat: same box, same minute
            worlds = {form: make_world(W, wl, np.ascontiguousarray(samples), lut, form, args.resampler)
                      for form in ("window", "in_place")}
            ms = {form: [] for form in worlds}
            for _ in range(args.repeats):
                for form, (_, _, f) in worlds.items():
                    ms[form].append(time_steps(f, data, args.steps))
            for form, (engines, keep, f) in worlds.items():
                row[form + "_step_ms"] = statistics.median(ms[form])
                row[form + "_step_ms_min_max"] = [min(ms[form]), max(ms[form])]
                row[form + "_resampled_to"] = f.sample_count
                row[form + "_form_used"] = f.form_used
                row[form + "_largest_slice"] = max(f.counts)
                f.close()
                for e in engines:
                    e.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {
        "what": "sharded %s resample, draw window against in place (%s, max_share 2.0), " % (
                    args.resampler, "bpf_shard_set_resample_form" if args.resampler == "systematic"
                    else "bpf_shard_set_multinomial_form") +
                "every rank on ONE MI355X in one process (badger_amcl_amd.local_world.LocalShardedFilter); step: restore "
                "+ sensor update + resample, %d steps per run, medians of %d runs, the two forms alternating within every "
                "repeat; 2-D likelihood field, 1081 beams, 2000x2000 map, 100 k particles in all" %
                (args.steps, args.repeats),
        "caveats": ["ranks sharing one GPU bound launch and host cost only and say nothing about xGMI",
                    "the in-place form's benefit is a byte and operation count (no 48 B per new sample into every rank, no "
                    "M-key tree on every rank); between two GPUs it is unmeasured",
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
