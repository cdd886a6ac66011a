"""Times the in-process sharded filter (bpf_shard_connect_local, badger_amcl_amd/local_world.py) on ONE GPU:

  totals     one f64 all-gather of one word per rank (the W weight totals)           bpf_shard_exchange_probe kind 0
  window     one int64 all-reduce of 6 x 4096 words (a draw window)                  bpf_shard_exchange_probe kind 1
  step       a whole sharded step -- restore, sensor update, resample -- of ONE filter of 100 k particles x 1081 beams
             on the 2000 x 2000 map (bench.py's headline workload), split evenly over the ranks; and, at W = 2, of
             100 k particles PER RANK, the layout of profiles/r03_bench_rehearsal_2ranks_1gpu.json

at W = 1, 2, 4 and 8, medians over --repeats runs, written to profiles/local_world.json beside the parent's figures.
With every rank on one GPU the numbers bound the launch and host cost of the protocol only (events, two host barriers,
one launch per rank); they say nothing about xGMI, and the path between devices (peer access) is not exercised.

usage: python tools/time_local_world.py [--out profiles/local_world.json] [--repeats 7] [--steps 40]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT = {
    "single_engine_ms_per_step": ("profiles/r03_bench_cfg2_lf_converged.json", "ms_per_step"),
    "two_processes_mailbox_100k_per_rank_ms_per_step": ("profiles/r03_bench_rehearsal_2ranks_1gpu.json", "ms_per_step"),
    "four_processes_mailbox_100k_per_rank_ms_per_step": ("profiles/r03_bench_rehearsal_4ranks_1gpu.json", "ms_per_step"),
}


def parent_figures():
    out = {}
    for name, (path, key) in PARENT.items():
        with open(os.path.join(ROOT, path)) as f:
            out[name] = {"value": json.loads(f.readline())[key], "from": path}
    return out


def make_world(W, wl, samples, lut):
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
        pf.srand48(42)
        engines.append(e)
        keep.append((m, sc))
        pfs.append(pf)
    f = LocalShardedFilter(pfs)
    cuts = [(n * r) // W for r in range(W + 1)]
    f.load([samples[cuts[r]:cuts[r + 1]] for r in range(W)])
    f.for_each_rank(lambda r, pf: pf.snapshot())
    return engines, keep, f


def probe(f, kind, words, reps):
    got = [None] * f.world

    def call(r, h, lib):
        ms = C.c_double()
        rc = lib.bpf_shard_exchange_probe(h, kind, words, reps, C.byref(ms))
        got[r] = ms.value
        return rc
    f._collective(call)
    return max(got)


def time_steps(f, data, steps):
    counts, leaf = list(f.counts), f.leaf_count

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
    return (time.perf_counter() - t0) * 1e3 / steps, f.sample_count


def time_single(wl, samples, lut, steps, repeats):
    """The same step on one plain engine, from this process (Python's call overhead included, as for the worlds)."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd import synth
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
    pf = bpf.ParticleFilter(e, 100, samples.shape[0], 0.0, 0.0, 85.0)
    pf.srand48(42)
    pf.initWithSamples(samples)
    pf.snapshot()
    data = bpf.PlanarData(wl["ranges"], wl["angles"], 30.0)
    out = []
    for _ in range(repeats):
        for _ in range(5):
            pf.restore(), sc.updateSensor(pf, data), pf.updateResample()
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pf.restore(), sc.updateSensor(pf, data), pf.updateResample()
        e.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    e.close()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_world.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--probe-reps", type=int, default=200)
    ap.add_argument("--worlds", default="1,2,4,8")
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
    one = synth.converged_cloud(n, pose, seed=42)
    rows = []
    for W in [int(w) for w in args.worlds.split(",")]:
        layouts = [("100k_total", one)]
        if W == 2:
            layouts.append(("100k_per_rank", np.ascontiguousarray(np.concatenate(
                [synth.converged_cloud(n, pose, seed=42 + r) for r in range(W)]))))
        for name, samples in layouts:
            engines, keep, f = make_world(W, wl, samples, lut)
            row = {"world": W, "layout": name, "particles_total": int(samples.shape[0])}
            if name == "100k_total":
                row["totals_allgather_ms"] = statistics.median(probe(f, 0, 1, args.probe_reps) for _ in range(args.repeats))
                row["window_allreduce_6x4096_ms"] = statistics.median(
                    probe(f, 1, 6 * 4096, args.probe_reps) for _ in range(args.repeats))
            ms = [time_steps(f, data, args.steps) for _ in range(args.repeats)]
            row["step_ms"] = statistics.median(v for v, _ in ms)
            row["step_ms_min_max"] = [min(v for v, _ in ms), max(v for v, _ in ms)]
            row["resampled_to"] = ms[-1][1]
            rows.append(row)
            print(json.dumps(row), flush=True)
            f.close()
            for e in engines:
                e.close()
    result = {
        "what": "in-process sharded filter (bpf_shard_connect_local), every rank on ONE MI355X, driven from Python "
                "threads (badger_amcl_amd.local_world.LocalShardedFilter); medians of %d runs; exchanges: host wall time "
                "per exchange over %d back-to-back exchanges between two stream synchronisations, max over the ranks; "
                "step: restore + sensor update + resample, %d steps per run, 2-D likelihood field, 1081 beams, "
                "2000x2000 map, converged cloud, multinomial" % (args.repeats, args.probe_reps, args.steps),
        "caveats": ["ranks sharing one GPU bound launch and host cost only and say nothing about xGMI",
                    "the multi-device path (peer access between the engines' devices) is unverified on hardware",
                    "the parent's figures are bench.py runs (C-level step loop per process, 300 / 20 steps); these go "
                    "through Python threads, one fan-out and join per call"],
        "single_engine_same_driver_ms_per_step": time_single(wl, one, lut, args.steps, args.repeats),
        "parent": parent_figures(),
        "rows": rows,
    }
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
