#!/usr/bin/env python3
"""Wall time of one filter step (planar LF sensor update + updateResample + getState) with the KLD stop rule counting
tree leaves (BPF_KLD_COUNT_LEAVES, the default) and distinct bins (BPF_KLD_COUNT_BINS, bpf_pf_set_kld_count),
alternated rep by rep in one process, on the 2000 x 2000 bench map with a 1081-beam scan: the converged 100 k cloud
(the headline's), a spread 100 k cloud and a spread 1 M cloud, for both resamplers.  Every rep starts from the same
set and drand48 state.  Records ms per step, the new set's size and count, and which form the stop rule took
(bpf_pf_state.kld_on_device: 2 = one-block kernel, 1 = device long stream, 0 = host windows; kld_last_form 4 = the
BINS device pipeline).
Run on the GPU box: python tools/time_kld_count.py [--reps R] [--only NAME] [--out FILE]; prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import badger_amcl_amd as bpf  # noqa: E402
import badger_amcl_amd.pf as hpf  # noqa: E402
from badger_amcl_amd import synth  # noqa: E402

MODES = (("leaves", hpf.KLD_COUNT_LEAVES), ("bins", hpf.KLD_COUNT_BINS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="one cloud: converged_100k, spread_100k or spread_1m")
    ap.add_argument("--mode", default="both", choices=("both", "leaves", "bins"),
                    help="one mode only (a rocprofv3 run per mode)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    modes = [md for md in MODES if args.mode in ("both", md[0])]
    size, beams = 2000, 1081
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
    clouds = {"converged_100k": lambda: synth.converged_cloud(100_000, pose),
              "spread_100k": lambda: synth.spread_cloud(100_000, size, seed=43, margin=0.5),
              "spread_1m": lambda: synth.spread_cloud(1_000_000, size, seed=43, margin=0.5)}
    out = {"beams": beams, "map": size, "reps": args.reps}
    for name, make in clouds.items():
        if args.only and name != args.only:
            continue
        samples = make()
        n = samples.shape[0]
        pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
        for resampler, rname in ((0, "multinomial"), (1, "systematic")):
            pf.setResampleModel(resampler)
            t = {k: 0.0 for k, _ in modes}
            rec = {}
            for rep in range(args.reps + 1):
                for mname, mode in modes:
                    pf.setKldCount(mode)
                    pf.srand48(42)
                    pf.initWithSamples(samples)
                    pf.getState()  # (the set's count in this mode, outside the timed step)
                    t0 = time.perf_counter()
                    sc.updateSensor(pf, data)
                    pf.updateResample()
                    st = pf.getState()
                    dt = time.perf_counter() - t0
                    if rep:  # the first round warms up
                        t[mname] += dt
                    rec[mname] = dict(M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count,
                                      form=st.kld_on_device, last_form=e.kld_last_form())
            for mname, _ in modes:
                key = "%s_%s_%s" % (name, rname, mname)
                out[key + "_ms"] = t[mname] / args.reps * 1e3
                out[key] = rec[mname]
        pf.setKldCount(hpf.KLD_COUNT_LEAVES)
    e.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
