#!/usr/bin/env python3
"""Wall time of seeding a filter of 100 000 samples from K Gaussian components, K in {1, 32, 1024}, three ways in the
same process and run:

  mixture   ParticleFilter.initWithMixture (bpf_pf_init_with_mixture): one upload of the component table, the Gaussian
            stream and the poses on the device, one read-back of the generation's result words, the tree;
  gaussian  ParticleFilter.initWithGaussian (bpf_pf_init_with_gaussian), the K = 1 yardstick: the same generation with
            one draw argument triple, the same tree.  The mixture at K = 1 should cost the same;
  host      what a caller had to do before the call existed: numpy forms the mixture on the host (its own generator,
            so not the filter's stream) and ParticleFilter.initWithSamples uploads it, 32 B per sample, then the tree
            (the leaf count is asked for, as the other two have it when they return).

Host clock around each call; every call returns after its last wait (getState after initWithSamples builds the
tree).  One untimed call of each first (allocations, code objects), then --reps timed calls interleaved way by way;
the median and the spread (min, max) are reported.  Nothing here is asserted anywhere.
Run on the GPU box: python tools/time_init_mixture.py [--reps R] [--samples N] [--out FILE]; prints one JSON line per
(K, way)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 32, 1024)
SIGMA = (0.2, 0.2, 0.05)


def components(n, k, seed=7):
    from badger_amcl_amd import pf as hpf
    rng = np.random.default_rng(seed)
    comps = np.zeros(k, dtype=hpf.MIXTURE_COMPONENT_DTYPE)
    comps["mean"] = np.stack([rng.uniform(-40, 40, k), rng.uniform(-40, 40, k), rng.uniform(-3, 3, k)], axis=1)
    comps["rotation"] = np.eye(3)
    comps["sigma"] = SIGMA
    comps["count"] = [(n * (i + 1)) // k - (n * i) // k for i in range(k)]
    return comps


def host_mixture(comps, rng):
    """the set in numpy: every sample mean + rotation * (sigma * standard normal), weight 1 / n"""
    n = int(comps["count"].sum())
    owner = np.repeat(np.arange(comps.shape[0]), comps["count"])
    s = np.empty((n, 4), dtype=np.float64)
    r = rng.standard_normal((n, 3)) * comps["sigma"][owner]
    s[:, :3] = comps["mean"][owner] + np.einsum("nij,nj->ni", comps["rotation"][owner], r)
    s[:, 3] = 1.0 / n
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import badger_amcl_amd as bpf
    n = args.samples
    e = bpf.Engine(0)
    pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
    pf.srand48(11)
    rng = np.random.default_rng(3)
    lines = []
    for k in KS:
        comps = components(n, k)
        c0 = comps[0]

        def mixture():
            pf.initWithMixture(comps)

        def gaussian():
            pf.initWithGaussian(c0["mean"], c0["rotation"], c0["sigma"])

        def host():
            pf.initWithSamples(host_mixture(comps, rng))
            pf.getState()

        ways = [("mixture", mixture), ("gaussian", gaussian), ("host", host)]
        times = {name: [] for name, _ in ways}
        for _, job in ways:
            job()
        for _ in range(args.reps):
            for name, job in ways:
                e.synchronize()
                t0 = time.perf_counter()
                job()
                times[name].append(time.perf_counter() - t0)
        for name, _ in ways:
            t = times[name]
            line = dict(way=name, k=k, samples=n, reps=args.reps, ms_median=1e3 * statistics.median(t),
                        ms_min=1e3 * min(t), ms_max=1e3 * max(t))
            print(json.dumps(line), flush=True)
            lines.append(line)
    e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
