"""Randomised differential soak of computeClusterStatsForSet / getMaxWeightPose on the device against the oracle:
random clouds (one blob, many blobs, spread, mixtures), sizes on both sides of the single-block kernel's limit (4 096
samples, 64 clusters), random weights.  Labels, counts and the heaviest cluster exact, sums within 1e-12 (the checks
of tests/test_gpu_next_rows.py::_assert_stats_equal).  A fifth of the cases sit in a map frame far from the origin
(each axis log-uniform in 10^3 .. 4 10^6 m, random sign), where the fixed-point sums may leave their format: there the
answer is the host evaluation's (the oracle's bits) or within n 2^-53 max(x^2, y^2) of the oracle on the covariances
(tests/test_gpu_far_stats.py).
usage: python tools/soak_stats.py [cases] [seed]"""
import os
import sys
import time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import badger_amcl_amd as bpf
from oracle import pyoracle as orc
from test_gpu_next_rows import _assert_stats_equal, _oracle_stats
from test_gpu_shard_stats import read_stats


def _assert_far_stats(pf, want, s):
    """Counts, labels and the heaviest cluster exact; the figures the oracle's bits (host evaluation) or within the
    magnitude-scaled bound of the device evaluation."""
    got = read_stats(pf)
    n, scale = s.shape[0], float(max(np.max(s[:, 0] ** 2), np.max(s[:, 1] ** 2)))
    assert int(got["n"][0]) == want["n"] and np.array_equal(got["count"], want["count"])
    same = (np.array_equal(got["weight"], want["weight"]) and np.array_equal(got["mean"], want["mean"]) and
            np.array_equal(got["cov"], want["cov"], equal_nan=True) and
            np.array_equal(got["set_cov"], want["set_cov"], equal_nan=True))
    if same:
        return
    tol = n * 2.0 ** -53 * scale
    assert np.allclose(got["weight"], want["weight"], rtol=1e-12, atol=0)
    assert np.allclose(got["mean"][:, :2], want["mean"][:, :2], rtol=1e-12, atol=0)
    assert np.allclose(got["mean"][:, 2], want["mean"][:, 2], rtol=0, atol=1e-12)
    assert np.all(np.abs(got["cov"][:, :4] - want["cov"][:, :4]) <= tol)
    assert np.allclose(got["cov"][:, 4], want["cov"][:, 4], rtol=0, atol=1e-10, equal_nan=True)
    assert np.all(np.abs(got["set_cov"][:4] - want["set_cov"][:4]) <= max(tol, 1e-9))
    assert np.allclose(got["set_mean"][:2], want["set_mean"][:2], rtol=1e-12, atol=0)

def run(cases=100, seed=1, e=None, quiet=False):
    """Returns the number of mismatching cases."""
    rng = np.random.default_rng(seed)
    own = e is None
    if own:
        e = bpf.Engine(0)
    t0 = time.time()
    bad = 0
    for case in range(cases):
        n = int(rng.choice([1, 2, 50, 1000, 4095, 4096, 4097, 9000, 30000]))
        kind = str(rng.choice(["blob", "blobs", "spread", "mix"]))
        s = np.zeros((n, 4))
        if kind == "blob":
            s[:, 0] = rng.normal(10, 0.3, n); s[:, 1] = rng.normal(5, 0.3, n); s[:, 2] = rng.normal(0.4, 0.1, n)
        elif kind == "blobs":
            k = int(rng.integers(2, 120))
            c = rng.uniform(0, 40, (k, 2)); th = rng.uniform(-3.1, 3.1, k); w = rng.integers(0, k, n)
            s[:, :2] = c[w] + rng.normal(0, 0.2, (n, 2)); s[:, 2] = th[w] + rng.normal(0, 0.05, n)
        elif kind == "spread":
            s[:, 0] = rng.uniform(0, 20, n); s[:, 1] = rng.uniform(0, 20, n); s[:, 2] = rng.uniform(-3.1, 3.1, n)
        else:
            h = n // 2
            s[:h, 0] = rng.normal(10, 0.3, h); s[:h, 1] = rng.normal(5, 0.3, h); s[:h, 2] = rng.normal(0.4, 0.1, h)
            s[h:, 0] = rng.uniform(0, 20, n - h); s[h:, 1] = rng.uniform(0, 20, n - h); s[h:, 2] = rng.uniform(-3.1, 3.1, n - h)
            s[:] = s[rng.permutation(n)]
        w = rng.uniform(0.01, 1.0, n)
        s[:, 3] = w / w.sum()
        far = rng.random() < 0.2
        if far:
            off = 10.0 ** rng.uniform(3.0, np.log10(4.0e6), 2) * rng.choice([-1.0, 1.0], 2)
            s[:, :2] += off
            kind += " far (%.3g, %.3g)" % (off[0], off[1])
        pf = bpf.ParticleFilter(e, 1, n, 0.0, 0.0, 85.0)
        pf.initWithSamples(s)
        try:
            if far:
                _assert_far_stats(pf, _oracle_stats(orc, s, n), s)
            else:
                _assert_stats_equal(pf, _oracle_stats(orc, s, n), exact=False, set_atol=1e-9)
        except AssertionError as ex:
            bad += 1
            print("MISMATCH case %d: n %d kind %s: %s" % (case, n, kind, str(ex).splitlines()[0][:200]), flush=True)
        if case % 20 == 19:
            print("%d cases, %d mismatching, %.0f s" % (case + 1, bad, time.time() - t0), flush=True)
    print("%d cases, %d mismatching, %.0f s" % (cases, bad, time.time() - t0))
    if own:
        e.close()
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 100,
                      int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
