"""Inputs for map frames far from the world origin (a georeferenced or site-wide frame: an origin tens of km to a few
thousand km out), and the exact reference of the cluster statistics.  CPU only; tests/test_far_frames_cpu.py holds
these inputs to their claims from the oracle alone, the test_gpu_far_*.py files run the engine on them.

Frame offsets.  A cloud built near the origin is translated by (dx, dy):

  control    (0, 0)
  few_km     (1 800, -2 500)
  under      the exact sum of w x^2 over the set lies in (0.99 * 2^31, 2^31): the last frame the 32.96 fixed-point sums
             of kernels_stats.hpp hold
  over_xx    ... in (2^31, 1.01 * 2^31): the first one they do not
  over_xy    (-70 000, 52 000): only the cross term passes 2^31 in magnitude, and it is negative
  far        (1.0e6, -2.0e6): every single term still passes the per-term guard (|t| < 2e9) for w = 1 / n
  guard      (3.9e6, -4.1e6): w y^2 alone exceeds 2e9

`under` and `over_xx` depend on the cloud and on its weights (sum w x^2 = W (mean^2 + variance)): offset() solves for
them, and the CPU tests check the interval with exact rational sums.

Key-edge clouds.  kld_pack admits an x key in [-2^23, 2^23 - 2], a y key in [-2^23, 2^23 - 1]; the key is
floor(x / bin) with the bin size the filter's histogram uses (bin_size() reads it from the oracle's tree)."""
import math
from fractions import Fraction

import numpy as np

from badger_amcl_amd import synth

BASE_POSE = np.array([9.7, 11.2, 0.4])
TWO31 = 2 ** 31
TERM_GUARD = 2.0e9

FIXED_OFFSETS = {
    "control": (0.0, 0.0),
    "few_km": (1800.0, -2500.0),
    "over_xy": (-70000.0, 52000.0),
    "far": (1.0e6, -2.0e6),
    "guard": (3.9e6, -4.1e6),
}
OFFSETS = ["control", "few_km", "under", "over_xx", "over_xy", "far", "guard"]
WEIGHTS = ["normalised", "ones"]
CLOUDS = {"blobs5000": 5000, "blob2000": 2000, "shards6000": 6000, "blob6000": 6000}


# ------------------------------------------------------------------------------------------------ clouds
def _blobs(n, stragglers, seed):
    """Three separated blobs (tests/test_gpu_next_rows.py::test_cluster_stats_of_loaded_multimodal_set) and
    `stragglers` lone samples around them: several heavy clusters and many light ones."""
    per = (n - stragglers) // 3
    sizes = [per, per, n - stragglers - 2 * per]
    parts = [synth.converged_cloud(m, BASE_POSE + np.array(off), seed=seed + i, sigma=(0.15, 0.15, 0.05))
             for i, (m, off) in enumerate(zip(sizes, [(0, 0, 0), (4.0, -2.0, 1.0), (-3.0, 3.5, -2.0)]))]
    rng = np.random.default_rng(seed + 17)
    lone = np.zeros((stragglers, 4))
    lone[:, 0] = BASE_POSE[0] + rng.uniform(-15, 15, stragglers)
    lone[:, 1] = BASE_POSE[1] + rng.uniform(-15, 15, stragglers)
    lone[:, 2] = rng.uniform(-math.pi, math.pi, stragglers)
    s = np.concatenate(parts + [lone])
    # the stragglers mixed in among the blobs' samples: clusters are created in the order of their first sample
    return np.ascontiguousarray(s[np.random.default_rng(seed + 23).permutation(n)])


def base_cloud(name):
    """[n, 4] poses near the origin, weights not set (column 3 is filled by cloud())."""
    if name == "blobs5000":
        return _blobs(5000, 200, seed=5)
    if name == "blob2000":
        return synth.converged_cloud(2000, BASE_POSE, seed=11, sigma=(0.15, 0.15, 0.05))
    if name == "shards6000":
        return _blobs(6000, 240, seed=31)
    if name == "blob6000":  # ONE cluster that every rank holds a share of
        return synth.converged_cloud(6000, BASE_POSE, seed=37, sigma=(0.15, 0.15, 0.05))
    raise ValueError(name)


def weights(n, form):
    if form == "ones":
        return np.ones(n)
    w = np.random.default_rng(9).uniform(0.5, 1.5, n)
    return w / w.sum()


def offset(name, base, w):
    """(dx, dy) of frame `name` for the cloud `base` with weights `w`."""
    if name in FIXED_OFFSETS:
        return FIXED_OFFSETS[name]
    target = {"under": 0.995, "over_xx": 1.005}[name] * TWO31
    # sum w (x + d)^2 = W d^2 + 2 d sum(w x) + sum(w x^2) = target, the positive root
    W, sx, sxx = math.fsum(w), math.fsum(w * base[:, 0]), math.fsum(w * base[:, 0] * base[:, 0])
    d = (-sx + math.sqrt(sx * sx - W * (sxx - target))) / W
    return (float(np.round(d, 3)), -2500.0 if W <= 2.0 else -40.0)  # y stays well inside for either weight form


_CACHE = {}


def cloud(name, frame, form):
    """The cloud `name` in frame `frame` with weights of form `form`: a fresh copy of a cached array."""
    key = (name, frame, form)
    if key not in _CACHE:
        base = base_cloud(name)
        w = weights(base.shape[0], form)
        dx, dy = offset(frame, base, w)
        s = base.copy()
        s[:, 0] += dx
        s[:, 1] += dy
        s[:, 3] = w
        _CACHE[key] = np.ascontiguousarray(s)
    return _CACHE[key].copy()


def converged_far(n, frame, seed=42):
    """A converged cloud (weights 1 / n) in a fixed frame, for the resample and convergence tests."""
    dx, dy = FIXED_OFFSETS[frame]
    s = synth.converged_cloud(n, BASE_POSE, seed=seed)
    s[:, 0] += dx
    s[:, 1] += dy
    return np.ascontiguousarray(s)


# ------------------------------------------------------------------------------------------------ exact sums
def terms(samples):
    """The nine weighted terms of every sample, formed as the kernels form them (kernels_stats.hpp, from
    particle_filter.cpp:577-600), in float64: [9, n]."""
    x, y, th, w = (np.ascontiguousarray(samples[:, k], dtype=np.float64) for k in range(4))
    wx, wy = w * x, w * y
    return np.stack([w, wx, wy, w * np.cos(th), w * np.sin(th), wx * x, wx * y, wy * x, wy * y])


def exact_sum(values):
    """The sum of float64 values as an exact Fraction (integers over one power-of-two denominator)."""
    total, shift = 0, 1200  # 2^-1200 is below the last bit of any double
    for v in values:
        num, den = float(v).as_integer_ratio()  # den is a power of two
        total += num * ((1 << shift) // den)
    return Fraction(total, 1 << shift)


def _moments(m):
    """normalizeCluster / computeSetStats (particle_filter.cpp:541-567, 607-635) in plain float64, the expressions of
    stats_moments (kernels_stats.hpp)."""
    W = m[0]
    mean = [m[1] / W, m[2] / W, math.atan2(m[4], m[3])]
    cov = [m[5] / W - mean[0] * mean[0], m[6] / W - mean[0] * mean[1], m[7] / W - mean[1] * mean[0],
           m[8] / W - mean[1] * mean[1], -2 * math.log(math.sqrt(m[3] * m[3] + m[4] * m[4]))]
    return mean, cov


def exact_stats(samples, labels):
    """The ten sums per cluster and for the whole set, each the EXACT sum of its float64 terms rounded once to double;
    then the moments in float64.  labels[i] = cluster index of sample i (the oracle's tree).  Same dict as
    pyoracle.KDTree.cluster_stats, plus "sums" (the exact Fractions of the whole set) and "largest" (the largest
    magnitude among all sums, per cluster and whole set, and all single terms: what has to fit the fixed-point format)."""
    t = terms(samples)
    labels = np.asarray(labels)
    n = int(labels.max()) + 1 if labels.size else 0
    out = dict(n=n, count=np.zeros(n, dtype=np.int32), weight=np.zeros(n), mean=np.zeros((n, 3)),
               cov=np.zeros((n, 5)))
    total = [Fraction(0)] * 9
    largest = Fraction(float(np.max(np.abs(t)))) if t.size else Fraction(0)
    for c in range(n):
        idx = np.flatnonzero(labels == c)
        sums = [exact_sum(t[k, idx]) for k in range(9)]
        total = [a + b for a, b in zip(total, sums)]
        largest = max([largest] + [abs(v) for v in sums])
        mean, cov = _moments([float(v) for v in sums])
        out["count"][c] = idx.size
        out["weight"][c] = float(sums[0])
        out["mean"][c] = mean
        out["cov"][c] = cov
    mean, cov = _moments([float(v) for v in total])
    out["set_mean"], out["set_cov"], out["sums"] = np.array(mean), np.array(cov), total
    out["largest"] = max([largest] + [abs(v) for v in total])
    return out


def oracle_tree(orc, samples):
    t = orc.KDTree()
    for k in range(samples.shape[0]):
        t.insert_pose(samples[k, :3], samples[k, 3])
    return t


def oracle_labels(orc, samples):
    """The cluster index of every sample from the oracle's tree (PFKDTree::cluster / getCluster)."""
    t = oracle_tree(orc, samples)
    t.cluster()
    return np.array([t.get_cluster(samples[k, :3]) for k in range(samples.shape[0])])


def oracle_stats(orc, samples):
    return oracle_tree(orc, samples).cluster_stats(samples, samples.shape[0])


_REF = {}


def reference(orc, name, frame, form):
    """(samples, oracle's serial statistics, exact statistics) of one case, computed once and shared."""
    key = (name, frame, form)
    if key not in _REF:
        s = cloud(name, frame, form)
        _REF[key] = (s, oracle_stats(orc, s), exact_stats(s, oracle_labels(orc, s)))
    s, want, exact = _REF[key]
    return s.copy(), want, exact


def fits_fixed_point(samples, exact):
    """Every term is below the per-term guard and every sum, per cluster and for the set, below 2^31: the device
    evaluation can hold this case.  (Sums of one sign only, as here away from the axes: no partial sum is larger.)"""
    return bool(np.all(np.abs(terms(samples)) < TERM_GUARD)) and exact["largest"] < TWO31


def cov_scale(samples):
    """max(x^2, y^2) over the set: what a covariance's rounding is measured in."""
    return float(max(np.max(samples[:, 0] ** 2), np.max(samples[:, 1] ** 2)))


# ------------------------------------------------------------------------------------------------ key edges
_BIN = {}


def bin_size(orc):
    """The x / y bin size of the filter's histogram, read from the oracle's tree: the smallest multiple of 1/64 m at
    which a second pose falls into a second bin (node_count counts the distinct bins; the reference's leaf counter is
    not that)."""
    if "b" not in _BIN:
        for k in range(1, 64 * 8):
            t = orc.KDTree()
            t.insert_pose((0.0, 0.0, 0.0))
            t.insert_pose((k / 64.0, 0.0, 0.0))
            if t.node_count() == 2:
                _BIN["b"] = k / 64.0
                break
    return _BIN["b"]


KEY_MIN = {"x": -(1 << 23), "y": -(1 << 23)}
KEY_MAX = {"x": (1 << 23) - 2, "y": (1 << 23) - 1}
EDGE_CLOUDS = ["mid", "inside+x", "inside-x", "inside+y", "inside-y", "straddle+x", "straddle-x", "straddle+y",
               "straddle-y"]


def keys_of(samples, b):
    """floor(x / bin), floor(y / bin) as int64 (kdhist.hpp host_pose_key; pf_kdtree.cpp:49-56)."""
    return np.floor(samples[:, 0] / b).astype(np.int64), np.floor(samples[:, 1] / b).astype(np.int64)


def packs(samples, b):
    kx, ky = keys_of(samples, b)
    return (kx >= KEY_MIN["x"]) & (kx <= KEY_MAX["x"]) & (ky >= KEY_MIN["y"]) & (ky <= KEY_MAX["y"])


def edge_cloud(name, n, b, seed=3, spread=10.0):
    """n poses, weights 1 / n, headings of a converged cloud; the cloud reaches over 2 * spread metres but most of it
    lies within a few metres (some hundred occupied bins, which the one-block resample kernels still take):
    inside<s><axis>    hugs the end of the admitted key range on that axis from inside: the distance from the edge is
                       half-normal (sigma 2 m); sample 0 sits in the last admitted bin, sample 1 2 * spread further in
    straddle<s><axis>  centred on that edge (sigma 2 m): about half of the samples do not pack
    mid                keys around +2^22 (x) and -2^22 (y)"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    s[:, 2] = 0.4 + rng.normal(0, 0.1, n)
    s[:, 3] = 1.0 / n
    pos = np.clip(rng.normal(0, 1.0, (n, 2)), -spread, spread)
    if name == "mid":
        pos += [(1 << 22) * b, -(1 << 22) * b]
    else:
        kind, sign, axis = name[:-2], name[-2], name[-1]
        a = "xy".index(axis)
        up = sign == "+"
        edge = (KEY_MAX[axis] + 1) * b if up else KEY_MIN[axis] * b  # where the admitted range ends
        if kind == "straddle":
            pos[:, a] = edge + np.clip(rng.normal(0, 2.0, n), -spread, spread)
        else:
            d = np.minimum(np.abs(rng.normal(0, 2.0, n)), 2 * spread - b)
            d[0], d[1] = b / 2, 2 * spread - b / 2
            # rounding must not carry a sample across the edge
            pos[:, a] = np.minimum(edge - d, np.nextafter(edge, -np.inf)) if up else np.maximum(edge + d, edge)
    s[:, 0] = pos[:, 0]
    s[:, 1] = pos[:, 1]
    return np.ascontiguousarray(s)
