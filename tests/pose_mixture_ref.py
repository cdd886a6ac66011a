"""The rule of bpf_pose_mixture_from_hits (include/badger_pf.h) in numpy: the definition the library is tested against.

Every number that reaches the output is formed by one IEEE operation at a time in double (Python floats), and
normalize_angle is the fmod form (math.fmod is C's fmod, which is exact), so the C code agrees bit for bit."""
import math

import numpy as np

COMPONENT_DTYPE = np.dtype([("mean", "<f8", (3,)), ("rotation", "<f8", (3, 3)), ("sigma", "<f8", (3,)),
                            ("count", "<i4"), ("reserved", "<i4")])
MAX_ROWS = 1024


def normalize_angle(a):
    """angles::normalize_angle, Noetic form: fmod(a + pi, 2 pi), then <= 0 ? + pi : - pi."""
    r = math.fmod(a + math.pi, 2.0 * math.pi)
    return r + math.pi if r <= 0.0 else r - math.pi


def largest_remainder(weights, total_count):
    """Counts of total_count samples shared out by weight: floor of the quota, the rest by remainder descending."""
    K = len(weights)
    W = 0.0
    for w in weights:
        W += w
    t = [(float(total_count) * w) / W for w in weights]
    c = [int(math.floor(v)) for v in t]
    order = sorted(range(K), key=lambda k: (-(t[k] - float(c[k])), k))
    given, at = sum(c), 0
    while given < total_count:
        c[order[at]] += 1
        given += 1
        at = (at + 1) % K
    at = K - 1
    while given > total_count:  # (rounding only; never seen)
        if c[order[at]] > 0:
            c[order[at]] -= 1
            given -= 1
        at = (at + K - 1) % K
    return c


def mixture_from_hits(poses, scores, total_count, xy_merge, theta_merge, max_components, sigma):
    """(components, source_row, merged) or None where the library refuses."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    sigma = [float(v) for v in sigma]
    n = poses.shape[0]
    if not (1 <= n <= MAX_ROWS and 1 <= max_components <= MAX_ROWS and total_count >= 1):
        return None
    if any(not (math.isfinite(v) and v >= 0.0) for v in [xy_merge, theta_merge] + sigma):
        return None
    usable = [r for r in range(n) if np.all(np.isfinite(poses[r])) and math.isfinite(scores[r]) and scores[r] > 0.0]
    if not usable:
        return None
    usable.sort(key=lambda r: (-scores[r], r))
    kept, merged = [], []
    for r in usable:
        x, y, th = (float(v) for v in poses[r])
        by = None
        for c, q in enumerate(kept):
            if (abs(x - float(poses[q, 0])) <= xy_merge and abs(y - float(poses[q, 1])) <= xy_merge and
                    abs(normalize_angle(th - float(poses[q, 2]))) <= theta_merge):
                by = c
                break
        if by is not None:
            merged[by] += 1
        elif len(kept) < max_components:
            kept.append(r)
            merged.append(0)
    counts = largest_remainder([float(scores[r]) for r in kept], total_count)
    comps = np.zeros(len(kept), dtype=COMPONENT_DTYPE)
    for k, r in enumerate(kept):
        comps[k]["mean"] = (poses[r, 0], poses[r, 1], normalize_angle(float(poses[r, 2])))
        comps[k]["rotation"] = np.eye(3)
        comps[k]["sigma"] = sigma
        comps[k]["count"] = counts[k]
    return comps, np.array(kept, dtype=np.int32), np.array(merged, dtype=np.int32)
