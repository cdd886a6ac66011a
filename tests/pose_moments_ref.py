"""numpy model of the pose moments (bpf_planar_pose_moments / bpf_cloud_pose_moments) and of the host step from moments
to mixture components (bpf_pose_mixture_apply_moments): the weights, the ten sums in the kernel's fixed order, the
rows, the cyclic Jacobi step.  The lattice and its poses are pose_refine_ref's.  Shared by
tests/test_pose_moments_cpu.py and tests/test_gpu_pose_moments.py, together with the corridor / corner scenarios whose
oracle-only moments both files use."""
import math

import numpy as np

import pose_refine_ref as prr
from pose_mixture_ref import COMPONENT_DTYPE, normalize_angle

MOMENTS_DTYPE = np.dtype([("mean", "<f8", (3,)), ("cov", "<f8", (6,)), ("weight_sum", "<f8"), ("score_max", "<f8"),
                          ("support", "<i4"), ("flags", "<i4")])
VALID, FACE_X, FACE_Y, FACE_T = 1, 2, 4, 8
THREADS, WAVE = 256, 64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # cov: xx, xy, xt, yy, yt, tt
MAX_ROWS = 1024


# ------------------------------------------------------------------------------------------------ weights and sums
def weights(scores, baseline):
    """(w[M], s_max): s_max the largest score with NaN below every number (NaN when there is none); w = s - thr where
    s > thr = baseline * s_max, else 0 (a NaN score: 0)"""
    s = np.asarray(scores, dtype=np.float64)
    ok = ~np.isnan(s)
    if not ok.any():
        return np.zeros_like(s), float("nan")
    s_max = np.float64(np.max(s[ok]))
    thr = np.float64(baseline) * s_max
    with np.errstate(invalid="ignore"):
        above = s > thr
        w = np.where(above, s - thr, 0.0)
    return w, float(s_max)


def terms(w, R, A):
    """[10, M]: the terms of W, Sa, Sb, St, Saa, Sab, Sat, Sbb, Sbt, Stt, each product rounded as written:
    w, w*du, (w*du)*dv"""
    d = [v.astype(np.float64) for v in prr.offsets(R, A)]
    first = [w * d[u] for u in range(3)]
    return np.stack([w] + first + [first[u] * d[v] for u, v in PAIRS])


def fixed_order_sum(t):
    """the kernel's sum of t[..., M]: 256 partials (partial p adds t[p], t[p + 256], ... ascending from 0.0), the xor
    butterfly v = v + v[lane ^ off] for off = 32 .. 1 inside each 64 partials, then the four results in order"""
    t = np.asarray(t, dtype=np.float64)
    M = t.shape[-1]
    rounds = -(-M // THREADS)
    pad = np.zeros(t.shape[:-1] + (rounds * THREADS,), dtype=np.float64)
    pad[..., :M] = t
    v = np.zeros(t.shape[:-1] + (THREADS,), dtype=np.float64)
    for j in range(rounds):
        v = v + pad[..., j * THREADS:(j + 1) * THREADS]
    idx = np.arange(THREADS)
    off = WAVE // 2
    while off > 0:
        v = v + v[..., idx ^ off]
        off >>= 1
    total = v[..., 0]
    for wave in range(1, THREADS // WAVE):
        total = total + v[..., wave * WAVE]
    return total


def moments_row(pose, scores, R, A, xy_step, theta_step, baseline):
    """one MOMENTS_DTYPE row from the M scores of the lattice around `pose`"""
    row = np.zeros((), dtype=MOMENTS_DTYPE)
    c = np.asarray(pose, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64)
    M, mc = prr.lattice(R, A)
    assert s.shape == (M,)
    w, s_max = weights(s, baseline)
    row["mean"] = c
    row["score_max"] = s_max
    if not s_max > 0.0:
        return row
    d, q = prr.steps(xy_step, theta_step, R, A, 0)
    step = (np.float64(d), np.float64(d), np.float64(q))
    with np.errstate(invalid="ignore", over="ignore"):
        S = fixed_order_sum(terms(w, R, A))
        W = S[0]
        m = [S[1 + u] / W for u in range(3)]
        row["mean"] = [c[u] + m[u] * step[u] for u in range(3)]
        row["cov"] = [((S[4 + k] / W - m[u] * m[v]) * step[u]) * step[v] for k, (u, v) in enumerate(PAIRS)]
    row["weight_sum"] = W
    row["support"] = int(np.count_nonzero(w > 0.0))
    best = prr.choose(s, mc)
    da, db, dt = (int(v[best]) for v in prr.offsets(R, A))
    flags = VALID
    if R > 0 and abs(da) == R:
        flags |= FACE_X
    if R > 0 and abs(db) == R:
        flags |= FACE_Y
    if A > 0 and abs(dt) == A:
        flags |= FACE_T
    row["flags"] = flags
    return row


def moments(poses, scores, R, A, xy_step, theta_step, baseline):
    """MOMENTS_DTYPE[n] from poses[n, 3] and scores[n, M]"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    scores = np.asarray(scores, dtype=np.float64).reshape(poses.shape[0], -1)
    return np.array([moments_row(p, s, R, A, xy_step, theta_step, baseline) for p, s in zip(poses, scores)],
                    dtype=MOMENTS_DTYPE)


def offset_moments(row, pose, R, A, xy_step, theta_step):
    """(mean offsets[3], cov[6]) of a valid row in units of the lattice's offsets (an axis without a radius: 0)"""
    d, q = prr.steps(xy_step, theta_step, R, A, 0)
    step = np.array([d, d, q])
    safe = np.where(step > 0.0, step, 1.0)
    m = np.where(step > 0.0, (row["mean"] - np.asarray(pose, dtype=np.float64)) / safe, 0.0)
    c = np.array([row["cov"][k] / (safe[u] * safe[v]) if step[u] > 0.0 and step[v] > 0.0 else 0.0
                  for k, (u, v) in enumerate(PAIRS)])
    return m, c


# ------------------------------------------------------------------------------------------------ moments to components
def jacobi(cov6):
    """(lambda[3], V[3, 3]): cyclic Jacobi on the symmetric matrix of cov6 = (xx, xy, xt, yy, yt, tt): pairs (0, 1),
    (0, 2), (1, 2), a rotation skipped at an exactly zero off-diagonal entry, at most 8 sweeps; the eigenvectors are
    V's columns and the eigenvalues stay in diagonal order.  Only + - * / and sqrt on float64 scalars."""
    f = np.float64
    a = np.zeros((3, 3), dtype=np.float64)
    for k, (u, v) in enumerate(PAIRS):
        a[u, v] = a[v, u] = cov6[k]
    V = np.eye(3, dtype=np.float64)
    one, two = f(1.0), f(2.0)
    for _ in range(8):
        if a[0, 1] == 0.0 and a[0, 2] == 0.0 and a[1, 2] == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = f(a[p, q])
            if apq == 0.0:
                continue
            with np.errstate(over="ignore"):
                tau = (a[q, q] - a[p, p]) / (two * apq)
                at = -tau if tau < 0.0 else tau
                mag = one / (at + np.sqrt(tau * tau + one))
            t = -mag if tau < 0.0 else mag
            c = one / np.sqrt(t * t + one)
            s = t * c
            app, aqq, arp, arq = f(a[p, p]), f(a[q, q]), f(a[r, p]), f(a[r, q])
            a[p, p] = app - t * apq
            a[q, q] = aqq + t * apq
            a[p, q] = a[q, p] = 0.0
            a[r, p] = a[p, r] = c * arp - s * arq
            a[r, q] = a[q, r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = f(V[k, p]), f(V[k, q])
                V[k, p] = c * vkp - s * vkq
                V[k, q] = s * vkp + c * vkq
    return np.array([a[0, 0], a[1, 1], a[2, 2]]), V


def apply_moments(comps, source_row, rows, sigma_floor, sigma_cap, take_mean):
    """the components after bpf_pose_mixture_apply_moments, or None where the library refuses"""
    comps = np.array(comps, dtype=COMPONENT_DTYPE).reshape(-1)
    src = np.asarray(source_row).reshape(-1)
    rows = np.asarray(rows, dtype=MOMENTS_DTYPE).reshape(-1)
    lo, hi = np.asarray(sigma_floor, dtype=np.float64), np.asarray(sigma_cap, dtype=np.float64)
    if not (1 <= comps.shape[0] <= MAX_ROWS and 1 <= rows.shape[0] <= MAX_ROWS):
        return None
    if np.any(src < 0) or np.any(src >= rows.shape[0]):
        return None
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo >= 0.0) and np.all(hi >= lo)):
        return None
    valid = (rows["flags"] & VALID) != 0
    if not np.all(np.isfinite(rows["cov"][valid])):
        return None
    for k in range(comps.shape[0]):
        row = rows[src[k]]
        if not row["flags"] & VALID:
            continue
        lam, V = jacobi(row["cov"])
        for i in range(3):
            axis = 0
            for j in (1, 2):
                if abs(V[j, i]) > abs(V[axis, i]):
                    axis = j
            low, high = lo[axis] * lo[axis], hi[axis] * hi[axis]
            v = lam[i]
            if not v >= low:
                v = low
            if v > high:
                v = high
            comps[k]["sigma"][i] = np.sqrt(v)
        comps[k]["rotation"] = V
        if take_mean:
            comps[k]["mean"] = (row["mean"][0], row["mean"][1], normalize_angle(float(row["mean"][2])))
    return comps


# ------------------------------------------------------------------------------------------------ corridor and corner
# Oracle-only scenarios: a scan cast at `pose` on a 200 x 120 map, restricted to beams that end on the walls named.
# The lattice is laid around `hit`, the pose a search at cell stride 2 would hand on: one cell off the casting pose
# across the corridor.  The best point is then one step off the centre in y, and among the equal scores along a flat
# direction the order rule takes the smallest m: the outer face.  (Around the casting pose itself the centre would tie
# with every point along x and win.)
SCENE_SIZE = (200, 120)
SCENE_RES = 0.05
SCENE_LATTICE = (3, 0.05, 2, 0.01)  # xy_radius, xy_step, theta_radius, theta_step
SCENE_BASELINE = 0.5
SCENE_BEAMS = 61


class Scene:
    """cells, the oracle's map and LUT, the pose, and a scan of SCENE_BEAMS beams cast from the pose (the scanner at
    the robot's origin).  corridor: two walls along x at j = 40 and j = 80, beams within 50 degrees of +-y, so that
    every beam ends on one of the two walls far from the map's ends.  corner: the corridor's lower wall and a wall along
    y at i = 130, beams from -100 to +10 degrees: both walls are seen."""

    def __init__(self, orc, kind):
        from badger_amcl_amd import synth
        sx, sy = SCENE_SIZE
        self.orc, self.kind, self.res = orc, kind, SCENE_RES
        cells = np.full((sy, sx), -1, dtype=np.int32)
        cells[40, :] = 1
        if kind == "corridor":
            cells[80, :] = 1
        else:
            cells[:, 130] = 1
        self.cells = cells
        self.origin = (np.float32((sx // 2) * SCENE_RES), np.float32((sy // 2) * SCENE_RES))
        self.max_dist = 2.0
        self.omap = orc.OccupancyMap(cells, SCENE_RES, self.origin)
        self.lut = self.omap.update_distances_lut(self.max_dist)
        self.pose = np.array([float(self.origin[0]) + 0.013, float(self.origin[1]) - 0.011, 0.0])
        self.hit = self.pose + np.array([0.0, SCENE_RES, 0.0])
        self.range_max = 30.0
        if kind == "corridor":
            half = SCENE_BEAMS // 2
            up = np.linspace(math.radians(40.0), math.radians(140.0), half + 1)
            down = np.linspace(math.radians(-140.0), math.radians(-40.0), half)
            self.angles = np.concatenate([down, up])
        else:
            self.angles = np.linspace(math.radians(-100.0), math.radians(10.0), SCENE_BEAMS)
        self.ranges = self.cast()
        self.scanner_pose = (0.0, 0.0, 0.0)
        self.map_factors = synth.MAP_FACTORS

    def cast(self):
        """exact ranges to the scenario's walls (the inner faces' centre lines), in double"""
        x, y, th = self.pose
        wy0 = float(self.origin[1]) + (40 - SCENE_SIZE[1] // 2) * SCENE_RES
        wy1 = float(self.origin[1]) + (80 - SCENE_SIZE[1] // 2) * SCENE_RES
        wx = float(self.origin[0]) + (130 - SCENE_SIZE[0] // 2) * SCENE_RES
        out = np.empty(self.angles.shape[0])
        for k, a in enumerate(self.angles):
            c, s = math.cos(th + a), math.sin(th + a)
            hits = []
            if s < 0.0:
                hits.append((wy0 - y) / s)
            if self.kind == "corridor" and s > 0.0:
                hits.append((wy1 - y) / s)
            if self.kind == "corner" and c > 0.0:
                hits.append((wx - x) / c)
            out[k] = min(hits)
        assert np.all(np.isfinite(out)) and out.max() < 6.0
        return out

    def oracle_scores(self, R, A, xy_step, theta_step):
        """[M]: the oracle's likelihood-field scores (converged = 0) of the lattice around the hit"""
        from badger_amcl_amd import synth
        orc = self.orc
        base = dict(scanner_pose=self.scanner_pose, off_map_factor=self.map_factors[0],
                    non_free_space_factor=self.map_factors[1], non_free_space_radius=self.map_factors[2])
        base.update(synth.LF_DEFAULTS)
        p = orc.planar(orc.MODEL_LF, SCENE_BEAMS, **base)
        poses = prr.lattice_poses(self.hit[None, :], R, A, xy_step, theta_step, 0)[0]
        s = np.ones((poses.shape[0], 4), dtype=np.float64)
        s[:, :3] = poses
        orc.planar_apply(p, self.omap, s, self.ranges, self.angles, self.range_max, 0, None)
        return s[:, 3].copy()

    def oracle_moments(self):
        R, d, A, q = SCENE_LATTICE
        return moments_row(self.hit, self.oracle_scores(R, A, d, q), R, A, d, q, SCENE_BASELINE)
