"""numpy model of the pose refinement (bpf_planar_refine_poses / bpf_cloud_refine_poses): the lattice, the pose
expressions, the order rule and the replay of a trace into centres.  Shared by tests/test_pose_refine_cpu.py and
tests/test_gpu_pose_refine.py, together with the inputs of the GPU test's comparison against the oracle
(planar_case, oracle_descent), so that the condition on those inputs is checked where no GPU is needed."""
import math

import numpy as np

MAX_POINTS = 2048
DECIDED = 4e-9  # relative margin above which the oracle's best point is decided (the search tests' bar)


def lattice(R, A):
    """(M, m_c)"""
    side, turns = 2 * R + 1, 2 * A + 1
    return side * side * turns, (R * side + R) * turns + A


def offsets(R, A):
    """(a - R, b - R, t - A) of every point m = (a (2R+1) + b) (2A+1) + t, as int64 arrays of length M"""
    side, turns = 2 * R + 1, 2 * A + 1
    m = np.arange(side * side * turns, dtype=np.int64)
    ab, t = m // turns, m % turns
    return ab // side - R, ab % side - R, t - A


def steps(xy_step, theta_step, R, A, level):
    """(d_l, q_l): the steps scaled by 2^-level exactly; a step whose radius is 0 is not read and counts as 0.0"""
    return (math.ldexp(float(xy_step), -level) if R > 0 else 0.0,
            math.ldexp(float(theta_step), -level) if A > 0 else 0.0)


def lattice_poses(centres, R, A, xy_step, theta_step, level):
    """[n, M, 3]: the poses of the lattice around every row of centres[n, 3]: c + (double)(offset) * step, the
    product rounded before the sum"""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    da, db, dt = offsets(R, A)
    d, q = steps(xy_step, theta_step, R, A, level)
    out = np.empty((c.shape[0], da.shape[0], 3), dtype=np.float64)
    out[:, :, 0] = c[:, None, 0] + (da.astype(np.float64) * d)[None, :]
    out[:, :, 1] = c[:, None, 1] + (db.astype(np.float64) * d)[None, :]
    out[:, :, 2] = c[:, None, 2] + (dt.astype(np.float64) * q)[None, :]
    return out


def choose(scores, centre):
    """the m the order rule picks from the M scores of one lattice: score descending, among equal scores the centre
    first, then m ascending, NaN below every number"""
    s = np.asarray(scores, dtype=np.float64)
    nan = np.isnan(s)
    if nan.all():
        return int(centre)
    best = np.max(s[~nan])
    at = np.flatnonzero(~nan & (s == best))
    return int(centre) if centre in at else int(at[0])


def replay(poses, trace, R, A, xy_step, theta_step):
    """(final[n, 3], moved[n], centres[n, L, 3]): the descent the trace[n, L] describes.  centres[:, l] is what level l
    started from.  A chosen centre leaves the pose untouched (bit for bit); any other m moves it to that point's
    pose."""
    c = np.array(poses, dtype=np.float64).reshape(-1, 3)
    trace = np.asarray(trace).reshape(c.shape[0], -1)
    n, L = trace.shape
    M, mc = lattice(R, A)
    assert trace.min() >= 0 and trace.max() < M
    da, db, dt = offsets(R, A)
    centres = np.empty((n, L, 3), dtype=np.float64)
    moved = np.zeros(n, dtype=np.int64)
    for level in range(L):
        centres[:, level] = c
        d, q = steps(xy_step, theta_step, R, A, level)
        m = trace[:, level]
        go = m != mc
        nxt = np.stack([c[:, 0] + da[m].astype(np.float64) * d, c[:, 1] + db[m].astype(np.float64) * d,
                        c[:, 2] + dt[m].astype(np.float64) * q], axis=1)
        c = np.where(go[:, None], nxt, c)
        moved += go
    return c, moved, centres


def decided(scores, centre):
    """(m of the best score under the order rule, whether that score is more than DECIDED relative above every other
    point's) for one lattice's M scores"""
    s = np.asarray(scores, dtype=np.float64)
    m = choose(s, centre)
    others = np.delete(s, m)
    ok = bool(np.isfinite(s[m]) and np.all(s[m] - others > DECIDED * abs(s[m])))
    return m, ok


# ---------------------------------------------------------------- inputs of the planar comparison against the oracle
MAX_BEAMS = 31
MODELS = ("lf", "gompertz", "prob", "beam")
MODEL_KW = {"prob": dict(do_beamskip=1)}  # armed; the score runs with set->converged = 0
CONFIGS = ((1, 1, 3), (2, 2, 2), (2, 0, 1), (0, 3, 4))  # (R, A, L)
MAPS = ("G1", "G2", "G3")
THETA_STEP = math.pi / 8.0  # half the step of a search at 8 headings
XY_STEP_CELLS = 2.0


def planar_case(orc, model, config):
    """(geo, start poses[n, 3], xy_step, theta_step) of one (model, (R, A, L)) case: the maps rotate over the cases;
    the poses are the centres of the 6 x 6 cells around the scenario's true cell at the nearest of 8 headings, plus
    four free cells far from it at other headings"""
    from map_geometry import GeoScenario
    name = MAPS[(MODELS.index(model) + CONFIGS.index(config)) % len(MAPS)]
    geo = GeoScenario.named(orc, name, beams=61, frac_nan=0.0)
    ci, cj = geo.size_x // 2, geo.size_y // 2
    heading = lambda h: (2.0 * math.pi * h) / 8.0 - math.pi  # noqa: E731
    h0 = min(range(8), key=lambda h: abs(heading(h) - geo.pose[2]))
    cells = [(i, j, h0) for i in range(ci - 3, ci + 3) for j in range(cj - 3, cj + 3)]
    free = geo.free_cells()
    cells += [free[(k + 1) * len(free) // 5] + (2 * k + 1,) for k in range(4)]
    poses = np.array([[float(geo.origin[0]) + (i - geo.size_x // 2) * geo.res,
                       float(geo.origin[1]) + (j - geo.size_y // 2) * geo.res, heading(h)] for i, j, h in cells])
    return geo, poses, XY_STEP_CELLS * geo.res, THETA_STEP


def oracle_lattice_scores(geo, op, centres, R, A, xy_step, theta_step, level):
    """[n, M]: the oracle's scores (converged = 0) of the lattice poses of `level` around centres[n, 3]"""
    p = lattice_poses(centres, R, A, xy_step, theta_step, level)
    s = np.ones((p.shape[0] * p.shape[1], 4), dtype=np.float64)
    s[:, :3] = p.reshape(-1, 3)
    geo.oracle_apply(op, s, 0)
    return s[:, 3].reshape(p.shape[0], p.shape[1])


def oracle_descent(orc, model, config):
    """The descent with the oracle's scores alone: (trace[n, L], decided[n, L])"""
    R, A, L = config
    geo, poses, xy_step, theta_step = planar_case(orc, model, config)
    op = geo.oracle_planar(MAX_BEAMS, model, kw=MODEL_KW.get(model))
    M, mc = lattice(R, A)
    n = poses.shape[0]
    trace = np.zeros((n, L), dtype=np.int64)
    dec = np.zeros((n, L), dtype=bool)
    c = poses.copy()
    for level in range(L):
        w = oracle_lattice_scores(geo, op, c, R, A, xy_step, theta_step, level)
        for r in range(n):
            trace[r, level], dec[r, level] = decided(w[r], mc)
        c = replay(c, trace[:, level:level + 1], R, A, *[math.ldexp(v, -level) for v in (xy_step, theta_step)])[0]
    return trace, dec
