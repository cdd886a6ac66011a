"""The mixture initialiser as the oracle forms it: K successive orc_pf_init_with_gaussian calls on consecutive slices
of one sample array, sharing the filter's rng (bpf_pf_init_with_mixture in include/badger_pf.h is defined as this).
Shared by tests/test_pose_mixture_cpu.py and tests/test_gpu_mixture_init.py."""
import ctypes as C

import numpy as np

from pose_mixture_ref import COMPONENT_DTYPE


def oracle_init_with_mixture(orc, opf, comps):
    """opf: pyoracle.ParticleFilter with max_samples = the counts' sum.  Leaves the set in opf (samples, sample_count,
    leaf_count of the whole set's tree, converged cleared) and returns the samples."""
    n = int(np.sum(comps["count"]))
    assert n == opf.pf.max_samples
    s = np.zeros((n, 4), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    nodes = C.c_int()
    at = 0
    for c in comps:
        k = int(c["count"])
        if k == 0:
            continue
        m, r, d = (np.ascontiguousarray(c[f], dtype=np.float64).reshape(-1) for f in ("mean", "rotation", "sigma"))
        part = s[at:at + k]
        orc.lib().orc_pf_init_with_gaussian(C.byref(opf.pf), m.ctypes.data_as(dp), r.ctypes.data_as(dp),
                                            d.ctypes.data_as(dp), part.ctypes.data_as(dp), k, C.byref(nodes))
        at += k
    opf.set_samples(s)  # (the tree of the WHOLE set, in sample order)
    opf.set_converged = 0
    return s


def oracle_max_weight_pose(orc, samples):
    """Node2D::getMaxWeightPose on the oracle's tree of `samples` [n, 4]: (weight, mean) of the heaviest cluster."""
    s = np.ascontiguousarray(samples, dtype=np.float64)
    t = orc.KDTree()
    for r in s:
        t.insert_pose(r[:3], r[3])
    t.cluster()
    st = t.cluster_stats(s, s.shape[0])
    k = int(np.argmax(st["weight"]))
    return float(st["weight"][k]), np.array(st["mean"][k])


# the end-to-end scenario of tests/test_gpu_mixture_init.py and its oracle-only precondition in
# tests/test_pose_mixture_cpu.py: Scenario(orc, size=200), E2E_N samples, E2E_CYCLES sensor updates + resamples
E2E_N, E2E_BEAMS, E2E_SEED = 4096, 61, 7
E2E_HEADINGS, E2E_STRIDE, E2E_HITS = 24, 2, 256
E2E_CYCLES = 3
E2E_CAP = 8
E2E_SIGMA = (0.05, 0.05, 0.03)


E2E_REFINE = (2, 2, 4)  # xy_radius, theta_radius, levels


def e2e_scenario(orc):
    """The scan is cast from the scenario's pose itself, so the scanner sits at the robot's origin: with the default
    scanner offset the pose that explains the scan is sc.pose less that offset, not sc.pose."""
    from scenario import Scenario
    return Scenario(orc, size=200, n=E2E_N, beams=E2E_BEAMS, scanner_pose=(0.0, 0.0, 0.0))


def e2e_refine_steps(res, headings=E2E_HEADINGS):
    """(xy_step, theta_step) of the refinement: half the search's cell stride, half its heading step"""
    return E2E_STRIDE * res / 2.0, np.pi / headings


def oracle_search_refine(sc_):
    """searchPoses -> refinePoses with the oracle's scores alone (pose_search_ref / pose_refine_ref are the models the
    device calls are held to): (poses[n, 3], scores[n]) of the refined best E2E_HITS candidates."""
    import pose_check_ref as ref
    import pose_search_ref as psr
    p = sc_.oracle_planar(E2E_BEAMS, "lf")
    free = ref.free_cells_2d(sc_.cells, sc_.lut, sc_.map_factors[2])
    sp = psr.Space(free, sc_.size, sc_.size, sc_.origin, sc_.res, E2E_HEADINGS, E2E_STRIDE)
    s = sp.samples(0, sp.total)
    sc_.oracle_apply(p, s, 0)
    top = psr.top_k(s[:, 3], 0, E2E_HITS)
    return oracle_descent(sc_, p, s[top, :3].copy(), s[top, 3].copy(), sc_.res, E2E_HEADINGS)


def oracle_descent(geo, p, poses, scores, res, headings):
    """the lattice descent of refinePoses on geo.oracle_apply(p, samples, 0)'s scores: (poses, scores)"""
    import pose_refine_ref as prr
    R, A, L = E2E_REFINE
    xy_step, theta_step = e2e_refine_steps(res, headings)
    mc = prr.lattice(R, A)[1]
    for level in range(L):
        lat = prr.lattice_poses(poses, R, A, xy_step, theta_step, level)
        sco = prr.oracle_lattice_scores(geo, p, poses, R, A, xy_step, theta_step, level)
        for r in range(poses.shape[0]):
            m = prr.choose(sco[r], mc)
            scores[r] = sco[r, m]
            if m != mc:
                poses[r] = lat[r, m]
    return poses, scores


def e2e_merge(res, headings=E2E_HEADINGS):
    """(xy_merge, theta_merge): one cell, half a search heading step"""
    return res, np.pi / headings


def oracle_cycles(sc_, opf, cycles):
    """`cycles` sensor updates + resamples of the oracle filter with the scenario's scan (likelihood field)"""
    p = sc_.oracle_planar(E2E_BEAMS, "lf")
    for _ in range(cycles):
        opf.update_sensor(lambda s, conv: sc_.oracle_apply(p, s, conv))
        opf.update_resample()


def within_e2e_bound(pose, truth, res, headings=E2E_HEADINGS):
    """one cell in x and y, one search heading step in theta"""
    d = np.fmod((pose[2] - truth[2]) + np.pi, 2.0 * np.pi)
    d = d + np.pi if d <= 0.0 else d - np.pi
    return (abs(pose[0] - truth[0]) <= res and abs(pose[1] - truth[1]) <= res and
            abs(d) <= 2.0 * np.pi / headings)


# the cloud form: the room, cloud, mounting and model of tests/test_gpu_pose_search_cloud.py at its smallest shape
# (6 x 200 rays, 8 headings, stride 2), the cloud cast from the scanner's place at TRUTH
E2E_CLOUD_HEADINGS = 8
E2E_CLOUD_BEAMS = 128
# the cloud model (128 of the points, sigma_hit 0.1 m) is far flatter than the planar field: components 0.1 m apart
# share a cluster, and the oracle alone needs 6 cycles to bring that cluster's mean within a cell of the truth in y
# (3 cycles: 0.057 m off; 6: 0.034; 10: 0.025)
E2E_CLOUD_CYCLES = 10


class CloudScene:
    """lut, points, mounting and the oracle's cloud model; oracle_apply has the signature pose_refine_ref scores
    through"""
    truth = np.array([0.3, 0.2, 0.1])  # test_gpu_cloud._setup
    res = 0.05

    def __init__(self, orc):
        from test_gpu_cloud import _setup
        self.orc = orc
        self.lut, pts, _, self.tf_xyz, self.tf_quat, self.max_dist = _setup(orc, 1, 6, 200, seed=0)
        self.points = np.ascontiguousarray(pts, dtype=np.float32)
        self.op = orc.cloud(orc.CLOUD_MODEL, E2E_CLOUD_BEAMS, self.tf_xyz, self.tf_quat, z_hit=0.5, z_rand=0.05,
                            sigma_hit=0.1)
        self.op.off_map_factor = 0.95

    def oracle_apply(self, p, samples, set_converged=0):
        return self.orc.cloud_apply(p, self.lut, samples, self.points)


def oracle_search_refine_cloud(scene):
    """oracle_search_refine for the cloud scanner: every column of the map's rectangle (pose_search_cloud_ref)"""
    import pose_search_cloud_ref as pscr
    sp = pscr.Space(list(scene.lut.min_cells), list(scene.lut.max_cells), scene.res, E2E_CLOUD_HEADINGS, E2E_STRIDE)
    s = sp.samples(0, sp.total)
    scene.oracle_apply(scene.op, s)
    top = pscr.top_k(s[:, 3], 0, E2E_HITS)
    return oracle_descent(scene, scene.op, s[top, :3].copy(), s[top, 3].copy(), scene.res, E2E_CLOUD_HEADINGS)


def oracle_cycles_cloud(scene, opf, cycles):
    for _ in range(cycles):
        opf.update_sensor(lambda s, conv: scene.oracle_apply(scene.op, s, conv))
        opf.update_resample()


def components(n, k, seed, zeros=(), same=None):
    """k components with ragged counts that sum to n; `zeros`: indices forced to count 0; same: one (mean, rotation,
    sigma) for all of them."""
    rng = np.random.default_rng(seed)
    comps = np.zeros(k, dtype=COMPONENT_DTYPE)
    live = [i for i in range(k) if i not in set(zeros)]
    p = rng.uniform(0.2, 1.0, len(live))
    comps["count"][live] = rng.multinomial(n, p / p.sum())
    for i in range(k):
        a = rng.uniform(-3.0, 3.0)
        comps[i]["mean"] = (rng.uniform(2.0, 8.0), rng.uniform(2.0, 8.0), rng.uniform(-3.0, 3.0))
        comps[i]["rotation"] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        comps[i]["sigma"] = rng.uniform(0.01, 0.5, 3)
        if same is not None:
            comps[i]["mean"], comps[i]["rotation"], comps[i]["sigma"] = same
    return comps
