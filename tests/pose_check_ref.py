"""Plain-Python restatement of Node::uniformPoseGenerator (node.cpp:847-868) and of its three consumers:
ParticleFilter::initWithPoseFn (particle_filter.cpp:135-163) and the recovery branches of resampleSystematic
(:295-324) and resampleMultinomial (:381-414).  Built from oracle pieces (KDTree, resample_limit) and the drand48
recurrence; shared by tests/test_pose_check_cpu.py (which pins it against the oracle's C restatement) and
tests/test_gpu_pose_check.py (which holds the device to it)."""
import bisect
import math

A48, C48, MASK48 = 0x5DEECE66D, 0xB, (1 << 48) - 1


class Rng:
    def __init__(self, s):
        self.s = int(s)

    def drand48(self):
        self.s = (A48 * self.s + C48) & MASK48
        return self.s / float(1 << 48)


def lcg_affine(k):
    """x -> a x + c (mod 2^48) for k drand48 steps."""
    a, c = 1, 0
    pa, pc = A48, C48
    while k:
        if k & 1:
            a, c = (a * pa) & MASK48, (c * pa + pc) & MASK48
        pa, pc = (pa * pa) & MASK48, (pc * pa + pc) & MASK48
        k >>= 1
    return a, c


def skip(state, k):
    a, c = lcg_affine(k)
    return (a * int(state) + c) & MASK48


def free_cells_2d(cells, lut, radius):
    """Node2D::updateFreeSpaceIndices (node_2d.cpp:317-337): i outer, j inner, FREE and distance > radius."""
    sy, sx = cells.shape
    return [(i, j) for i in range(sx) for j in range(sy) if cells[j, i] == -1 and float(lut[j, i]) > radius]


def free_cells_3d(min_cells, max_cells):
    """Node3D::updateFreeSpaceIndices (node_3d.cpp:306-318): every column of the cell bounds, i outer, j inner."""
    return [(i, j) for i in range(min_cells[0], max_cells[0]) for j in range(min_cells[1], max_cells[1])]


class FreeSpace:
    """Node::randomFreeSpacePose (node.cpp:823-845) over a free-space list and a convertMapToWorld."""

    def __init__(self, cells, to_world):
        self.cells, self.to_world = cells, to_world

    @staticmethod
    def planar(cells, size_x, size_y, origin, res):
        # occupancy_map.cpp:75-88
        return FreeSpace(cells, lambda i, j: (float(origin[0]) + (i - size_x // 2) * res,
                                              float(origin[1]) + (j - size_y // 2) * res))

    @staticmethod
    def octo(min_cells, max_cells, res):
        # octomap.cpp:83-95: no origin, no half-cell offset
        return FreeSpace(free_cells_3d(min_cells, max_cells), lambda i, j: (i * res, j * res))

    def pose(self, rng):
        idx = int(rng.drand48() * len(self.cells))
        x, y = self.to_world(*self.cells[idx])
        return [x, y, rng.drand48() * 2 * math.pi - math.pi]


def check_active(g0, m):
    return g0 > 0.0 and m < 1.0 and m >= 0.0  # node.cpp:859 (a NaN fails it)


def uniform_pose(rng, fs, g0, m, score=lambda pose: 1.0):
    """Node::uniformPoseGenerator, literally: the reference's scorePose returns 1.0 (node_2d.cpp:298-316)."""
    good = g0
    p = fs.pose(rng)
    if check_active(g0, m):
        while score(p) < good:
            p = fs.pose(rng)
            good *= m
    return p


def retries(g0, m):
    """K = min{k : !(1.0 < thr[k])}, thr[0] = g0, thr[k + 1] = thr[k] * m; 0 with the check inactive."""
    if not check_active(g0, m):
        return 0
    thr, k = g0, 0
    while 1.0 < thr:
        thr *= m
        k += 1
    return k


class FastGen:
    """uniform_pose with score 1.0 as arithmetic: skip 2K elements, then one randomFreeSpacePose."""

    def __init__(self, fs, g0, m):
        self.fs, self.k = fs, retries(g0, m)
        self.a, self.c = lcg_affine(2 * self.k)

    def __call__(self, rng):
        rng.s = (self.a * rng.s + self.c) & MASK48
        return self.fs.pose(rng)


def init_with_pose_fn(rng, n, gen):
    """initWithPoseFn: n back-to-back calls."""
    return [gen(rng) for _ in range(n)]


def resample(samples, leaf_count, w_diff, rng, gen, resampler, orc_pf, kdtree_cls):
    """Both resamplers with random_pose_fn_ = gen; returns (poses, leaf_count, node_count, random flags).
    samples: N x 4 with the weights the resampler sees; orc_pf: an oracle ParticleFilter for resample_limit."""
    n = samples.shape[0]
    maxs = orc_pf.pf.max_samples
    c = [0.0]
    for w in samples[:, 3]:
        c.append(c[-1] + float(w))

    def find(u):
        i = bisect.bisect_right(c, u) - 1
        assert 0 <= i < n and c[i] <= u < c[i + 1], "CDF miss"
        return i

    t = kdtree_cls()
    want, rnd = [], []
    if resampler == 0:
        while len(want) < maxs:
            if rng.drand48() < w_diff:
                pose, r = gen(rng), True
            else:
                pose, r = [float(v) for v in samples[find(rng.drand48()), :3]], False
            want.append(pose)
            rnd.append(r)
            t.insert_pose(pose, 1.0)
            if len(want) > orc_pf.resample_limit(t.leaf_count()):
                break
    else:
        count = orc_pf.resample_limit(leaf_count)
        n_random = 0
        if w_diff > 0.0:
            count = int(count * (1.0 + w_diff))
            count = min(count, maxs)
            n_random = int(w_diff * count)
        n_sys = count - n_random
        start = rng.drand48()
        delta = 1.0 / n_sys
        for _ in range(n_random):
            want.append(gen(rng))
            rnd.append(True)
        target = start
        for _ in range(n_sys):
            want.append([float(v) for v in samples[find(target), :3]])
            rnd.append(False)
            target += delta
            if target > 1.0:
                target -= 1.0
        for pose in want:
            t.insert_pose(pose, 1.0)
    return want, t.leaf_count(), t.node_count(), rnd
