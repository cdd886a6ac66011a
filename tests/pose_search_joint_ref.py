"""numpy model of the joint pose search (bpf_planar_search_poses_joint, bpf_cloud_search_poses_joint): the heading
table, the composed poses of a candidate and the sequential scoring that carries the weight from scan to scan.  The
candidate enumeration is pose_search_ref.Space / pose_search_cloud_ref.Space, the order pose_search_ref.order.  Shared by
tests/test_pose_search_joint_cpu.py and the GPU tests of the joint search."""
import math

import numpy as np


def heading_table(headings):
    """(C_h, S_h): math.cos / math.sin of theta_h = (2.0 * pi * h) / H - pi, one call per heading (the C library's
    functions, the ones the engine's host code tabulates)"""
    n = int(headings)
    th = [(2.0 * math.pi * float(h)) / float(n) - math.pi for h in range(n)]
    return np.array([math.cos(t) for t in th], dtype=np.float64), np.array([math.sin(t) for t in th], dtype=np.float64)


def compose(space, cands, offsets):
    """[n, S, 3]: the poses candidate c is scored at, its base pose composed with offsets[s] = (dx, dy, dth) as
    coordAdd writes it, left to right, every product and sum rounded on its own; theta is not normalised"""
    c = np.asarray(cands, dtype=np.int64)
    _, _, h, base = space.rows(c)
    ch, sh = heading_table(space.headings)
    ch, sh = ch[h], sh[h]
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 3)
    out = np.empty((c.shape[0], off.shape[0], 3), dtype=np.float64)
    for s, (dx, dy, dth) in enumerate(off):
        out[:, s, 0] = (base[:, 0] + dx * ch) - dy * sh
        out[:, s, 1] = (base[:, 1] + dx * sh) + dy * ch
        out[:, s, 2] = base[:, 2] + dth
    return out


def sequential_scores(poses, apply_scan):
    """w_S of every candidate: w_0 = 1.0, and apply_scan(s, samples) multiplies the weights of samples[n, 4] =
    {poses[:, s], w_s} in place, as applyModelToSampleSet does.  Returns the weights after the last scan."""
    n, n_scans = poses.shape[0], poses.shape[1]
    w = np.ones(n, dtype=np.float64)
    for s in range(n_scans):
        samples = np.empty((n, 4), dtype=np.float64)
        samples[:, :3] = poses[:, s]
        samples[:, 3] = w
        apply_scan(s, samples)
        w = samples[:, 3].copy()
    return w


def pose_add(pose, offset):
    """pose (+) offset for one pose: where the robot stands at a scan taken `offset` from `pose`"""
    x, y, th = (float(v) for v in pose)
    dx, dy, dth = (float(v) for v in offset)
    c, s = math.cos(th), math.sin(th)
    return np.array([(x + dx * c) - dy * s, (y + dx * s) + dy * c, th + dth], dtype=np.float64)
