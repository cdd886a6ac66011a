"""numpy model of the exhaustive pose search with the cloud scanner (bpf_cloud_search_poses): the candidate enumeration
over the columns of the 3-D map's rectangle.  The order of the result is pose_search_ref.order / top_k.  Shared by
tests/test_pose_search_cloud_cpu.py, which pins the enumeration against pose_check_ref.FreeSpace.octo, and
tests/test_gpu_pose_search_cloud.py, which holds the device to it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pose_search_ref import order, top_k  # noqa: E402,F401  (re-exported: one order for both searches)


def first_multiple_at_or_above(a, s):
    """the first multiple of s >= a, for a of either sign (Python's floor division negated is a ceiling)"""
    return -((-int(a)) // int(s)) * int(s)


class Space:
    """The candidate space of one 3-D map: C_s (the columns min <= c < max of Node3D::updateFreeSpaceIndices whose i and
    j the stride divides, i outer, j inner) x H headings.  Never a list: n_i x n_j by arithmetic."""

    def __init__(self, min_cells, max_cells, res, headings, stride):
        s = int(stride)
        self.stride, self.res, self.headings = s, float(res), int(headings)
        self.i0 = first_multiple_at_or_above(min_cells[0], s)
        self.j0 = first_multiple_at_or_above(min_cells[1], s)
        self.n_i = (int(max_cells[0]) - 1 - self.i0) // s + 1 if self.i0 < int(max_cells[0]) else 0
        self.n_j = (int(max_cells[1]) - 1 - self.j0) // s + 1 if self.j0 < int(max_cells[1]) else 0
        self.columns = self.n_i * self.n_j
        self.total = self.columns * self.headings

    def rows(self, cands):
        """(i, j, heading, poses[n, 3]) of the candidate indices `cands`: x = i * res, y = j * res (octomap.cpp:83-95),
        theta = (2.0 * pi * h) / H - pi in double as written."""
        c = np.asarray(cands, dtype=np.int64)
        f, h = c // self.headings, c % self.headings
        i = self.i0 + (f // self.n_j) * self.stride
        j = self.j0 + (f % self.n_j) * self.stride
        poses = np.empty((c.shape[0], 3), dtype=np.float64)
        poses[:, 0] = i.astype(np.float64) * self.res
        poses[:, 1] = j.astype(np.float64) * self.res
        poses[:, 2] = (2.0 * np.pi * h.astype(np.float64)) / float(self.headings) - np.pi
        return i, j, h, poses

    def samples(self, first, count):
        """[count, 4] sample rows {pose, 1.0} of candidates first .. first + count - 1, for a scorer."""
        s = np.empty((count, 4), dtype=np.float64)
        s[:, :3] = self.rows(np.arange(first, first + count))[3]
        s[:, 3] = 1.0
        return s
