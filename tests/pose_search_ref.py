"""numpy model of the exhaustive pose search (bpf_planar_search_poses): the candidate enumeration over a free-space
list and the order of the result.  Shared by tests/test_pose_search_cpu.py, which pins the enumeration against
pose_check_ref.FreeSpace.planar, and tests/test_gpu_pose_search.py, which holds the device to it."""
import numpy as np


class Space:
    """The candidate space of one map: F_s (the free list's entries with i % s == 0 and j % s == 0, in order) x H
    headings.  free_cells: [(i, j)] of Node2D::updateFreeSpaceIndices, i outer, j inner."""

    def __init__(self, free_cells, size_x, size_y, origin, res, headings, stride):
        ij = np.array(free_cells, dtype=np.int64).reshape(-1, 2)
        keep = (ij[:, 0] % stride == 0) & (ij[:, 1] % stride == 0)
        self.ij = ij[keep]
        self.size_x, self.size_y, self.res = int(size_x), int(size_y), float(res)
        self.origin = (float(origin[0]), float(origin[1]))
        self.headings = int(headings)
        self.total = self.ij.shape[0] * self.headings

    @classmethod
    def of(cls, geo, headings, stride):
        """of a map_geometry.GeoScenario"""
        return cls(geo.free_cells(), geo.size_x, geo.size_y, geo.origin, geo.res, headings, stride)

    def rows(self, cands):
        """(i, j, heading, poses[n, 3]) of the candidate indices `cands`: x, y as convertMapToWorld forms them
        (integer halves, multiply then add), theta = (2.0 * pi * h) / H - pi in double as written."""
        c = np.asarray(cands, dtype=np.int64)
        f, h = c // self.headings, c % self.headings
        i, j = self.ij[f, 0], self.ij[f, 1]
        poses = np.empty((c.shape[0], 3), dtype=np.float64)
        poses[:, 0] = self.origin[0] + (i - self.size_x // 2).astype(np.float64) * self.res
        poses[:, 1] = self.origin[1] + (j - self.size_y // 2).astype(np.float64) * self.res
        poses[:, 2] = (2.0 * np.pi * h.astype(np.float64)) / float(self.headings) - np.pi
        return i, j, h, poses

    def samples(self, first, count):
        """[count, 4] sample rows {pose, 1.0} of candidates first .. first + count - 1, for an oracle to score."""
        s = np.empty((count, 4), dtype=np.float64)
        s[:, :3] = self.rows(np.arange(first, first + count))[3]
        s[:, 3] = 1.0
        return s


def order(scores, cands):
    """Positions of (scores, cands) in the search's order: score descending, equal scores by candidate ascending, NaN
    behind every number (stable sorts, least significant key first)."""
    scores = np.asarray(scores, dtype=np.float64)
    cands = np.asarray(cands, dtype=np.int64)
    nan = np.isnan(scores)
    key = np.where(nan, -np.inf, scores)
    idx = np.argsort(cands, kind="stable")
    idx = idx[np.argsort(-key[idx], kind="stable")]
    return idx[np.argsort(nan[idx], kind="stable")]


def top_k(scores, first, k):
    """Candidate indices of the best min(k, len) of scores[0 ...] = the scores of candidates first, first + 1, ..."""
    cands = first + np.arange(len(scores), dtype=np.int64)
    return cands[order(scores, cands)[:k]]
