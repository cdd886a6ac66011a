"""Test-only: the statistics stages of badger_amcl_amd.sharded.HipShardBackend restated in plain Python over the
oracle backend, so that ShardedFilter.compute_cluster_stats / get_cluster / get_max_weight_pose -- the choice of the
regime, the two exchanges, the host route, the cache -- run under gloo without a GPU.

The ten per-cluster sums are Python integers floor(Fraction(t) * 2**96) (the engine's 32.96 fixed point, `fx_from`
in kernels_stats.hpp), so the reduced sums are exact by construction and can be compared with `==` across world
sizes and splits."""
import math
from fractions import Fraction

import numpy as np
import torch

from shard_backends import OracleShardBackend

CELL_XY, CELL_TH = 0.5, 10 * np.pi / 180
BLOCK_MAX, BLOCK_BINS, BLOCK_CLUSTERS = 4096, 1024, 64  # kStatBlockMax / Bins / Clusters
ONE = 1 << 96
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def pose_key(p):
    return (int(np.floor(p[0] / CELL_XY)), int(np.floor(p[1] / CELL_XY)), int(np.floor(p[2] / CELL_TH)))


def pack(k):
    """kld_pack (kernels_kld.hpp): None when the key does not fit."""
    a, b, c = k[0] + (1 << 23), k[1] + (1 << 23), k[2] + (1 << 15)
    if a < 0 or a >= (1 << 24) - 1 or b < 0 or b >= (1 << 24) or c < 0 or c >= (1 << 16):
        return None
    return (a << 40) | (b << 16) | c


def unpack(pk):
    return ((pk >> 40) - (1 << 23), ((pk >> 16) & 0xFFFFFF) - (1 << 23), (pk & 0xFFFF) - (1 << 15))


def terms(p):
    """(ten exact integers, all finite and in range) for one sample (x, y, theta, w)."""
    x, y, th, w = (float(v) for v in p)
    c, s = math.cos(th), math.sin(th)
    ts = [w, w * x, w * y, w * c, w * s, w * x * x, w * x * y, w * y * x, w * y * y]
    if not all(abs(t) < 2.0e9 for t in ts):  # (NaN fails the comparison too)
        return None
    return [int(math.floor(Fraction(t) * ONE)) for t in ts] + [ONE]


def bins_of(samples, first):
    """[(packed key, global index of the key's first sample)] in increasing first-index order; None: host route."""
    seen, out = {}, []
    for i in range(samples.shape[0]):
        pk = pack(pose_key(samples[i]))
        if pk is None or terms(samples[i]) is None:
            return None
        if pk not in seen:
            seen[pk] = first + i
            out.append((pk, first + i))
    return out


def label_bins(bins):
    """bins: {packed key: smallest first index}.  26-connected components by union-find over the BINS, the later
    root under the earlier; a component's label = rank of its earliest bin among the components' earliest bins."""
    parent = {pk: pk for pk in bins}

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for pk in bins:
        k = unpack(pk)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dt in (-1, 0, 1):
                    if dx == dy == dt == 0:
                        continue
                    o = pack((k[0] + dx, k[1] + dy, k[2] + dt))
                    if o is None or o not in bins:
                        continue
                    a, b = find(pk), find(o)
                    if a != b:
                        if bins[a] < bins[b]:
                            a, b = b, a
                        parent[a] = b
    roots = sorted((pk for pk in bins if find(pk) == pk), key=lambda q: bins[q])
    rank = {pk: r for r, pk in enumerate(roots)}
    return {pk: rank[find(pk)] for pk in bins}, len(roots)


def fx_to_double(v):
    hi, lo = v >> 64, v & M64  # (Python's >> floors, like the signed hi word)
    return float(hi) * 2.0 ** -32 + float(lo) * 2.0 ** -96


def moments(sums):
    """stats_moments (kernels_stats.hpp) on one row of ten integer sums."""
    m = [fx_to_double(v) for v in sums]
    w = m[0]
    with np.errstate(all="ignore"):
        mean = [np.float64(m[1]) / w, np.float64(m[2]) / w, math.atan2(m[4], m[3])]
        cov = [np.float64(m[5]) / w - mean[0] * mean[0], np.float64(m[6]) / w - mean[0] * mean[1],
               np.float64(m[7]) / w - mean[1] * mean[0], np.float64(m[8]) / w - mean[1] * mean[1]]
        r = math.sqrt(m[3] * m[3] + m[4] * m[4])
        cov.append(-2 * math.log(r) if r > 0 else float("inf"))
    return w, np.array(mean, dtype=np.float64), int(sums[9] >> 96), np.array(cov, dtype=np.float64)


def to_limbs(v):
    """128-bit two's complement of v as four 32-bit limbs, least significant first, the top one signed."""
    u = v & ((1 << 128) - 1)
    top = (u >> 96) & M32
    return [u & M32, (u >> 32) & M32, (u >> 64) & M32, top - (1 << 32) if top >> 31 else top]


def from_limbs(l):
    v = (l[0] + (l[1] << 32) + (l[2] << 64) + (l[3] << 96)) & ((1 << 128) - 1)
    return v - (1 << 128) if v >> 127 else v


class StatsOracleShardBackend(OracleShardBackend):
    """OracleShardBackend + the statistics stages.  `stage_calls` lists the stage methods in call order;
    `int_sums` holds the reduced integer sums [cluster][10] of the last device-style evaluation."""

    stats_host_option = False  # BPF_OPT_STATS_HOST

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.stage_calls = []
        self.int_sums = None
        self._res = None

    # ---- results
    def _install(self, sums):
        self.int_sums = [list(row) for row in sums]
        cl = [moments(row) for row in sums]
        tot = [sum(row[k] for row in sums) for k in range(10)]
        _, set_mean, _, set_cov = moments(tot)
        best, bw = -1, 0.0
        for k, c in enumerate(cl):
            if c[0] > bw:  # first of equals
                best, bw = k, c[0]
        self._res = dict(n=len(cl), set_mean=set_mean, set_cov=set_cov, clusters=cl, best_w=bw if best >= 0 else 0.0,
                         best_pose=cl[best][1].copy() if best >= 0 else np.zeros(3))

    def stats_result(self):
        return self._res["n"], self._res["set_mean"], self._res["set_cov"]

    def stats_cluster(self, k):
        if k < 0 or k >= self._res["n"]:
            return None
        return self._res["clusters"][k]

    def stats_max_weight_pose(self):
        return self._res["best_w"], self._res["best_pose"]

    # ---- gathered form
    def stats_local_soa(self):
        return torch.from_numpy(np.ascontiguousarray(self.samples[:, :4].T))

    def stats_gathered(self, soa, global_n):
        self.stage_calls.append("gathered")
        if self.stats_host_option:
            return -1
        s = np.ascontiguousarray(soa.numpy().T)
        assert s.shape == (global_n, 4) and global_n <= BLOCK_MAX
        listed = bins_of(s, 0)
        if listed is None:
            return -1
        if len(listed) > BLOCK_BINS:
            return 0
        labels, C = label_bins(dict(listed))
        if C > BLOCK_CLUSTERS:
            return 0
        sums = [[0] * 10 for _ in range(C)]
        for i in range(global_n):
            row = sums[labels[pack(pose_key(s[i]))]]
            for k, t in enumerate(terms(s[i])):
                row[k] += t
        self._install(sums)
        return 1

    # ---- distributed form
    def stats_local_bins(self, global_first):
        self.stage_calls.append("local_bins")
        listed = None if self.stats_host_option else bins_of(self.samples, global_first)
        if listed is None:
            return torch.zeros((2, 0), dtype=torch.int64), True
        # (a packed key uses all 64 bits: it travels as the int64 with the same bit pattern, as on the device)
        t = torch.tensor([[b[0] - (1 << 64) if b[0] >> 63 else b[0] for b in listed], [b[1] for b in listed]],
                         dtype=torch.int64).reshape(2, len(listed))
        return t, False

    def stats_label(self, all_bins, counts, pad):
        self.stage_calls.append("label")
        a = all_bins.numpy()
        assert a.shape == (len(counts), 2, pad)
        merged = {}
        for r, c in enumerate(counts):
            for q in range(c):
                pk, first = int(a[r, 0, q]) & M64, int(a[r, 1, q])
                if pk not in merged or first < merged[pk]:
                    merged[pk] = first
        self._labels, self._clusters = label_bins(merged)
        return self._clusters

    def stats_local_sums(self):
        self.stage_calls.append("local_sums")
        sums = [[0] * 10 for _ in range(self._clusters)]
        for i in range(self.samples.shape[0]):
            row = sums[self._labels[pack(pose_key(self.samples[i]))]]
            for k, t in enumerate(terms(self.samples[i])):
                row[k] += t
        words = []
        for k in range(10):          # [term][cluster][limb], as the engine lays them out
            for c in range(self._clusters):
                words += to_limbs(sums[c][k])
        return torch.tensor(words, dtype=torch.int64)

    def stats_finish(self, reduced):
        self.stage_calls.append("finish")
        w = [int(v) for v in reduced.tolist()]
        C = self._clusters
        assert len(w) == 40 * C
        self._install([[from_limbs(w[4 * (k * C + c):4 * (k * C + c) + 4]) for k in range(10)] for c in range(C)])

    # ---- host route
    def stats_local_samples_host(self):
        return self.samples

    def stats_host(self, all_samples):
        self.stage_calls.append("host")
        s = np.ascontiguousarray(all_samples, dtype=np.float64)
        t = self.orc.KDTree()
        for k in range(s.shape[0]):
            t.insert_pose(s[k, :3], s[k, 3])
        want = t.cluster_stats(s, s.shape[0])
        self.int_sums = None
        cl = [(want["weight"][k], want["mean"][k], int(want["count"][k]), want["cov"][k]) for k in range(want["n"])]
        best, bw = -1, 0.0
        for k, c in enumerate(cl):
            if c[0] > bw:
                best, bw = k, c[0]
        self._res = dict(n=want["n"], set_mean=want["set_mean"], set_cov=want["set_cov"], clusters=cl,
                         best_w=bw if best >= 0 else 0.0, best_pose=cl[best][1].copy() if best >= 0 else np.zeros(3))
