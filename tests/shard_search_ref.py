"""numpy model of the pose search over a sharded filter (bpf_shard_search_poses and its siblings): the split of a
range over the ranks, the key map of the device's lists with its inverse, the merge of the ranks' padded lists, and
the pruned call's decisions replayed per rank with the floor the ranks share behind their seeds.  Shared by
tests/test_shard_search_cpu.py and tests/test_gpu_shard_search.py.

The replay re-states pose_search_pruned_ref.replay (which has no floor) and is checked against it where no floor is
set."""
import struct

import numpy as np

import pose_search_ref as psr
from pose_search_pruned_ref import SEED, WINDOW


def split(first, total, world):
    """[(first_r, count_r)] of ranks 0 .. world - 1: units [first + T r / W, first + T (r + 1) / W)"""
    return [(first + (total * r) // world, (total * (r + 1)) // world - (total * r) // world) for r in range(world)]


# ---- the key map (kernels_pose_search.hpp: search_key_of / search_score_of)
def key_of(score):
    score = float(score)
    if score != score:
        return 0
    u = struct.unpack("<Q", struct.pack("<d", score + 0.0))[0]  # -0.0 -> +0.0
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | (1 << 63)


def score_of(key):
    if key == 0:
        return float("nan")
    u = key & 0x7FFFFFFFFFFFFFFF if key >> 63 else (~key) & 0xFFFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<Q", u))[0]


# ---- the merge of the ranks' lists (k_search_merge_lists)
def entries_of(scores, cands):
    """[(key, inv)] sorted best first: the lexicographically larger (key, ~candidate) is the better entry"""
    e = [(key_of(s), (~int(c)) & 0xFFFFFFFFFFFFFFFF) for s, c in zip(scores, cands)]
    return sorted(e, reverse=True)


def merge_lists(lists, k):
    """lists[r]: rank r's sorted entries (at most k).  Every list is padded to k rows with the empty entry (0, 0) and
    travels with its count; the fold takes list after list into a running best k, as the device's bitonic merge
    does.  Returns the merged entries."""
    best = []
    for lst in lists:
        padded = list(lst) + [(0, 0)] * (k - len(lst))
        count = len(lst)
        best = sorted(best + padded[:count], reverse=True)[:k]
    return best


# ---- the pruned call of one rank, with a floor
class RankReplay:
    """One rank's pruned call over its share: bounds[q] and the block list are the share's own (q = 0 is the share's
    first block at heading 0).  seed() runs the call up to the exchange of the floor and returns the word the rank
    publishes (its k-th exact score, or None: the list holds fewer than k rows or that score is a NaN); finish(floor)
    runs the rest against `floor` (None: no rank published one) and returns the stats fields and `best`."""

    def __init__(self, bounds, scores, start, member, headings, k, window=WINDOW, seed=SEED, max_members=None):
        self.bounds = np.asarray(bounds, dtype=np.float64)
        self.scores, self.start, self.member = scores, np.asarray(start), np.asarray(member)
        self.headings, self.k, self.window, self.seed_rows = headings, k, window, seed
        self.nq = self.bounds.shape[0]
        self.sizes = np.diff(self.start)
        self.size_q = np.repeat(self.sizes, headings)
        # the seed's windows are sized by the largest block of the WHOLE list, which a share may not hold
        self.max_members = int(self.sizes.max()) if max_members is None and self.nq else max_members

    def member_scores(self, q):
        b, h = divmod(int(q), self.headings)
        return self.scores[self.member[self.start[b]:self.start[b + 1]], h]

    def fold(self, best, new):
        a = np.concatenate([best] + list(new))
        nan = np.isnan(a)
        return np.concatenate([np.sort(a[~nan])[::-1], a[nan]])[:self.k]  # NaN below every number

    def tau_of(self, best, floor):
        """prune_tau: (full, tau)"""
        own = best.shape[0] >= self.k
        if floor is not None:  # (a NaN k-th score of the rank's own is below every floor)
            return True, (float(best[self.k - 1]) if own and best[self.k - 1] > floor else floor)
        return (True, best[self.k - 1]) if own else (False, 0.0)

    def seed(self):
        if self.nq == 0:
            self.best = np.zeros(0)
            return None
        self.seed_q = psr.order(self.bounds, np.arange(self.nq))[:min(self.seed_rows, self.nq)]
        self.best = self.fold(np.zeros(0), [self.member_scores(q) for q in self.seed_q])
        if self.best.shape[0] >= self.k and self.best[self.k - 1] == self.best[self.k - 1]:
            return float(self.best[self.k - 1])
        return None

    def finish(self, floor):
        nq, k, window, bounds, size_q = self.nq, self.k, self.window, self.bounds, self.size_q
        if nq == 0:
            return dict(block_candidates=0, seed_candidates=0, pruned_block_candidates=0, expanded_block_candidates=0,
                        scored_candidates=0, windows=0, best=np.zeros(0))
        best = self.best
        seed_members = int(size_q[self.seed_q].sum())
        full, tau = self.tau_of(best, floor)
        in_seed = np.zeros(nq, dtype=bool)
        in_seed[self.seed_q] = True
        surv = np.flatnonzero(~in_seed & ~(full & (bounds < tau)))
        first = np.concatenate([[0], np.cumsum(size_q[surv])]).astype(np.int64)
        total = int(first[-1])
        kept = np.zeros(surv.shape[0], dtype=bool)
        dropped = expanded = expanded_members = 0
        for lo in range(0, total, window):
            hi = min(lo + window, total)
            full, tau = self.tau_of(best, floor)
            new = []
            i = int(np.searchsorted(first, lo, side="right")) - 1  # the survivor that holds slot lo
            while i < surv.shape[0] and first[i] < hi:
                q = surv[i]
                if first[i] >= lo:
                    kept[i] = not (full and bounds[q] < tau)
                    if kept[i]:
                        expanded += 1
                        expanded_members += int(size_q[q])
                    else:
                        dropped += 1
                if kept[i]:
                    ms = self.member_scores(q)
                    new.append(ms[max(lo - first[i], 0):min(hi - first[i], ms.shape[0])])
                i += 1
            best = self.fold(best, new)
        candidates = int(self.sizes.sum()) * self.headings
        seed_room = min(min(self.seed_rows, nq) * self.max_members, candidates)
        return dict(block_candidates=nq, seed_candidates=int(self.seed_q.shape[0]),
                    pruned_block_candidates=nq - int(self.seed_q.shape[0]) - int(surv.shape[0]) + dropped,
                    expanded_block_candidates=expanded, scored_candidates=seed_members + expanded_members,
                    windows=-(-nq // window) + -(-seed_room // window) + -(-total // window), best=best)


def floor_of(words):
    """the floor of the ranks' published words: the largest, None when no rank published one"""
    have = [w for w in words if w is not None]
    return max(have) if have else None


def replay_world(bounds, scores, start, member, headings, k, first_block, block_count, world, shared=True,
                 window=WINDOW, seed=SEED):
    """The sharded pruned call over blocks first_block .. first_block + block_count - 1 of the block list (bounds[q]
    over the WHOLE list): per rank the stats fields and `best` (its own list's scores), with the floor (shared) or
    as stand-alone range calls; and the floor itself."""
    start = np.asarray(start)
    ranks, widest = [], int(np.diff(start).max()) if start.shape[0] > 1 else 0
    for lo, n in split(first_block, block_count, world):
        sub_start = start[lo:lo + n + 1]
        ranks.append(RankReplay(bounds[lo * headings:(lo + n) * headings], scores, sub_start, member, headings, k,
                                window, seed, widest))
    words = [r.seed() for r in ranks]
    floor = floor_of(words) if shared else None
    return [r.finish(floor) for r in ranks], floor
