"""Pure-Python restatement, in IEEE doubles, of the multinomial resample of a sharded set in place
(include/badger_pf.h, bpf_shard_set_multinomial_form): the candidate draws from the drand48 stream, their owners by
shard_in_place_ref's slice arithmetic, the ranks' (key, first draw index) lists, their merge, the stop formula and the
stable partition of the reference's set by owner.

Draw m reads stream elements 2 m + 1 (the w_diff test, drawn also when w_diff = 0) and 2 m + 2 (the uniform); with
w_diff > 0 the elements follow the resolved chain (a random pose takes 2 K + 2 elements instead of one)."""
import bisect

import numpy as np

import shard_in_place_ref as ipr
from pose_check_ref import Rng
from shard_stats_ref import pose_key

WINDOW, IN_PLACE = ipr.WINDOW, ipr.IN_PLACE


def candidates(rng_state, maxs, w_diff=0.0, gen=None):
    """Every candidate draw m = 0 .. maxs - 1: (uniform or None, random pose or None, rng state after the draw)."""
    rng = Rng(rng_state)
    out = []
    for _ in range(maxs):
        if rng.drand48() < w_diff:
            pose = gen(rng)
            out.append((None, [float(v) for v in pose], rng.s))
        else:
            out.append((rng.drand48(), None, rng.s))
    return out


def local_cdfs(slices):
    """Each shard's running sum of its weights, c[0] = 0 (the engine's local CDF)."""
    cdfs = []
    for s in slices:
        c = [0.0]
        for w in s[:, 3]:
            c.append(c[-1] + float(w))
        cdfs.append(c)
    return cdfs


def find_local(u, offset, cdf):
    """draw_window_column's search inside the owner's slice: offset + c[i] <= u < offset + c[i + 1]; past the shard's
    running sum (rounding) the last particle."""
    n = len(cdf) - 1
    if not u < offset + cdf[n]:
        return n - 1
    lo, hi = 0, n
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if offset + cdf[mid] <= u:
            lo = mid
        else:
            hi = mid
    return lo


def stop_from_lists(t, leaves, limit, maxs):
    """(M, leaf count, bin count, stopped, branch) from the merged list: t[j] the first draw index of key j (ascending),
    leaves[j] the leaf count after its insertion.  c_j = max(t_j + 1, limit(L_j) + 1); M is the smallest c_j that does
    not pass t_{j+1} (t_B = maxs).  branch: which term of the max gave M ("limit", or "insert": the draw that added
    key j was itself the last)."""
    t = list(t) + [maxs]
    for j in range(len(leaves)):
        lim = limit(leaves[j])
        c = max(t[j] + 1, lim + 1)
        if c <= t[j + 1]:
            return c, leaves[j], j + 1, True, "limit" if lim + 1 >= t[j] + 1 else "insert"
    return maxs, leaves[-1], len(leaves), False, None


def resample(slices, sums, sums_are_totals, rng_state, maxs, limit, leaf_of_keys, w_diff=0.0, gen=None,
             max_share=2.0, auto=False):
    """slices[q]: [n_q, 4] samples of rank q with the weights the resampler sees; sums: the W totals (or CDF sums);
    limit(k) = resampleLimit; leaf_of_keys(keys) -> the leaf count after each key of `keys` inserted in order (for
    BPF_KLD_COUNT_BINS: range(1, len + 1)).
    Returns dict(M, leaf, bins, counts, form, slices (the new poses per rank, [n, 3]), owner, source (per draw < M: the
    global source index, -1 for a random pose), rng (state after the resample), stopped, B, branch)."""
    W = len(slices)
    edges = ipr.slice_edges(sums, sums_are_totals)
    cdfs = local_cdfs(slices)
    firsts = [sum(len(s) for s in slices[:q]) for q in range(W)]
    cand = candidates(rng_state, maxs, w_diff, gen)
    kept = [[] for _ in range(W)]  # per rank: (m, pose, key, global source)
    for m, (u, pose, _) in enumerate(cand):
        if pose is not None:
            kept[0].append((m, pose, pose_key(pose), -1))
            continue
        q = ipr.owner(u, edges)
        assert len(slices[q]) > 0, "CDF miss"
        i = find_local(u, edges[q], cdfs[q])
        p = [float(v) for v in slices[q][i, :3]]
        kept[q].append((m, p, pose_key(p), firsts[q] + i))
    # bin lists: distinct keys with the smallest draw index, per rank
    lists = []
    for q in range(W):
        first = {}
        for m, _, key, _ in kept[q]:
            first.setdefault(key, m)
        lists.append(sorted(first.items(), key=lambda kv: kv[1]))
    # merge: by key, the minimum draw index; then in first-draw order
    merged = {}
    for lst in lists:
        for key, t in lst:
            merged[key] = min(t, merged.get(key, t))
    order = sorted(merged.items(), key=lambda kv: kv[1])
    B = len(order)
    leaves = list(leaf_of_keys([kv[0] for kv in order]))
    M, leaf, bins, stopped, branch = stop_from_lists([kv[1] for kv in order], leaves, limit, maxs)
    new = [[p for m, p, _, _ in kept[q] if m < M] for q in range(W)]
    counts = [len(v) for v in new]
    owner = [None] * M
    source = [None] * M
    for q in range(W):
        for m, _, _, src in kept[q]:
            if m < M:
                owner[m], source[m] = q, src
    even = (M + W - 1) // W
    form = IN_PLACE if auto or not float(max(counts)) > max_share * float(even) else WINDOW
    return dict(M=M, leaf=leaf, bins=bins, counts=counts, form=form, owner=owner, source=source,
                slices=[np.array(v, dtype=np.float64).reshape(-1, 3) for v in new], rng=cand[M - 1][2],
                stopped=stopped, B=B, branch=branch, lists=lists)


def permutation(owner):
    """perm with concat(new slices) == S[perm]: the reference's draws 0 .. M - 1 sorted stably by owner."""
    return sorted(range(len(owner)), key=lambda m: (owner[m], m))


def owner_of_sources(source, cuts):
    """The rank that holds global source index g for contiguous cuts [c_0 = 0, ..., c_W]; random poses (-1): rank 0."""
    return [0 if g < 0 else bisect.bisect_right(cuts, g) - 1 for g in source]
