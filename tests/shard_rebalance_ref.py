"""Restatement of the rebalance of a sharded set (include/badger_pf.h, bpf_shard_rebalance_*;
badger_amcl_amd/csrc/shard_rebalance_plan.hpp): the plan from the W local counts alone, and numpy emulations of the
pack and assemble kernels.  No GPU, no engine."""
import numpy as np


def even_split(G, W):
    return [(G * (r + 1)) // W - (G * r) // W for r in range(W)]


def plan(counts):
    """dict(P, Q, keep_lo, keep_n, out, moved) for the local counts of every rank."""
    W = len(counts)
    if not 1 <= W <= 16 or any(c < 0 for c in counts):
        raise ValueError("rebalance plan: 1 .. 16 ranks, no negative count")
    P = [0]
    for c in counts:
        P.append(P[-1] + int(c))
    G = P[W]
    Q = [(G * r) // W for r in range(W + 1)]
    keep_lo, keep_n = [], []
    for r in range(W):
        lo, hi = max(P[r], Q[r]), min(P[r + 1], Q[r + 1])
        keep_lo.append(lo if hi > lo else P[r])
        keep_n.append(hi - lo if hi > lo else 0)
    out = [int(counts[r]) - keep_n[r] for r in range(W)]
    return dict(world=W, P=P, Q=Q, keep_lo=keep_lo, keep_n=keep_n, out=out, moved=sum(out))


def owner(pl, g):
    """The rank q with P[q] <= g < P[q + 1]."""
    q = 0
    for r in range(1, pl["world"]):
        if g >= pl["P"][r]:
            q = r
    return q


def source(pl, rank, g):
    """(owner, index): the local index in the old slice when the owner is `rank`, else the entry of the owner's
    outgoing list."""
    q = owner(pl, g)
    if q == rank:
        return q, g - pl["P"][q]
    if g < pl["keep_lo"][q]:
        return q, g - pl["P"][q]
    return q, g - pl["P"][q] - pl["keep_n"][q]


def pack(pl, rank, local):
    """k_rebalance_pack: rank's outgoing rows [4, out[rank]] (head span, then tail span) of its slice [n, 4]."""
    head = pl["keep_lo"][rank] - pl["P"][rank]
    kn = pl["keep_n"][rank]
    i = np.arange(pl["out"][rank])
    loc = np.where(i < head, i, i + kn)
    return np.ascontiguousarray(np.asarray(local).reshape(-1, 4)[loc].T)


def assemble(pl, rank, local, rows):
    """k_rebalance_assemble: rank's new slice [n_new, 4] from its old slice and every rank's packed rows."""
    first, n_new = pl["Q"][rank], pl["Q"][rank + 1] - pl["Q"][rank]
    new = np.zeros((n_new, 4))
    local = np.asarray(local).reshape(-1, 4)
    for o in range(n_new):
        q, j = source(pl, rank, first + o)
        new[o] = local[j] if q == rank else rows[q][:, j]
    return new


def rebalance(slices):
    """The whole thing on host arrays: (new slices, plan)."""
    pl = plan([np.asarray(s).reshape(-1, 4).shape[0] for s in slices])
    rows = [pack(pl, r, slices[r]) for r in range(pl["world"])]
    return [assemble(pl, r, slices[r], rows) for r in range(pl["world"])], pl


def brute_force(counts):
    """By enumeration of every global index: (out counts, for every rank the list of (owner, index) of its new slice)."""
    W, G = len(counts), sum(counts)
    old_owner = [r for r in range(W) for _ in range(counts[r])]
    old_local = [i for r in range(W) for i in range(counts[r])]
    new = even_split(G, W)
    new_owner = [r for r in range(W) for _ in range(new[r])]
    out_lists = [[g for g in range(G) if old_owner[g] == r and new_owner[g] != r] for r in range(W)]
    at = [{g: j for j, g in enumerate(o)} for o in out_lists]
    srcs = []
    for r in range(W):
        mine = []
        for g in range(G):
            if new_owner[g] != r:
                continue
            q = old_owner[g]
            mine.append((q, old_local[g]) if q == r else (q, at[q][g]))
        srcs.append(mine)
    return [len(o) for o in out_lists], srcs, out_lists
