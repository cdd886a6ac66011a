"""Pure-Python restatement, in IEEE doubles, of the systematic resample of a sharded set in place
(include/badger_pf.h, bpf_shard_set_resample_form): the reference's serial target chain, i_wrap, the shards' slices of
the global CDF, the ownership counts, the rotation, and the imbalance cap.  Python floats are IEEE doubles and every
operation below is a single correctly rounded one, in the order the engine's host code performs it."""
import math

MASK48 = (1 << 48) - 1
WINDOW, IN_PLACE = 0, 1


def drand48_next(state):
    return (0x5DEECE66D * (state & MASK48) + 0xB) & MASK48


def target_chain(rng_state, n):
    """(targets of teeth 0 .. n - 1 in the reference's order, i_wrap, rng state after the one drand48).
    particle_filter.cpp:337-341: target += delta; if (target > 1.0) target -= 1.0.  i_wrap: the first tooth formed
    after the subtraction, n when there is none."""
    st = drand48_next(rng_state)
    t = math.ldexp(float(st), -48)
    delta = 1.0 / n
    out, i_wrap = [], n
    for i in range(n):
        out.append(t)
        t += delta
        if t > 1.0:
            t -= 1.0
            if i_wrap == n:
                i_wrap = i + 1
    return out, i_wrap, st


def ascending(targets, i_wrap):
    return targets[i_wrap:] + targets[:i_wrap]


def slice_edges(sums, sums_are_totals):
    """edge[q] .. edge[q + 1]: shard q's slice of the global CDF (shard_slice of kernels_pf.hpp): with weight totals
    the slice is total_q / T, with CDF sums the sums themselves, added left to right."""
    T = 1.0
    if sums_are_totals:
        T = 0.0
        for s in sums:
            T += s
    edges, off = [0.0], 0.0
    for s in sums:
        off += (s / T) if sums_are_totals else s
        edges.append(off)
    return edges


def owner(r, edges):
    """The shard whose ownership test (r >= offset and (r < top or last)) takes target r."""
    W = len(edges) - 1
    q = 0
    for k in range(1, W):
        if r >= edges[k]:
            q = k
    return q


def plan(rng_state, count, n_random, sums, sums_are_totals, max_share=2.0):
    """dict(targets, i_wrap, asc, counts, firsts, form): counts[q] = samples of rank q's new slice (rank 0's random
    poses included), firsts[q] its first global index, form = WINDOW when the cap applies."""
    W = len(sums)
    n = count - n_random
    targets, i_wrap, _ = target_chain(rng_state, n)
    asc = ascending(targets, i_wrap)
    assert all(b >= a for a, b in zip(asc, asc[1:]))
    edges = slice_edges(sums, sums_are_totals)
    counts = [0] * W
    for r in asc:
        counts[owner(r, edges)] += 1
    counts[0] += n_random
    firsts = [sum(counts[:q]) for q in range(W)]
    even = (count + W - 1) // W
    form = WINDOW if float(max(counts)) > max_share * float(even) else IN_PLACE
    return dict(targets=targets, i_wrap=i_wrap, asc=asc, counts=counts, firsts=firsts, form=form, edges=edges)


def rotate(new_set, n_random, i_wrap):
    """The in-place set from the single engine's: S[:n_random] + teeth[i_wrap:] + teeth[:i_wrap] (rows of an array or
    items of a list)."""
    head, teeth = new_set[:n_random], new_set[n_random:]
    if hasattr(new_set, "shape"):
        import numpy as np
        return np.concatenate([head, teeth[i_wrap:], teeth[:i_wrap]])
    return list(head) + list(teeth[i_wrap:]) + list(teeth[:i_wrap])
