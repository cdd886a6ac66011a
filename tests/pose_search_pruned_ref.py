"""numpy model of the pruned pose search (bpf_planar_search_poses_pruned): the block list with its members in CSR over
the strided free list, and the pooled LUT image P_B, separably and by its definition.  Shared by
tests/test_pose_search_pruned_cpu.py and tests/test_gpu_pose_search_pruned.py.

Definitions ("Pose search, pruned form"): block (bi, bj) of size B holds the cells with i // B ==
bi and j // B == bj; the block list holds the blocks with an entry of F_s, bi outer, bj inner; block candidate q =
block_index * H + h has the members c = f * H + h with F_s[f] in the block.  P_B lives on the padded image (padded u =
i + 1 in 0 .. size_x + 1, v likewise): entry (u, v) is the minimum code over the padded window W_x(u) x W_y(v), where
W(u) = [u - 1, u + B] for u <= size and W(size + 1) = [0, B + 1] + [size - B, size + 1] (the far border, where the
scoring kernel's clamp also sends every negative coordinate); padded cells outside the map hold the off-map code."""
import numpy as np

BLOCKS = (2, 4, 8, 16, 32, 64)


def block_list(ij, block):
    """(blocks[nb, 2] = (bi, bj) in list order, start[nb + 1], member[n] = indices into ij) of the free list ij[n, 2]"""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    bi, bj = ij[:, 0] // block, ij[:, 1] // block
    nbj = int(bj.max()) + 1 if ij.shape[0] else 1
    key = bi * nbj + bj
    member = np.argsort(key, kind="stable")
    keys, counts = np.unique(key, return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    blocks = np.stack([keys // nbj, keys % nbj], axis=1) if keys.shape[0] else np.zeros((0, 2), dtype=np.int64)
    return blocks, start, member


def members_of(start, member, headings, q):
    """candidates of block candidate q, ascending"""
    b, h = q // headings, q % headings
    return member[start[b]:start[b + 1]] * headings + h


def padded_codes(codes, off_code):
    """[size_y + 2, size_x + 2] padded image (row v, column u) of the real codes[size_y, size_x]"""
    sy, sx = codes.shape
    p = np.full((sy + 2, sx + 2), off_code, dtype=np.int64)
    p[1:sy + 1, 1:sx + 1] = codes
    return p


def window(u, size, block):
    """padded coordinates (inside 0 .. size + 1) of W(u)"""
    if u <= size:
        lo, hi = u - 1, u + block
        return [x for x in range(max(lo, 0), min(hi, size + 1) + 1)]
    near = list(range(0, min(block + 1, size + 1) + 1))
    far = list(range(max(size - block, 0), size + 2))
    return sorted(set(near + far))


def pooled_brute_entry(padded, block, u, v):
    """P_B(u, v) by its definition"""
    sy, sx = padded.shape[0] - 2, padded.shape[1] - 2
    us, vs = window(u, sx, block), window(v, sy, block)
    return int(padded[np.ix_(vs, us)].min())


def pooled(codes, off_code, block):
    """P_B as a padded [size_y + 2, size_x + 2] array: two passes of a sliding minimum, as the device forms it"""
    p = padded_codes(codes, off_code)
    hp, wp = p.shape

    def one_axis(a, size):
        # a: [n, size + 2], minimum along axis 1 over W
        ext = np.full((a.shape[0], size + 2 + block + 2), off_code, dtype=np.int64)
        ext[:, 1:size + 3] = a  # ext column x + 1 = padded x; column 0 = padded -1
        out = np.empty_like(a)
        acc = ext[:, 0:size + 2].copy()
        for d in range(1, block + 2):
            acc = np.minimum(acc, ext[:, d:d + size + 2])
        out[:] = acc  # out[:, u] = min ext[:, u .. u + B + 1] = padded u - 1 .. u + B
        near = a[:, 0:min(block + 1, size + 1) + 1].min(axis=1)
        far = a[:, max(size - block, 0):size + 2].min(axis=1)
        out[:, size + 1] = np.minimum(near, far)
        return out

    rows = one_axis(p, wp - 2)
    return one_axis(rows.T.copy(), hp - 2).T.copy()


def tile_shape(size_x, size_y):
    """(ltx, lty) of the engine's tiled image (bpf_map2d_set)"""
    return (size_x + 2 + 7) // 8 + 1, (size_y + 2 + 7) // 8


def tiled_index(u, v, ltx):
    """element index of padded (u, v) in the 8x8-tiled image: tile (v >> 3, u >> 3), cell (u & 7) * 8 + (v & 7)"""
    return ((v >> 3) * ltx + (u >> 3)) * 64 + ((u & 7) << 3) + (v & 7)


def to_tiles(padded, off_code):
    """the padded image in the tiled layout, the rest of the tiles holding the off-map code"""
    hp, wp = padded.shape
    ltx, lty = tile_shape(wp - 2, hp - 2)
    out = np.full(ltx * lty * 64, off_code, dtype=np.uint16)
    v, u = np.mgrid[0:hp, 0:wp]
    out[tiled_index(u, v, ltx)] = padded
    return out


def clamp_cell(c, size):
    """kernels_score.hpp clamp_cell: min((unsigned)c, size + 1)"""
    return min(c & 0xFFFFFFFF, size + 1)


WINDOW = 65536  # bpf_pose_search_window
SEED = 1024     # block candidates of the seed: the rows of the bound list


def replay(bounds, scores, start, member, headings, k, window=WINDOW, seed=SEED):
    """The pruned call's decisions replayed from its inputs: bounds[q] as bpf_planar_search_bounds returns them,
    scores[f, h] the exact scores of the candidates, the block list in CSR.  Returns the stats fields the call must
    report (all but `candidates`) and `best`, the scores of its hits.  The call is deterministic: the seed is the top
    `seed` of (bound descending, q ascending); tau is the k-th exact score once k are known; survivors are taken in
    index order; a survivor is decided in the window that holds its first member, against the tau before that
    window, and its members are folded window by window."""
    import pose_search_ref as psr
    bounds = np.asarray(bounds, dtype=np.float64)
    nq = bounds.shape[0]
    sizes = np.diff(start)
    size_q = np.repeat(sizes, headings)

    def member_scores(q):
        b, h = divmod(int(q), headings)
        return scores[member[start[b]:start[b + 1]], h]

    def fold(best, new):
        return np.sort(np.concatenate([best] + list(new)))[::-1][:k]

    def tau_of(best):
        return (True, best[k - 1]) if best.shape[0] >= k else (False, 0.0)

    seed_q = psr.order(bounds, np.arange(nq))[:min(seed, nq)]
    best = fold(np.zeros(0), [member_scores(q) for q in seed_q])
    seed_members = int(size_q[seed_q].sum())
    full, tau = tau_of(best)
    in_seed = np.zeros(nq, dtype=bool)
    in_seed[seed_q] = True
    surv = np.flatnonzero(~in_seed & ~(full & (bounds < tau)))
    first = np.concatenate([[0], np.cumsum(size_q[surv])]).astype(np.int64)
    total = int(first[-1])
    kept = np.zeros(surv.shape[0], dtype=bool)
    dropped = expanded = expanded_members = 0
    for lo in range(0, total, window):
        hi = min(lo + window, total)
        full, tau = tau_of(best)
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
                ms = member_scores(q)
                new.append(ms[max(lo - first[i], 0):min(hi - first[i], ms.shape[0])])
            i += 1
        best = fold(best, new)
    candidates = int(sizes.sum()) * headings
    seed_room = min(min(seed, nq) * int(sizes.max()), candidates) if nq else 0
    return dict(block_candidates=nq, seed_candidates=int(seed_q.shape[0]),
                pruned_block_candidates=nq - int(seed_q.shape[0]) - int(surv.shape[0]) + dropped,
                expanded_block_candidates=expanded, scored_candidates=seed_members + expanded_members,
                windows=-(-nq // window) + -(-seed_room // window) + -(-total // window), best=best)
