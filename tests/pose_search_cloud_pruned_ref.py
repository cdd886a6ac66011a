"""numpy model of the pruned pose search with the cloud scanner (bpf_cloud_search_poses_pruned): the block list of the
rectangle C_s by arithmetic (floor division, bounds of either sign), the pooled volume P_B by its definition and
separably, the dense layout, the kernel's cell expression with its BORDER clamp, and the replay of the call's
decisions.  Shared by tests/test_pose_search_cloud_pruned_cpu.py and tests/test_gpu_pose_search_cloud_pruned.py.

Definitions ("Pose search, pruned 3-D form"): block (bi, bj) of size B holds the columns of C_s
with i // B == bi and j // B == bj (Python's floor division); the block list holds the blocks with a column of C_s, bi
outer, bj inner; block candidate q = block_index * H + h has the members c = f * H + h whose column f lies in the
block, f ascending.  P_B lives on the grid positions of the dense volume (x = i - min_i + 1 in 0 .. w + 1, y likewise,
one plane per z cell): entry (x, y, k) is the smallest ratio of the on-map cells of W(x) x W(y) in plane k, or
border_code when there is none, with W(g) = [g - 1, g + B] for g <= size and W(size + 1) = [0, B + 1] + [size - B,
size + 1] -- the far border, where the kernel's clamp min(c1, span + 2) also sends what wraps below grid position 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_search_pruned_ref as ppr  # noqa: E402
from pose_search_cloud_ref import Space  # noqa: E402,F401

BLOCKS = ppr.BLOCKS
INF = 256  # "above every ratio": what border_code counts as inside the minimum


# ------------------------------------------------------------------------------------ the block list
def block_axis(first, n, stride, block):
    """(block indices holding a column first + a * stride, a < n, ascending; start[nb + 1] into a)"""
    idx, start = [], []
    for a in range(n):
        b = (first + a * stride) // block
        if not idx or idx[-1] != b:
            idx.append(b)
            start.append(a)
    start.append(n)
    return np.array(idx, dtype=np.int64), np.array(start, dtype=np.int64)


def block_list(sp, block):
    """(blocks[nb, 2] = (bi, bj) in list order, start[nb + 1], member[columns] = indices f into C_s) of the Space sp:
    the product of the two axes, a block's members with a outer and b inner (f = a * n_j + b ascending)"""
    bi, ai = block_axis(sp.i0, sp.n_i, sp.stride, block)
    bj, aj = block_axis(sp.j0, sp.n_j, sp.stride, block)
    blocks, start, member = [], [0], []
    for ib in range(bi.shape[0]):
        for jb in range(bj.shape[0]):
            a = np.arange(ai[ib], ai[ib + 1])[:, None]
            b = np.arange(aj[jb], aj[jb + 1])[None, :]
            f = (a * sp.n_j + b).reshape(-1)
            blocks.append((bi[ib], bj[jb]))
            member.append(f)
            start.append(start[-1] + f.shape[0])
    blocks = np.array(blocks, dtype=np.int64).reshape(-1, 2)
    member = np.concatenate(member).astype(np.int64) if member else np.zeros(0, dtype=np.int64)
    return blocks, np.array(start, dtype=np.int64), member


def anchor_poses(blocks, block, res, headings):
    """[nb * H, 3] anchor poses in q order: the column (bi * B, bj * B) by the cell expression of the search"""
    nb = blocks.shape[0]
    poses = np.empty((nb * headings, 3), dtype=np.float64)
    h = np.tile(np.arange(headings, dtype=np.float64), nb)
    poses[:, 0] = np.repeat((blocks[:, 0] * block).astype(np.float64) * res, headings)
    poses[:, 1] = np.repeat((blocks[:, 1] * block).astype(np.float64) * res, headings)
    poses[:, 2] = (2.0 * np.pi * h) / float(headings) - np.pi
    return poses


# ------------------------------------------------------------------------------------ the volume
def free_codes(distance_ratios):
    """(border_code, zero_code): the two highest ratios no entry of the LUT holds, or (-1, -1)"""
    used = np.zeros(256, dtype=bool)
    used[np.asarray(distance_ratios, dtype=np.uint8)] = True
    free = [c for c in range(255, -1, -1) if not used[c]][:2]
    return (free[0], free[1]) if len(free) == 2 else (-1, -1)


def ratios_volume(pose_indices, distance_ratios, w, h, nz):
    """[nz, h, w] true ratios of the two-level LUT (plane k, row j, column i; column index j * w + i)"""
    pi = np.asarray(pose_indices, dtype=np.int64).reshape(h, w)
    dr = np.asarray(distance_ratios, dtype=np.int64)
    return np.stack([dr[pi + k] for k in range(nz)], axis=0)


def tile_shape(w, h):
    """(ntx, nty) of a plane of the dense volume (bpf_map3d_set)"""
    return (w + 2 + 7) // 8, (h + 2 + 7) // 8


def dense_offset(x, y, ntx):
    """byte offset of grid position (x, y) in a plane: tile (y >> 3, x >> 3), cell (x & 7) * 8 + (y & 7)"""
    return ((y >> 3) * ntx + (x >> 3)) * 64 + ((x & 7) << 3) + (y & 7)


def pooled_brute_entry(vol_k, block, x, y):
    """P_B(x, y) of one plane vol_k[h, w] by its definition; INF when the window holds no on-map cell"""
    h, w = vol_k.shape
    padded = ppr.padded_codes(vol_k, INF)
    xs, ys = ppr.window(x, w, block), ppr.window(y, h, block)
    return int(padded[np.ix_(ys, xs)].min())


def pooled_planes(vol, block):
    """[nz, h + 2, w + 2] P_B on the grid positions, INF for "no on-map cell": two sliding minima per plane"""
    return np.stack([ppr.pooled(vol[k], INF, block) for k in range(vol.shape[0])], axis=0)


def to_dense(planes, border_code, zero_code):
    """the grid planes [nz, h + 2, w + 2] (INF = border) as the bytes of the dense layout: nz planes whose remaining
    entries hold border_code, and the zero plane behind them"""
    nz, hp, wp = planes.shape
    ntx, nty = tile_shape(wp - 2, hp - 2)
    plane = ntx * nty * 64
    out = np.full((nz + 1) * plane, border_code, dtype=np.uint8)
    out[nz * plane:] = zero_code
    y, x = np.mgrid[0:hp, 0:wp]
    off = dense_offset(x, y, ntx)
    for k in range(nz):
        out[k * plane + off] = np.where(planes[k] >= INF, border_code, planes[k]).astype(np.uint8)
    return out, ntx, nty


# ------------------------------------------------------------------------------------ the kernel's cell expression
def voxel1(x, exact):
    """k_cloud_score's cell - min + 1 as an unsigned 32-bit value, from x = v / res + 1.5 - min: by truncation in the
    exact-reciprocal form (voxel1_exact), by floor in the other (voxel_rel + 1)"""
    c = int(np.trunc(x)) if exact else int(np.floor(x))
    return c & 0xFFFFFFFF


def border_clamp(c1, span):
    """cell_xy, BORDER: min(c1, span + 2) on unsigned values"""
    return min(c1, span + 2)


# ------------------------------------------------------------------------------------ the call's decisions
def replay(bounds, scores, start, member, headings, k):
    """every stats field but `candidates`, and the hits' scores: the planar replay over this block list (the call is
    the same one: seed, tau, survivors in index order, expansion windows)"""
    return ppr.replay(bounds, scores, start, member, headings, k)
