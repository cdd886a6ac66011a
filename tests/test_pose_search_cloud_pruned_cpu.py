"""CPU checks of the numpy model behind the pruned cloud pose search (pose_search_cloud_pruned_ref.py): the pooling
windows against the scoring kernel's cell expression and BORDER clamp by enumeration, the block list of the rectangle
against scalar Python over free_cells_3d, and the separable P_B against its brute-force definition."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_check_ref as ref  # noqa: E402
import pose_search_cloud_pruned_ref as pcr  # noqa: E402
import pose_search_pruned_ref as ppr  # noqa: E402


# ------------------------------------------------------------------------------------ 1. the windows
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("block", [2, 4, 8, 16])
@pytest.mark.parametrize("size,min_c", [(13, -5), (5, 3), (40, -17)])
def test_a_members_cell_lies_in_the_anchors_window(size, min_c, block, exact):
    """x = v / res + 1.5 - min is what the kernel truncates (floors, in the other form) to cell - min + 1.  A member's
    x is the anchor's plus di in [0, B) plus an error below half a cell (the 2^-21 rule), so its cell is the anchor's
    + di - 1, + di or + di + 1.  For every anchor from 3 B below the map to 3 B above in quarter cells: a member that
    is on the map reads a cell of W(anchor's grid position); one that is off reads border_code, the smallest term."""
    span = size - 1
    checked = 0
    for quarter in range(-4 * 3 * block, 4 * (size + 3 * block) + 1):
        xa = 1.0 + quarter / 4.0  # on the map <=> 1 <= floor(x) <= size
        ga = pcr.border_clamp(pcr.voxel1(xa, exact), span)
        wa = set(ppr.window(ga, size, block))
        for di in range(block):
            for pert in (-1.0, -0.499, 0.0, 0.499, 1.0):
                # +-1 cell on the member's cell itself, and shifts of the coordinate just below half a cell
                xm = xa + di + (pert if abs(pert) < 1.0 else 0.0)
                c1 = pcr.voxel1(xm, exact)
                if abs(pert) == 1.0:
                    c1 = (pcr.voxel1(np.floor(xa) + di, exact) + int(pert)) & 0xFFFFFFFF
                gm = pcr.border_clamp(c1, span)
                if 1 <= gm <= size:
                    assert gm in wa, (xa, ga, di, pert, gm)
                    checked += 1
    assert checked > size * block


def test_grid_position_zero_and_the_wrap():
    """the exact form truncates: x in (-1, 1) gives grid position 0 (the cells min - 1 and, by truncation, min - 2);
    everything lower wraps to the far border span + 2, as everything above the map does"""
    span = 12
    assert pcr.border_clamp(pcr.voxel1(0.5, True), span) == 0
    assert pcr.border_clamp(pcr.voxel1(-0.5, True), span) == 0
    assert pcr.border_clamp(pcr.voxel1(-0.5, False), span) == span + 2
    assert pcr.border_clamp(pcr.voxel1(-1.0, True), span) == span + 2
    assert pcr.border_clamp(pcr.voxel1(span + 2.0, True), span) == span + 2
    assert pcr.border_clamp(pcr.voxel1(1e9, False), span) == span + 2
    assert pcr.border_clamp(pcr.voxel1(span + 1.9, True), span) == span + 1


# ------------------------------------------------------------------------------------ 2. the block list
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("mn,mx", [([-7, -9, 0], [6, 4, 3]), ([0, 0, 0], [11, 9, 2]), ([3, 5, -1], [17, 12, 1]),
                                   ([-20, -13, 0], [-4, -2, 1])])
@pytest.mark.parametrize("block", [2, 4])
def test_block_list_and_members_against_scalar_python(mn, mx, stride, block):
    """B = 2 is below stride 3 and equal to stride 2, B = 4 above every stride; bounds negative, zero, positive"""
    sp = pcr.Space(mn, mx, 0.05, 3, stride)
    cols = [(i, j) for (i, j) in ref.free_cells_3d(mn, mx) if i % stride == 0 and j % stride == 0]
    assert len(cols) == sp.columns
    want = {}
    for f, (i, j) in enumerate(cols):
        want.setdefault((i // block, j // block), []).append(f)  # floor division
    keys = sorted(want)  # bi outer, bj inner
    blocks, start, member = pcr.block_list(sp, block)
    assert [tuple(b) for b in blocks.tolist()] == keys
    assert start[-1] == sp.columns and sorted(member.tolist()) == list(range(sp.columns))
    for b, key in enumerate(keys):
        assert member[start[b]:start[b + 1]].tolist() == want[key], key
    # a member's column lies in [anchor, anchor + B) on both axes
    i, j, _, _ = sp.rows(member * sp.headings)
    ai, aj = np.repeat(blocks[:, 0] * block, np.diff(start)), np.repeat(blocks[:, 1] * block, np.diff(start))
    assert np.all((i >= ai) & (i < ai + block) & (j >= aj) & (j < aj + block))
    # block candidates: q = block * H + h
    q = 1 * sp.headings + 2
    assert ppr.members_of(start, member, sp.headings, q).tolist() == [f * sp.headings + 2 for f in want[keys[1]]]
    poses = pcr.anchor_poses(blocks, block, sp.res, sp.headings)
    assert poses[q, 0] == (keys[1][0] * block) * sp.res and poses[q, 1] == (keys[1][1] * block) * sp.res
    assert poses[q, 2] == (2.0 * np.pi * 2.0) / 3.0 - np.pi


# ------------------------------------------------------------------------------------ 3. the pooled volume
def _volume(seed=5, w=13, h=9, nz=3):
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 40, size=(nz, h, w)).astype(np.int64)
    vol[rng.random(vol.shape) < 0.5] = 255  # far from every obstacle
    return vol


@pytest.mark.parametrize("block", [2, 4, 16])
def test_pooled_volume_against_brute_force(block):
    """13 x 9 x 3: the windows of B = 2 and 4 are smaller than the map, that of B = 16 covers it"""
    vol = _volume()
    nz, h, w = vol.shape
    planes = pcr.pooled_planes(vol, block)
    assert planes.shape == (nz, h + 2, w + 2)
    for k in range(nz):
        for y in range(h + 2):
            for x in range(w + 2):
                assert planes[k, y, x] == pcr.pooled_brute_entry(vol[k], block, x, y), (k, x, y)
    assert (block + 2 > max(w, h)) == (block == 16)
    # no pooling over z: a plane depends on its own cells only
    other = vol.copy()
    other[1] = 255
    again = pcr.pooled_planes(other, block)
    assert np.array_equal(again[0], planes[0]) and np.array_equal(again[2], planes[2])
    # a corner window without an on-map cell holds the border code
    if block == 2:
        far = np.full_like(vol, 255)
        assert pcr.pooled_planes(far, block).max() == 255


def test_dense_layout_and_free_codes():
    vol = _volume()
    nz, h, w = vol.shape
    border, zero = pcr.free_codes(vol.reshape(-1))
    assert (border, zero) == (254, 253)
    planes = pcr.pooled_planes(vol, 4)
    planes[0, 0, 0] = pcr.INF
    out, ntx, nty = pcr.to_dense(planes, border, zero)
    assert (ntx, nty) == (2, 2) and out.shape[0] == (nz + 1) * ntx * nty * 64
    plane = ntx * nty * 64
    assert out[0] == border and np.all(out[nz * plane:] == zero)
    assert out[1 * plane + pcr.dense_offset(5, 9, ntx)] == planes[1, 9, 5]
    assert out[1 * plane + pcr.dense_offset(15, 3, ntx)] == border  # beyond the grid positions in use
    assert pcr.dense_offset(5, 9, ntx) == 8 * 5 + 9 + (8 * ntx - 1) * (9 & ~7)  # the kernel's form of the offset
    assert pcr.free_codes(np.arange(256)) == (-1, -1)
