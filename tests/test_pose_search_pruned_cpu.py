"""The numpy model of the pruned pose search (pose_search_pruned_ref.py) against the definitions it restates: the
pooled image by brute force, the windows against the scoring kernel's truncation and clamp, the block members as a
partition of the candidate space, and the layout of the stats struct in the Python binding."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_pruned_ref as ppr  # noqa: E402

MAPS = {"wide": (37, 21), "narrow": (8, 70)}  # (size_x, size_y): the second is narrower than most B
N_LEVELS = 23


def random_codes(name, seed=5):
    sx, sy = MAPS[name]
    rng = np.random.default_rng(seed)
    levels = rng.integers(0, N_LEVELS, size=(sy, sx))
    # low levels rare, so that a window's minimum is decided by few cells and a wrong window shows
    levels = np.maximum(levels, rng.integers(0, N_LEVELS, size=(sy, sx)))
    return levels.astype(np.int64) * 8, N_LEVELS * 8


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("block", ppr.BLOCKS)
def test_pooled_image_is_its_definition(name, block):
    codes, off = random_codes(name)
    sx, sy = MAPS[name]
    P = ppr.pooled(codes, off, block)
    assert P.shape == (sy + 2, sx + 2)
    brute = np.array([[ppr.pooled_brute_entry(ppr.padded_codes(codes, off), block, u, v) for u in range(sx + 2)]
                      for v in range(sy + 2)])
    assert np.array_equal(P, brute)
    # both borders and the far-border wrap, spelled out for one row / column
    pad = ppr.padded_codes(codes, off)
    v = min(3, sy)
    rows = slice(max(v - 1, 0), min(v + block, sy + 1) + 1)
    assert P[v, 0] == pad[rows, 0:min(block, sx + 1) + 1].min()
    far = np.concatenate([pad[rows, 0:min(block + 1, sx + 1) + 1], pad[rows, max(sx - block, 0):sx + 2]], axis=1)
    assert P[v, sx + 1] == far.min()
    assert P[sy + 1, sx + 1] <= min(pad[1, 1], pad[sy, sx], pad[1, sx], pad[sy, 1])  # all four corners of the map
    assert P.max() <= off and np.all(P <= pad)


@pytest.mark.parametrize("size", [8, 21, 37, 70])
@pytest.mark.parametrize("block", ppr.BLOCKS)
def test_windows_cover_what_a_member_can_reach(size, block):
    """An anchor's end point a (in padded cell units, before truncation) and a member's a + d + eps, d in 0 .. B - 1,
    |eps| tiny: the member's padded cell trunc(.) is off the map or inside the window of the anchor's clamped cell."""
    rng = np.random.default_rng(size * 100 + block)
    a = np.concatenate([rng.uniform(-3.0 * block - 5, size + 3.0 * block + 5, 4000),
                        np.arange(-block - 3, size + block + 4).astype(np.float64),  # integers: the ties of truncation
                        np.arange(-block - 3, size + block + 4) + 1.0 - 1e-12])
    for av in a:
        anchor = ppr.clamp_cell(int(math.trunc(av)), size)
        win = set(ppr.window(anchor, size, block))
        for d in range(block):
            for eps in (-1e-9, 0.0, 1e-9):
                cell = ppr.clamp_cell(int(math.trunc(av + d + eps)), size)
                on_map = 1 <= cell <= size
                assert (not on_map) or cell in win, (av, d, eps, anchor, cell)


def test_tiled_layout_matches_the_kernels_offset():
    """element index = byte offset / 2 of kernels_score.hpp: 16 u + 2 v + (16 ltx - 2) (v & ~7)"""
    for sx, sy in MAPS.values():
        ltx, lty = ppr.tile_shape(sx, sy)
        v, u = np.mgrid[0:sy + 2, 0:sx + 2]
        assert np.array_equal(ppr.tiled_index(u, v, ltx) * 2, 16 * u + 2 * v + (16 * ltx - 2) * (v & ~7))
        assert ppr.tiled_index(u, v, ltx).max() < ltx * lty * 64
        codes, off = random_codes("wide" if (sx, sy) == MAPS["wide"] else "narrow")
        P = ppr.pooled(codes, off, 4)
        tiles = ppr.to_tiles(P, off)
        assert tiles.shape[0] == ltx * lty * 64
        assert np.array_equal(tiles[ppr.tiled_index(u, v, ltx)], P)
        assert np.count_nonzero(tiles != off) <= (sx + 2) * (sy + 2)


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_members_partition_the_candidate_space(name, stride):
    sx, sy = MAPS[name]
    rng = np.random.default_rng(11)
    free = rng.random((sx, sy)) < 0.6
    ij = np.array([(i, j) for i in range(0, sx, stride) for j in range(0, sy, stride) if free[i, j]], dtype=np.int64)
    headings = 5
    for block in ppr.BLOCKS:
        blocks, start, member = ppr.block_list(ij, block)
        nb = blocks.shape[0]
        assert start[0] == 0 and start[-1] == ij.shape[0] and np.all(np.diff(start) > 0)
        # bi outer, bj inner; every block non-empty and distinct
        order = blocks[:, 0] * (sy + 1) + blocks[:, 1]
        assert np.all(np.diff(order) > 0)
        seen = np.concatenate([ppr.members_of(start, member, headings, q) for q in range(nb * headings)])
        assert np.array_equal(np.sort(seen), np.arange(ij.shape[0] * headings))
        for b in range(nb):
            cells = ij[member[start[b]:start[b + 1]]]
            assert np.all(cells // block == blocks[b])
            assert np.all(np.diff(member[start[b]:start[b + 1]]) > 0)  # ascending inside a block
        if block > max(sx, sy):
            assert nb == 1


def test_stats_struct_and_block_list_of_the_binding():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    names = [n for n, _ in _lib.PoseSearchStats._fields_]
    assert names == ["candidates", "block_candidates", "seed_candidates", "pruned_block_candidates",
                     "expanded_block_candidates", "scored_candidates", "windows"]
    assert all(t is C.c_longlong for _, t in _lib.PoseSearchStats._fields_)
    assert C.sizeof(_lib.PoseSearchStats) == 7 * 8
    assert [getattr(_lib.PoseSearchStats, n).offset for n in names] == [8 * k for k in range(7)]
    assert hpf.POSE_SEARCH_BLOCKS == ppr.BLOCKS == (2, 4, 8, 16, 32, 64)
    assert hpf.POSE_SEARCH_BLOCK in hpf.POSE_SEARCH_BLOCKS
    assert hpf.POSE_SEARCH_STATS_FIELDS == tuple(names)
    # the header declares the same fields in the same order
    header = open(os.path.join(os.path.dirname(HERE), "include", "badger_pf.h")).read()
    body = header[header.index("long long candidates;"):header.index("} bpf_pose_search_stats;")]
    import re
    assert re.findall(r"long long (\w+);", body) == names


@pytest.mark.parametrize("k", [1, 7, 300])
def test_replay_keeps_the_top_k_and_its_accounts_add_up(k):
    """the replay of the call's decisions (the GPU test holds the device's stats to it) on random scores with bounds
    that hold: the best k survive, small windows and a small seed so that every path is taken"""
    rng = np.random.default_rng(k)
    sx, sy, headings, block = 37, 21, 3, 4
    free = rng.random((sx, sy)) < 0.7
    ij = np.array([(i, j) for i in range(sx) for j in range(sy) if free[i, j]], dtype=np.int64)
    blocks, start, member = ppr.block_list(ij, block)
    scores = rng.random((ij.shape[0], headings)) ** 4
    best_member = np.maximum.reduceat(scores[member], start[:-1], axis=0).reshape(-1)
    bounds = best_member + rng.random(best_member.shape[0]) * 0.3
    out = ppr.replay(bounds, scores, start, member, headings, k, window=50, seed=5)
    assert np.array_equal(out["best"], np.sort(scores.reshape(-1))[::-1][:k])
    assert out["block_candidates"] == blocks.shape[0] * headings == (
        out["seed_candidates"] + out["pruned_block_candidates"] + out["expanded_block_candidates"])
    assert out["seed_candidates"] == 5 and out["scored_candidates"] <= scores.size
    assert out["pruned_block_candidates"] > 0 and out["expanded_block_candidates"] > 0
    loose = ppr.replay(np.full_like(bounds, 2.0), scores, start, member, headings, k, window=50, seed=5)
    assert loose["pruned_block_candidates"] == 0 and loose["scored_candidates"] == scores.size
