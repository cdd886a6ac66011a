"""The pose search over a sharded filter without a GPU: the split of a range over the ranks, the merge of the ranks'
padded lists, the key map with its inverse, and the exactness of the shared floor on random bounds and scores
(tests/shard_search_ref.py; the device side is tests/test_gpu_shard_search.py)."""
import math
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_pruned_ref as ppr  # noqa: E402
import shard_search_ref as ssr  # noqa: E402

WORLDS = (1, 2, 3, 8, 16)


@pytest.mark.parametrize("W", WORLDS)
def test_split_covers_the_range_exactly_once(W):
    from badger_amcl_amd.sharded import even_counts
    for T in (0, 1, W - 1, W, W + 1, 65537):
        for first in (0, 5):
            parts = ssr.split(first, T, W)
            assert len(parts) == W
            at = first
            for lo, n in parts:
                assert lo == at and n >= 0
                at += n
            assert at == first + T
            assert [n for _, n in parts] == even_counts(T, W)  # the convention of the sample split
            assert max(n for _, n in parts) - min(n for _, n in parts) <= 1


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("W", WORLDS)
def test_merge_of_padded_lists_is_a_sort_of_the_union(W, k):
    rng = np.random.default_rng(100 * W + k)
    n = 40 * W
    # few distinct values, so that ties are decided by the candidate; NaNs and both zeros among them
    pool = np.array([0.0, -0.0, 1.5, -2.0, 1e-310, float("nan"), 7.25])
    scores = pool[rng.integers(0, pool.shape[0], n)]
    cands = rng.permutation(10 * n)[:n]
    cuts = sorted(rng.integers(0, n + 1, W - 1).tolist())  # some ranks hold nothing, some fewer than k
    lists, lo = [], 0
    for hi in cuts + [n]:
        lists.append(ssr.entries_of(scores[lo:hi], cands[lo:hi])[:k])
        lo = hi
    got = ssr.merge_lists(lists, k)
    want = ssr.entries_of(scores, cands)[:k]
    assert got == want
    # the order is the search's: score descending, equal scores by candidate ascending, NaN last
    dec = [(ssr.score_of(key), (~inv) & 0xFFFFFFFFFFFFFFFF) for key, inv in got]
    for (s0, c0), (s1, c1) in zip(dec[:-1], dec[1:]):
        if math.isnan(s0):
            assert math.isnan(s1) and c0 < c1
        elif not math.isnan(s1):
            assert s0 > s1 or (s0 == s1 and c0 < c1)


def test_key_decode_is_the_inverse_of_the_key_map():
    tiny = struct.unpack("<d", struct.pack("<Q", 1))[0]  # the smallest denormal
    values = [0.0, tiny, -tiny, 2.2250738585072014e-308, 1e-310, -1e-310, 1.0, -1.0, 1.7976931348623157e308,
              -1.7976931348623157e308, 0.1, -0.1, float("inf"), float("-inf")]
    for v in values:
        back = ssr.score_of(ssr.key_of(v))
        assert struct.pack("<d", back) == struct.pack("<d", v), v
    # -0.0 shares +0.0's key, a NaN maps to 0 and 0 decodes to a NaN
    assert ssr.key_of(-0.0) == ssr.key_of(0.0)
    assert struct.pack("<d", ssr.score_of(ssr.key_of(-0.0))) == struct.pack("<d", 0.0)
    assert ssr.key_of(float("nan")) == 0 and math.isnan(ssr.score_of(0))
    # key order is numeric order, and every number's key is above the NaN's
    ordered = sorted(set(values) | {0.0})
    keys = [ssr.key_of(v) for v in ordered]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and min(keys) > 0


def _random_case(rng, n_blocks, headings, tight):
    """a block list over n_blocks blocks of 1 .. 9 members, exact scores, and bounds at or above every member"""
    sizes = rng.integers(1, 10, n_blocks)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    member = rng.permutation(int(start[-1]))
    scores = rng.uniform(0.0, 1.0, (int(start[-1]), headings))
    # one good region, as a scan that fits one place gives
    good = rng.integers(0, n_blocks)
    scores[member[start[good]:start[good + 1]]] += 2.0
    best = np.maximum.reduceat(scores[member], start[:-1], axis=0).reshape(-1)
    slack = rng.uniform(0.0, 0.05 if tight else 1.0, best.shape[0])
    slack[rng.integers(0, best.shape[0], best.shape[0] // 4)] = 0.0  # bounds that are met
    return start, member, scores, best + slack


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("W", WORLDS)
def test_floor_replay_is_exact_and_the_floor_is_below_the_global_kth(W, k, tight):
    rng = np.random.default_rng(1000 * W + 10 * k + tight)
    headings, n_blocks = 3, 700
    start, member, scores, bounds = _random_case(rng, n_blocks, headings, tight)
    first_block, block_count = 3, n_blocks - 7
    members = np.concatenate([ppr.members_of(start, member, headings, q)
                              for q in range(first_block * headings, (first_block + block_count) * headings)])
    flat = scores.reshape(-1)
    want = np.sort(flat[members])[::-1][:k]
    # small windows and a small seed, so that the expansion runs over several windows and the seed leaves blocks out
    for shared in (True, False):
        ranks, floor = ssr.replay_world(bounds, scores, start, member, headings, k, first_block, block_count, W,
                                        shared=shared, window=256, seed=16)
        merged = np.sort(np.concatenate([r["best"] for r in ranks]))[::-1][:k]
        assert merged.tobytes() == want.tobytes(), (W, k, shared)
        if shared and floor is not None:
            assert floor <= want[k - 1]
        for r, (lo, n) in zip(ranks, ssr.split(first_block, block_count, W)):
            assert r["block_candidates"] == n * headings
            assert r["block_candidates"] == (r["seed_candidates"] + r["pruned_block_candidates"]
                                             + r["expanded_block_candidates"])


@pytest.mark.parametrize("k", [1, 64])
def test_replay_without_a_floor_is_the_single_engine_replay(k):
    rng = np.random.default_rng(77 + k)
    headings = 4
    start, member, scores, bounds = _random_case(rng, 300, headings, True)
    one = ppr.replay(bounds, scores, start, member, headings, k, window=256, seed=16)
    ranks, floor = ssr.replay_world(bounds, scores, start, member, headings, k, 0, 300, 1, shared=False, window=256,
                                    seed=16)
    for field, v in one.items():
        if field == "best":
            assert ranks[0]["best"].tobytes() == v.tobytes()
        else:
            assert ranks[0][field] == v, field
    # W = 1 with the floor: the floor is the rank's own tau behind the seed, which changes no decision
    shared, floor = ssr.replay_world(bounds, scores, start, member, headings, k, 0, 300, 1, shared=True, window=256,
                                     seed=16)
    assert {f: v for f, v in shared[0].items() if f != "best"} == {f: v for f, v in one.items() if f != "best"}


def test_a_rank_without_k_rows_or_with_a_nan_kth_sets_no_floor():
    start = np.array([0, 2, 4])
    member = np.arange(4)
    scores = np.array([[0.5], [float("nan")], [0.25], [0.125]])
    bounds = np.array([1.0, 1.0])
    r = ssr.RankReplay(bounds[:1], scores, start[:2], member, 1, 2)
    assert r.seed() is None  # two rows, the second a NaN
    r = ssr.RankReplay(bounds[:1], scores, start[:2], member, 1, 3)
    assert r.seed() is None  # fewer than k rows
    r = ssr.RankReplay(bounds[1:], scores, start[1:], member, 1, 2)
    assert r.seed() == 0.125
    assert ssr.floor_of([None, None]) is None and ssr.floor_of([None, 0.125, 0.5]) == 0.5
