"""The restatement of the in-place systematic resample (shard_in_place_ref.py) against the CPU oracle's systematic
resampler, with no GPU: rotating the oracle's new set by the model's i_wrap gives the set the model builds tooth by
tooth in ascending-target order; the oracle's stream position is the model's; the ownership counts add up, follow the
shards' slices of the CDF and send every tooth to the shard that holds its source particle; the cap and the binding's
symbols."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import shard_in_place_ref as ipr  # noqa: E402


def cloud(n, seed, spread):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    s[:, 0] = rng.normal(1.0, spread, n)
    s[:, 1] = rng.normal(-2.0, spread, n)
    s[:, 2] = rng.uniform(-np.pi, np.pi, n)
    w = rng.random(n) ** 3 + 1e-3
    s[:, 3] = w / w.sum()
    return s


def model_source_indices(weights, asc):
    """The single engine's CDF search for every ascending target: c[i] <= r < c[i + 1] on the running sum."""
    c = [0.0]
    for w in weights:
        c.append(c[-1] + float(w))
    return [int(np.searchsorted(c, r, side="right")) - 1 for r in asc], c


@pytest.mark.parametrize("n,seed,spread", [(3, 1, 0.1), (255, 2, 0.1), (257, 3, 5.0), (1200, 4, 0.05), (4097, 5, 8.0)])
def test_rotating_the_oracles_set_gives_the_models(orc, n, seed, spread):
    s = cloud(n, seed, spread)
    opf = orc.ParticleFilter(2, n, 0.0, 0.0, 85.0, seed=seed)
    opf.set_resample_model(orc.RESAMPLE_SYSTEMATIC)
    opf.set_samples(s)
    opf.pf.w_slow = opf.pf.w_fast = 1.0  # w_diff = 0 (straight after a set_samples the reference's 1 - 0 / 0 is NaN)
    rng0 = opf.pf.rng
    count = opf.resample_limit(opf.leaf_count)
    out = opf.update_resample()
    assert out.sample_count == count and out.w_diff == 0.0 and out.status == 0
    targets, i_wrap, st = ipr.target_chain(rng0, count)
    assert opf.pf.rng == st
    asc = ipr.ascending(targets, i_wrap)
    assert all(b > a for a, b in zip(asc, asc[1:])) and 0.0 <= asc[0] and asc[-1] <= 1.0
    assert i_wrap == count or targets[i_wrap] < targets[i_wrap - 1]
    idx, cdf = model_source_indices(s[:, 3], asc)
    assert max(idx) < n
    want = s[idx, :3]
    got = ipr.rotate(opf.samples[:count], 0, i_wrap)
    assert np.array_equal(got[:, :3], want)
    assert np.array_equal(ipr.rotate(opf.last_idx, 0, i_wrap), np.array(idx))
    assert np.all(got[:, 3] == 1.0 / count)
    # ownership: for any contiguous split, with the shards' CDF sums as the engine gathers them
    for W, cuts in [(1, [0, n]), (2, [0, n // 2, n]), (3, [0, n // 3, n // 3, n]),
                    (8, [(n * r) // 8 for r in range(9)])]:
        sums = []
        for q in range(W):
            acc = 0.0
            for w in s[cuts[q]:cuts[q + 1], 3]:
                acc += float(w)
            sums.append(acc)
        P = ipr.plan(rng0, count, 0, sums, False, max_share=float(W))
        assert P["form"] == ipr.IN_PLACE and sum(P["counts"]) == count and P["i_wrap"] == i_wrap
        at = 0
        for q in range(W):
            mine = idx[at:at + P["counts"][q]]
            # a tooth within rounding of a slice border may sit one particle across it; none does for these seeds
            assert all(cuts[q] <= i < cuts[q + 1] for i in mine), (W, q)
            at += P["counts"][q]


def test_wrap_positions_and_the_chain():
    # u0 + (n - 1) / n < 1 <=> no wrap; the first wrapped tooth is the smallest target
    for state, n in [(0, 7), (123456789, 100), ((1 << 48) - 1, 5), (0x1234ABCD5678, 4097)]:
        t, i_wrap, st = ipr.target_chain(state, n)
        assert st == ipr.drand48_next(state) and len(t) == n and t[0] == st / 2.0 ** 48
        asc = ipr.ascending(t, i_wrap)
        assert sorted(t) == asc
        if i_wrap < n:
            assert t[i_wrap] == min(t) and t[i_wrap - 1] == max(t)
        else:
            assert t == asc


def test_slices_cap_and_empty_shards():
    # all weight on one particle of the middle rank: every tooth is its, the others empty out
    P = ipr.plan(42, 100, 0, [0.0, 1.0, 0.0], False, max_share=3.0)
    assert P["counts"] == [0, 100, 0] and P["firsts"] == [0, 0, 100] and P["form"] == ipr.IN_PLACE
    assert ipr.plan(42, 100, 0, [0.0, 1.0, 0.0], False)["form"] == ipr.WINDOW  # 100 > 2 * ceil(100 / 3)
    # totals: the slice is total_q / T
    P = ipr.plan(7, 1000, 0, [3.0, 1.0, 0.0, 4.0], True)
    assert P["edges"] == [0.0, 0.375, 0.5, 0.5, 1.0] and P["counts"][2] == 0 and sum(P["counts"]) == 1000
    assert abs(P["counts"][0] - 375) <= 1 and abs(P["counts"][3] - 500) <= 1
    # the random poses of w_diff > 0 sit at rank 0's head
    P = ipr.plan(7, 1000, 100, [1.0, 1.0], True)
    assert sum(P["counts"]) == 1000 and abs(P["counts"][0] - 550) <= 1 and P["firsts"] == [0, P["counts"][0]]
    # a target of exactly 1.0 (beyond the CDF) belongs to the last shard
    assert ipr.owner(1.0, [0.0, 0.5, 1.0]) == 1 and ipr.owner(0.5, [0.0, 0.5, 1.0]) == 1
    assert ipr.owner(0.0, [0.0, 0.0, 1.0]) == 1  # an empty first shard owns nothing
    assert ipr.rotate(list(range(10)), 2, 3) == [0, 1, 5, 6, 7, 8, 9, 2, 3, 4]


def test_the_binding_declares_the_in_place_calls():
    from badger_amcl_amd import _lib, sharded
    for name in ("bpf_shard_set_resample_form", "bpf_shard_get_resample_form", "bpf_shard_slice",
                 "bpf_shard_inplace_select_dev", "bpf_shard_inplace_xy_sums_dev", "bpf_shard_inplace_converged_dev",
                 "bpf_shard_inplace_converged_finish"):
        assert name in _lib.SIGNATURES
    assert (sharded.RESAMPLE_WINDOW, sharded.RESAMPLE_IN_PLACE) == (ipr.WINDOW, ipr.IN_PLACE)
