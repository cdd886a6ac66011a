"""The restatement of the in-place multinomial resample (shard_in_place_mn_ref.py) against the CPU oracle, with no GPU:
the stop count, the leaf and bin counts at the stop and the stream state are the oracle's, and the concatenation of the
ranks' new slices is the oracle's set S[0:M] sorted stably by the owner of each draw.  Both kld_count modes, uneven
cuts, empty and one-sample shards, and the recovery draws (w_diff > 0) for K = 0 and K = 4 rejected trials."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kld_bins_ref as kbr  # noqa: E402
import pose_check_ref as pcr  # noqa: E402
import shard_in_place_mn_ref as mnr  # noqa: E402
from badger_amcl_amd import synth  # noqa: E402



def cloud(kind, n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4))
    if kind == "blob":
        s[:, 0], s[:, 1] = rng.normal(1.0, 0.15, n), rng.normal(-2.0, 0.15, n)
        s[:, 2] = rng.normal(0.3, 0.05, n)
    elif kind == "mixture":
        c = rng.integers(0, 3, n)
        s[:, 0] = np.array([1.0, -6.0, 9.0])[c] + rng.normal(0, 0.3, n)
        s[:, 1] = np.array([-2.0, 4.0, 0.5])[c] + rng.normal(0, 0.3, n)
        s[:, 2] = np.array([0.3, -2.0, 1.5])[c] + rng.normal(0, 0.1, n)
    else:
        s[:, 0], s[:, 1] = rng.uniform(-40, 40, n), rng.uniform(-40, 40, n)
        s[:, 2] = rng.uniform(-np.pi, np.pi, n)
    w = rng.random(n) ** 3 + 1e-3
    s[:, 3] = w / w.sum()
    return s


def cuts_for(n, W, style):
    if style == "even":
        return [(n * r) // W for r in range(W + 1)]
    if style == "empty":       # one empty shard in the middle (or the only cut there is)
        c = [(n * r) // max(W - 1, 1) for r in range(W)]
        return c[:W // 2 + 1] + c[W // 2:] if W > 1 else [0, n]
    if style == "tiny":        # 1- to 7-sample shards in front
        c = [0]
        for r in range(W - 1):
            c.append(c[-1] + 1 + 3 * r)
        return c + [n]
    raise ValueError(style)


def serial_sums(s, cuts):
    sums = []
    for q in range(len(cuts) - 1):
        acc = 0.0
        for w in s[cuts[q]:cuts[q + 1], 3]:
            acc += float(w)
        sums.append(acc)
    return sums


def leaf_fn(orc, mode):
    def leaves(keys):
        t = orc.KDTree()
        out = []
        for k in keys:
            t.insert_key(list(k), 1.0)
            out.append(kbr.tree_count(t, mode))
        return out
    return leaves


def check(orc, s, cuts, maxs, min_samples, seed, mode, want_poses, want_M, want_leaf, want_nodes, want_rng, rng0,
          w_diff=0.0, gen=None):
    opf = orc.ParticleFilter(min_samples, maxs, 0.0, 0.0, 85.0, seed=seed)
    slices = [s[cuts[q]:cuts[q + 1]] for q in range(len(cuts) - 1)]
    R = mnr.resample(slices, serial_sums(s, cuts), False, rng0, maxs, opf.resample_limit, leaf_fn(orc, mode),
                     w_diff=w_diff, gen=gen, max_share=float(len(slices)))
    assert R["M"] == want_M
    assert R["leaf"] == (want_leaf if mode == kbr.LEAVES else want_nodes)
    assert R["bins"] == want_nodes
    assert R["rng"] == want_rng
    assert sum(R["counts"]) == want_M and R["form"] == mnr.IN_PLACE
    perm = mnr.permutation(R["owner"])
    got = np.concatenate(R["slices"])
    assert np.array_equal(got, np.asarray(want_poses)[perm])
    # the owner of a draw is the rank that holds its source particle
    assert R["owner"] == mnr.owner_of_sources(R["source"], cuts)
    return R


CASES = [("blob", 3000, 100, 11), ("blob", 600, 5, 12), ("mixture", 2000, 50, 13), ("mixture", 5000, 100, 14),
         ("spread", 600, 20, 15), ("spread", 3000, 100, 16)]


@pytest.mark.parametrize("kind,n,min_samples,seed", CASES)
@pytest.mark.parametrize("W,style", [(1, "even"), (2, "even"), (3, "tiny"), (4, "empty"), (5, "tiny"), (3, "empty")])
def test_the_models_set_is_the_oracles_permuted(orc, kind, n, min_samples, seed, W, style):
    s = cloud(kind, n, seed)
    opf = orc.ParticleFilter(min_samples, n, 0.0, 0.0, 85.0, seed=seed)
    opf.set_samples(s)
    opf.pf.w_slow = opf.pf.w_fast = 1.0  # w_diff = 0
    rng0 = int(opf.pf.rng)
    out = opf.update_resample()
    assert out.status == 0 and out.w_diff == 0.0
    M = out.sample_count
    R = check(orc, s, cuts_for(n, W, style), n, min_samples, seed, kbr.LEAVES, opf.samples[:M, :3], M, out.leaf_count,
              out.node_count, int(opf.pf.rng), rng0)
    assert int(opf.pf.rng) == pcr.skip(rng0, 2 * M)
    if R["stopped"]:
        assert M < n


@pytest.mark.parametrize("kind,n,min_samples,seed", [("blob", 3000, 100, 21), ("mixture", 2000, 50, 22),
                                                     ("spread", 1500, 20, 23)])
@pytest.mark.parametrize("W,style", [(1, "even"), (3, "tiny"), (4, "empty")])
def test_bins_mode(orc, kind, n, min_samples, seed, W, style):
    s = cloud(kind, n, seed)
    opf = orc.ParticleFilter(min_samples, n, 0.0, 0.0, 85.0, seed=seed)
    rng0 = int(opf.pf.rng)
    r = kbr.Rng(rng0)
    want, count, leaf, nodes, _ = kbr.resample(s, 0, 0.0, r, None, 0, opf, orc.KDTree, kbr.BINS)
    assert count == nodes
    check(orc, s, cuts_for(n, W, style), n, min_samples, seed, kbr.BINS, want, len(want), leaf, nodes, r.s, rng0)


@pytest.mark.parametrize("g0,m,K", [(0.0, 0.5, 0), (10.0, 0.5, 4)])
@pytest.mark.parametrize("kind,n,min_samples,seed,w_diff", [("blob", 2000, 100, 31, 0.1), ("mixture", 1500, 50, 32, 0.3),
                                                            ("spread", 800, 20, 33, 0.05)])
@pytest.mark.parametrize("W,style", [(2, "even"), (3, "tiny"), (4, "empty")])
def test_recovery(orc, g0, m, K, kind, n, min_samples, seed, w_diff, W, style):
    cells, origin = synth.make_map(60, 0.05)
    omap = orc.OccupancyMap(cells, 0.05, origin)
    lut = omap.update_distances_lut(1.0)
    fs = pcr.FreeSpace.planar(pcr.free_cells_2d(cells, lut, 0.3), 60, 60, origin, 0.05)
    assert pcr.retries(g0, m) == K
    s = cloud(kind, n, seed)
    opf = orc.ParticleFilter(min_samples, n, 0.0, 0.0, 85.0, seed=seed)
    rng0 = int(opf.pf.rng)
    r = pcr.Rng(rng0)
    want, leaf, nodes, rnd = pcr.resample(s, 0, w_diff, r, pcr.FastGen(fs, g0, m), 0, opf, orc.KDTree)
    assert any(rnd) and not all(rnd)
    R = check(orc, s, cuts_for(n, W, style), n, min_samples, seed, kbr.LEAVES, want, len(want), leaf, nodes, r.s, rng0,
              w_diff=w_diff, gen=pcr.FastGen(fs, g0, m))
    # the random poses sit on rank 0, in draw order
    assert [o for o, is_r in zip(R["owner"], rnd) if is_r] == [0] * sum(rnd)


def test_the_stop_formula_on_hand_made_lists():
    """Both branches of c_j = max(t_j + 1, limit(L_j) + 1), and no stop."""
    lim = {1: 100, 2: 10, 3: 30, 4: 6}.get
    run = mnr.stop_from_lists
    assert run([0, 5], [1, 2], lim, 50) == (11, 2, 2, True, "limit")         # 10 draws allowed with 2 leaves
    assert run([0, 5, 8], [1, 2, 3], lim, 50) == (31, 3, 3, True, "limit")   # key 2 arrives before 11: the bound grows
    # the bound FALLS to 6 with key 3 at draw 20: the draw that adds it is the last one (the t_j + 1 branch)
    assert run([0, 5, 8, 20], [1, 2, 3, 4], lim, 50) == (21, 4, 4, True, "insert")
    assert run([0, 5], [1, 2], {1: 100, 2: 60}.get, 50) == (50, 2, 2, False, None)  # no stop: max_samples


def test_the_binding_declares_the_multinomial_in_place_calls():
    """Fails without the feature."""
    from badger_amcl_amd import _lib, local_world, sharded
    for name in ("bpf_shard_set_multinomial_form", "bpf_shard_get_multinomial_form", "bpf_shard_inplace_mn_select_dev",
                 "bpf_shard_inplace_mn_bins_dev", "bpf_shard_inplace_mn_stop_dev"):
        assert name in _lib.SIGNATURES
    for name in ("inplace_mn_select", "inplace_mn_bins", "inplace_mn_stop", "set_multinomial_form"):
        assert hasattr(sharded.HipShardBackend, name)
    import inspect
    assert "multinomial_form" in inspect.signature(sharded.ShardedFilter.__init__).parameters
    assert "multinomial_form" in inspect.signature(local_world.LocalShardedFilter.__init__).parameters


def test_one_case_stops_early_and_one_does_not(orc):
    """The two regimes, in one test: a blob stops well below max_samples, a spread cloud draws all of them."""
    seen = []
    for kind, n, min_samples, seed in [("blob", 3000, 100, 11), ("spread", 600, 20, 15)]:
        s = cloud(kind, n, seed)
        opf = orc.ParticleFilter(min_samples, n, 0.0, 0.0, 85.0, seed=seed)
        opf.set_samples(s)
        opf.pf.w_slow = opf.pf.w_fast = 1.0
        rng0 = int(opf.pf.rng)
        out = opf.update_resample()
        M = out.sample_count
        R = check(orc, s, cuts_for(n, 3, "tiny"), n, min_samples, seed, kbr.LEAVES, opf.samples[:M, :3], M,
                  out.leaf_count, out.node_count, int(opf.pf.rng), rng0)
        seen.append((R["stopped"], M))
    assert seen[0][0] and seen[0][1] < 3000
    assert not seen[1][0] and seen[1][1] == 600
