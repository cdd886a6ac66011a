"""The sharded filter (all ranks in this process, W = 2 and 3) in map frames far from the origin
(tests/far_frames.py), against ONE engine that holds the whole set.

Statistics.  bpf_shard_compute_cluster_stats / get_cluster / get_max_weight_pose on 6 000 samples (the distributed
form): the same bits on every rank as the single engine's evaluation, at every frame.  Where the sums do not fit the
32.96 fixed-point format the single engine falls to its host evaluation and the sharded filter must take its host
route (f.stats_route), with the same bits again.  Two ways of leaving the format that only a sharded set has: ONE
rank's own sums pass 2^31 (it marks what it exports, kernels_shard_stats.hpp), and every rank's share of a cluster fits
while their total does not (k_sstat_import finds it in the reduced words).

Convergence.  The in-place systematic and multinomial resample sum the UNWEIGHTED x and y of each rank's new slice
(k_inplace_xy_sums): 3 000 samples a million metres out are 3e9 > 2^31.  Converged flag and percentage, poses, leaf
and bin counts and the rng states equal the single engine's updateResample, which is exact against the oracle
(test_gpu_resample_regimes._oracle_check)."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_local_world.py

import far_frames as ff
from badger_amcl_amd import synth

pytestmark = pytest.mark.gpu

SEED, BEAMS, N = 21, 61, 6000
POP = (0.0002, 3.0)  # a bound no set of 6 000 reaches: the resampled set keeps all 6 000 samples


@pytest.fixture(scope="module")
def pool():
    import badger_amcl_amd as bpf
    engines = [bpf.Engine(0) for _ in range(4)]  # [0 .. 2]: the ranks, [3]: the single engine
    yield engines
    for e in engines:
        e.close()


def _cuts(n, W):
    return [(n * r) // W for r in range(W + 1)]


def _world_and_single(pool, whole, W, cuts=None):
    """(every rank's statistics, the route, the single engine's statistics in its default mode)."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    from test_gpu_local_world import _world_stats
    from test_gpu_shard_stats import reference_stats
    n = whole.shape[0]
    cuts = cuts or _cuts(n, W)
    pfs = [bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0) for e in pool[:W]]
    f = LocalShardedFilter(pfs)
    try:
        f.load([whole[cuts[r]:cuts[r + 1]] for r in range(W)], tree=False)
        got = _world_stats(f)
        route = f.stats_route
    finally:
        f.shutdown()
        f.close()
    return got, route, reference_stats(pool[3], whole), reference_stats(pool[3], whole, host=True)


def _check(got, route, single, single_host, fits, what):
    from test_gpu_shard_stats import assert_same_bits
    print("far shards %s: fits %d route %s" % (what, fits, route))
    assert route == ("distributed" if fits else "host"), what
    for r, g in enumerate(got):
        assert_same_bits(g, single, (what, r))
    if not fits:  # ... and the single engine fell to its host evaluation too
        assert_same_bits(single, single_host, (what, "single engine's route"))


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("frame", ff.OFFSETS)
@pytest.mark.parametrize("name", ["shards6000", "blob6000"])
def test_statistics_equal_the_single_engine_in_every_frame(pool, orc, name, frame, W):
    """shards6000: three blobs and stragglers, where `over_xx` leaves the format in the set's sums only.  blob6000: one
    cluster that every rank holds a share of, where at `over_xx` every rank's share fits and the total does not."""
    s, want, exact = ff.reference(orc, name, frame, "normalised")
    fits = ff.fits_fixed_point(s, exact)
    assert fits == (frame in ("control", "few_km", "under"))
    got, route, single, single_host = _world_and_single(pool, s, W)
    _check(got, route, single, single_host, fits, (name, frame, W))
    if frame == "over_xx" and name == "blob6000":
        cuts = _cuts(N, W)
        t = ff.terms(s)
        shares = [float(ff.exact_sum(t[5, cuts[r]:cuts[r + 1]])) for r in range(W)]
        assert max(shares) < 2.0 ** 31 < sum(shares)


@pytest.mark.parametrize("frame", ["control", "few_km"])
def test_statistics_with_weights_of_one(pool, orc, frame):
    """Unnormalised weights (bpf_pf_set_samples admits them): 6 000 samples of weight 1 leave the format 600 m out."""
    s, want, exact = ff.reference(orc, "shards6000", frame, "ones")
    fits = ff.fits_fixed_point(s, exact)
    assert fits == (frame == "control")
    got, route, single, single_host = _world_and_single(pool, s, 2)
    _check(got, route, single, single_host, fits, ("ones", frame))


@pytest.mark.parametrize("W", [2, 3])
def test_one_rank_alone_leaves_the_format(pool, orc, W):
    """Rank 0's slice of the one-cluster set sits where ITS OWN sum of w x^2 passes 2^31 (its weights are 1 / W of the
    total, so that is further out than `over_xx` of the whole set); the other ranks stay at the control."""
    base = ff.base_cloud("blob6000")
    w = ff.weights(N, "normalised")
    cut = _cuts(N, W)[1]
    dx, dy = ff.offset("over_xx", base[:cut], w[:cut])
    s = base.copy()
    s[:, 3] = w
    s[:cut, 0] += dx
    s[:cut, 1] += dy
    t = ff.terms(s)
    mine, rest = ff.exact_sum(t[5, :cut]), ff.exact_sum(t[5, cut:])
    assert mine > ff.TWO31 and rest < 1000 and np.all(np.abs(t) < ff.TERM_GUARD)
    got, route, single, single_host = _world_and_single(pool, np.ascontiguousarray(s), W)
    _check(got, route, single, single_host, False, ("one rank", W))


# ------------------------------------------------------------------------------------------------ convergence
def _far_scenario(orc, frame):
    from map_geometry import GeoScenario
    dx, dy = ff.FIXED_OFFSETS[frame]
    sc = GeoScenario(orc, 151, 62, 0.05, (dx + 3.75, dy + 1.5), beams=BEAMS, n=N, cloud="converged")
    assert float(sc.origin[0]) == dx + 3.75 and float(sc.origin[1]) == dy + 1.5  # exact in float32
    w = sc.samples[:, 3].copy()
    sc.samples = synth.converged_cloud(N, sc.pose, seed=41, sigma=(0.1, 0.1, 0.05))
    sc.samples[:, 3] = w
    return sc


_REF = {}


def single_resample(orc, key, make_scenario, resampler):
    """One engine: sensor update, updateResample against the oracle; the scored set, the rng before, the record.
    Computed once per key and shared."""
    from test_gpu_resample_regimes import _oracle_check, _options
    from test_gpu_local_world import _single
    if key not in _REF:
        sc = make_scenario()
        n = sc.samples.shape[0]
        e, scn, pf, data, od = _single(sc, resampler=resampler, seed=SEED, beams=BEAMS)
        try:
            _options([e])
            pf.setPopulationSizeParameters(*POP)
            scn.updateSensor(pf, data)
            scored, rng0 = pf.getCurrentSet().samples.copy(), pf.getRngState()
            one = _oracle_check(orc, pf, n, resampler=resampler, pop=POP)
            st = pf.getState()
            one.update(conv=st.converged, pct=st.percent_converged, scored=scored, rng0=rng0)
            _REF[key] = (sc, one)
        finally:
            e.close()
    return _REF[key]


def in_place_against_single(engines, sc, one, resampler, W, what, orc=None, keys_pack=True):
    """The sharded in-place resample of `sc` on W ranks against the single engine's record `one`: poses (in the
    in-place order: rotated teeth / sorted by owner), weights, counts of the tree, rng, converged flag and percentage.
    keys_pack = False: some histogram key of the set lies outside kld_pack's range, where the in-place multinomial
    form hands the resample to the window form before it changes anything (shard_update_resample_in_place_mn): the
    single engine's set in its own order, in even slices, and every other figure as exact."""
    import badger_amcl_amd as bpf
    import shard_in_place_ref as ipr
    from badger_amcl_amd.local_world import LocalShardedFilter
    from badger_amcl_amd.sharded import even_counts
    from test_gpu_local_world import ODOM, _shard_of
    from test_gpu_resample_regimes import _options
    from test_gpu_shard_in_place_mn import permuted
    n, M = sc.samples.shape[0], one["M"]
    cuts = _cuts(n, W)
    keep, pfs = [], []
    for r, e in enumerate(engines[:W]):
        m, scn, pf, data = _shard_of(sc, cuts[r], cuts[r + 1]).gpu_objects(e, BEAMS, "lf", min_samples=100,
                                                                          max_samples=n, seed=SEED)
        pf.setResampleModel(resampler)
        pf.setPopulationSizeParameters(*POP)
        bpf.Odom(e).setModel(*ODOM)
        keep.append((m, scn, data))
        pfs.append(pf)
    _options(engines[:W])
    f = LocalShardedFilter(pfs, max_share=float(W), resample_form="in_place" if resampler == 1 else "window",
                           multinomial_form="in_place" if resampler == 0 else "window")
    try:
        f.load([sc.samples[cuts[r]:cuts[r + 1]] for r in range(W)], tree=resampler == 1)
        f.update_sensor(keep[0][2])
        f.update_resample()
        assert not f.cdf_miss
        if keys_pack:
            assert f.form_used == "in_place" and f.windows_used == 0
        else:
            assert resampler == 0 and f.form_used == "window" and f.windows_used >= 1
        S = one["samples"]
        leaf, bins = one["leaf"], one["bins"]
        if not keys_pack:
            want = S
            assert f.counts == even_counts(M, W)
        elif resampler == 1:
            _, i_wrap, _ = ipr.target_chain(one["rng0"], M)
            want = ipr.rotate(S, 0, i_wrap)
            # the reference's leaf counter depends on the order of insertion: the rotated set's own tree, as
            # tests/test_gpu_shard_in_place_bindings.py takes it (there from an engine, here from the oracle's tree)
            t = ff.oracle_tree(orc, want)
            leaf, bins = t.leaf_count(), t.node_count()
            assert bins == one["bins"]
        else:
            want, counts = permuted(S, one["scored"], cuts)
            assert f.counts == counts
        got = np.concatenate([p for p in f.local_sets() if p.shape[0] > 0])
        assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
        assert np.all(got[:, 3] == 1.0 / M)
        assert (f.sample_count, f.leaf_count, f.bin_count) == (M, leaf, bins)
        assert f.rng_states() == [one["rng"]] * W
        states = f.rank_states()
        print("far in-place %s resampler %d W %d: converged %s percent %s (single %d, %.1f)" %
              (what, resampler, W, [s.converged for s in states], [s.percent_converged for s in states],
               one["conv"], one["pct"]))
        assert [s.converged for s in states] == [one["conv"]] * W
        assert [s.percent_converged for s in states] == [one["pct"]] * W
    finally:
        f.shutdown()
        f.close()


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("resampler", [1, 0], ids=["systematic", "multinomial"])
@pytest.mark.parametrize("frame", ["far", "few_km"])
def test_in_place_resample_and_convergence_in_a_far_frame(pool, orc, frame, resampler, W):
    sc, one = single_resample(orc, (frame, resampler), lambda: _far_scenario(orc, frame), resampler)
    assert one["M"] == N and one["conv"] == 1 and one["pct"] == 100.0  # converged, and every rank keeps its thousands
    cuts = _cuts(N, W)
    if frame == "far":
        # what the 32.96 format cannot hold: the unweighted sum of a rank's y (and of x at W = 2)
        assert min(abs(float(np.sum(one["samples"][cuts[r]:cuts[r + 1], 1]))) for r in range(W)) > 2.0 ** 31
    in_place_against_single(pool, sc, one, resampler, W, frame, orc)
