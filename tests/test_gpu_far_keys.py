"""Every resample regime at the edge of the histogram key's packing (kld_pack: x key in [-2^23, 2^23 - 2], y key in
[-2^23, 2^23 - 1]; tests/far_frames.py builds the clouds).  Elsewhere in the suite the keys stay below ~10^3 in
magnitude, or about 10^7 where every device path declines: the hash (pk * golden) >> k, the unpacking with >> 40 and
& 0xFFFFFF, the "kld_pack, undone" decodes of the sharded kernels and the neighbour lookups that skip an unpackable
neighbour have not seen a key with its high bits set, a negative key near -2^23, or a cloud of which PART declines.

Single engine: the regimes as tests/test_gpu_resample_regimes.py and tests/test_gpu_kld_bins.py force them -- the
one-block kernel with its register tree and with its LDS tree (BPF_OPT_FUSED_LDS_TREE), the whole-stream device tree
(BPF_OPT_KLD_DEVICE_MIN = 1), the host's windows, for both resamplers and both KLD count modes (leaves; the opt-in
occupied-bin bound).  On `mid` and the inside clouds the regime asked for is the one that ran (kld_on_device), and
the result is exact against the oracle (leaves) or the restatement of kld_bins_ref.py (bins): count, bit-equal poses,
leaf and bin counts, rng state, converged; on the straddle clouds the same exactness whichever route takes the set,
and last_status 0.

Sharded: the initialiser's tree and the in-place multinomial resample (both decode packed keys) against the single
engine.  Statistics: labels and counts at the edge are exact, so the neighbours kld_pack refuses change nothing."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_local_world.py

import far_frames as ff

pytestmark = pytest.mark.gpu

N = 3000
POP_LOOSE = (0.05, 0.99)  # the stop rule ends the stream inside the window: the count AT the stop is checked
FORM_HOST, FORM_DEVICE, FORM_BLOCK = 0, 1, 2  # bpf_pf_state.kld_on_device

# name: (resampler, BPF_OPT_FUSED_RESAMPLE, BPF_OPT_FUSED_LDS_TREE, BPF_OPT_KLD_DEVICE_MIN, kld_on_device expected)
REGIMES = {
    "block": (0, 1, 0, 8192, FORM_BLOCK),
    "block_lds_tree": (0, 1, 1, 8192, FORM_BLOCK),
    "device_tree": (0, 1, 0, 1, FORM_DEVICE),
    "host_windows": (0, 0, 0, 8192, FORM_HOST),
    "systematic_block": (1, 1, 0, 8192, FORM_BLOCK),
    "systematic_block_lds_tree": (1, 1, 1, 8192, FORM_BLOCK),
    "systematic_general": (1, 0, 0, 1, None),  # (its counting path is the driver's choice; the result is what counts)
}


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


_SETS = {}


def _edge_set(orc, name):
    if name not in _SETS:
        s = ff.edge_cloud(name, N, ff.bin_size(orc))
        s[:, 3] = np.random.default_rng(4).uniform(0.5, 1.5, N)
        s[:, 3] /= s[:, 3].sum()
        _SETS[name] = s
    return _SETS[name].copy()


def _leaves_against_oracle(orc, engine, s, resampler):
    """tests/test_gpu_resample_regimes.py::_oracle_check, and the converged flag with it."""
    import badger_amcl_amd as bpf
    pf = bpf.ParticleFilter(engine, 100, N, 0.0, 0.0, 85.0)
    pf.setResampleModel(resampler)
    pf.setPopulationSizeParameters(*POP_LOOSE)
    pf.srand48(11)
    pf.setKldCount(0)
    pf.initWithSamples(s)
    st0, rng0 = pf.getState(), pf.getRngState()
    pf.updateResample()
    st1, after = pf.getState(), pf.getCurrentSet().samples
    opf = orc.ParticleFilter(100, N, 0.0, 0.0, 85.0)
    opf.pf.rng = rng0
    opf.set_resample_model(resampler)
    opf.set_samples(s, leaf_count=st0.leaf_count)
    opf.set_population_size_parameters(*POP_LOOSE)
    # a set that was loaded, not scored: w_slow = w_fast = 0, and the reference's w_diff = 1 - 0 / 0 is a NaN whose
    # conversion to a count of random poses C leaves undefined.  The engine resamples such a set without recovery
    # draws; the oracle is given averages that say the same (w_diff = 0).
    assert (st0.w_slow, st0.w_fast) == (0.0, 0.0)
    opf.pf.w_slow = opf.pf.w_fast = 1.0
    out = opf.update_resample()
    M = out.sample_count
    assert out.status == 0 and out.w_diff == 0.0
    assert (st1.sample_count, st1.leaf_count, st1.bin_count) == (M, out.leaf_count, out.node_count)
    assert np.array_equal(after[:, :3], opf.samples[:M, :3])
    assert np.all(after[:, 3] == 1.0 / M)
    assert pf.getRngState() == opf.pf.rng
    assert st1.converged == out.converged
    assert abs(st1.percent_converged - out.percent_converged) <= 1e-4
    return st1


@pytest.mark.parametrize("mode", [0, 1], ids=["leaves", "bins"])
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("cloud", ff.EDGE_CLOUDS)
def test_resample_regimes_at_the_packing_edge(engine, orc, cloud, regime, mode):
    import badger_amcl_amd.pf as hpf
    from test_gpu_kld_bins import _run
    resampler, fused, lds_tree, device_min, expected = REGIMES[regime]
    s = _edge_set(orc, cloud)
    engine.set_option(hpf.OPT_FUSED_LDS_TREE, lds_tree)
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    engine.set_option(hpf.OPT_FUSED_RESAMPLE, fused)
    engine.set_option(hpf.OPT_KLD_DEVICE_MIN, device_min)
    try:
        if mode == 0:
            st = _leaves_against_oracle(orc, engine, s, resampler)
        else:
            st, _ = _run(engine, orc, s, resampler, 100, N, fused=fused, kld_min=device_min, pop=POP_LOOSE)
        print("far keys %s %s mode %d: M %d leaf %d bins %d kld_on_device %d windows %d" %
              (cloud, regime, mode, st.sample_count, st.leaf_count, st.bin_count, st.kld_on_device,
               st.resample_windows))
        assert st.last_status == 0
        assert 100 < st.sample_count <= N
        if mode == 0:
            assert st.sample_count < N  # the stop lies inside the stream (753 .. 1998 by the oracle alone)
        if not cloud.startswith("straddle") and expected is not None:
            assert st.kld_on_device == expected
    finally:
        engine.set_option(hpf.OPT_FUSED_LDS_TREE, 0)
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
        engine.set_option(hpf.OPT_FUSED_RESAMPLE, 1)
        engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 8192)


@pytest.mark.parametrize("n", [N, 5000], ids=["one_block", "multi_launch"])
@pytest.mark.parametrize("cloud", [c for c in ff.EDGE_CLOUDS if not c.startswith("straddle")])
def test_cluster_statistics_at_the_packing_edge(engine, orc, cloud, n):
    """Device mode on clouds whose outermost bins have neighbours kld_pack refuses: cluster count, counts (the labels)
    and the heaviest cluster are the oracle's.  2 097 km out (mid) and 4 194 km out (the edges) the sum of w x^2 is a
    thousand times beyond the fixed-point format, so the figures themselves are the host evaluation's: the oracle's
    bits."""
    import badger_amcl_amd as bpf
    from test_gpu_next_rows import _assert_stats_equal
    s = ff.edge_cloud(cloud, n, ff.bin_size(orc), seed=8)
    s[:, 3] = np.random.default_rng(5).uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    assert max(float(np.sum(ff.terms(s)[k])) for k in (5, 8)) > 1000.0 * ff.TWO31
    want = ff.oracle_stats(orc, s)
    assert want["n"] >= 1 and int(want["count"].sum()) == n
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
    pf.initWithSamples(s)
    _assert_stats_equal(pf, want, exact=True)


# ------------------------------------------------------------------------------------------------ sharded
@pytest.fixture(scope="module")
def pool():
    import badger_amcl_amd as bpf
    engines = [bpf.Engine(0) for _ in range(4)]  # [0 .. 2]: the ranks, [3]: the single engine
    yield engines
    for e in engines:
        e.close()


def _edge_of(cloud, b):
    sign, axis = cloud[-2], cloud[-1]
    return "xy".index(axis), ((ff.KEY_MAX[axis] + 1) * b if sign == "+" else ff.KEY_MIN[axis] * b), sign == "+"


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("cloud", ["inside-x", "inside+y", "straddle+x"])
def test_shard_initialiser_at_the_packing_edge(pool, orc, cloud, W):
    """bpf_shard_init_with_gaussian_all: the slices concatenate to one engine's initWithGaussian, and the tree counts
    (from the ranks' packed bin keys where they pack) and the rng agree."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    b = ff.bin_size(orc)
    a, edge, up = _edge_of(cloud, b)
    sigma = (0.6, 0.6, 0.1)
    mean = np.array([0.0, 0.0, 0.4])
    if cloud.startswith("inside"):
        mean[a] = edge - 6 * sigma[a] if up else edge + 6 * sigma[a]
    else:
        mean[a] = edge
    pf1 = bpf.ParticleFilter(pool[3], 100, N, 0.0, 0.0, 85.0)
    pf1.srand48(7)
    pf1.initWithGaussian(mean, np.eye(3), sigma)
    st, whole = pf1.getState(), pf1.getCurrentSet().samples
    share = 1.0 - ff.packs(whole, b).mean()
    assert (share == 0.0) if cloud.startswith("inside") else (0.1 <= share <= 0.9)
    pfs = [bpf.ParticleFilter(e, 100, N, 0.0, 0.0, 85.0) for e in pool[:W]]
    for pf in pfs:
        pf.srand48(7)
    f = LocalShardedFilter(pfs)
    try:
        f.init_with_gaussian(mean, np.eye(3), sigma)
        print("far keys init %s W %d: tree route %s leaf %d bins %d" % (cloud, W, f.tree_route, f.leaf_count,
                                                                         f.bin_count))
        assert np.array_equal(np.concatenate(f.local_sets()), whole)
        assert (f.leaf_count, f.bin_count) == (st.leaf_count, st.bin_count)
        assert f.rng_states() == [pf1.getRngState()] * W
    finally:
        f.shutdown()
        f.close()


def _edge_scenario(orc, cloud):
    """A map whose origin lies in the cloud (exact in float32: a multiple of 0.5 m at this magnitude) and the edge cloud
    as its particle set, with the scenario's non-uniform prior weights."""
    from map_geometry import GeoScenario
    b = ff.bin_size(orc)
    a, edge, up = _edge_of(cloud, b)
    origin = [0.0, 1.5]
    origin[a] = edge - 2.0 if up else edge + 2.0
    sc = GeoScenario(orc, 151, 62, 0.05, tuple(origin), beams=61, n=N, cloud="converged")
    assert float(sc.origin[a]) == origin[a]
    w = sc.samples[:, 3].copy()
    sc.samples = ff.edge_cloud(cloud, N, b, seed=6)
    sc.samples[:, 3] = w
    return sc


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("cloud", ["inside-x", "inside+y", "straddle+x"])
def test_sharded_in_place_multinomial_at_the_packing_edge(pool, orc, cloud, W):
    from test_gpu_far_shards import in_place_against_single, single_resample
    sc, one = single_resample(orc, ("edge", cloud), lambda: _edge_scenario(orc, cloud), 0)
    packs = bool(np.all(ff.packs(sc.samples, ff.bin_size(orc))))
    assert packs == cloud.startswith("inside")
    in_place_against_single(pool, sc, one, 0, W, cloud, orc, keys_pack=packs)
