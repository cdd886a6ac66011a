"""A sharded filter with all its ranks in ONE process (bpf_shard_connect_local, badger_amcl_amd/local_world.py): W
engines on device 0, one host thread each, every step one collective C call per rank, the exchanges the pulls of
kernels_local_exchange.hpp ordered by events and a host barrier.  Compared, as the other sharded tests compare, with
ONE engine that holds the whole set.

The cap "the resampled set differs in at most ONE pose per cycle" (tests/test_gpu_cpp_shard_node.py::_check_cycles) is a
condition on the seed: more ranks mean more slice edges a draw can round across.  The scenario, seed, even splits and
world sizes of the cycle tests below were first run through the CPU backend of tests/test_sharded_cpu.py
(OracleShardBackend over gloo, both resamplers, W = 2, 3, 8, three cycles): seeds 21 and 5 gave 0 differing poses in
every cycle there; seed 21 is kept.  That backend counts leaves only; the bins count mode draws the same stream from
the same CDFs and differs in where the stream stops."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py

from scenario import Scenario

pytestmark = pytest.mark.gpu

ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion
SEED = 21
N, BEAMS = 3000, 60
BPF_ERR_INVALID_ARGUMENT, BPF_ERR_EXCHANGE = 1, 9


def _even_cuts(n, W):
    return [(n * r) // W for r in range(W + 1)]


def _shard_of(sc, lo, hi):
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    return shard


class World:
    """W engines on device 0 set up from one scenario (every rank: map, scanner, model, filter with the GLOBAL
    bounds, its slice), connected as one local world."""

    def __init__(self, sc, W, model="lf", resampler=0, kld=None, alpha=(0.0, 0.0), model_kw=None, seed=SEED,
                 timeout_ms=None, beams=BEAMS):
        import badger_amcl_amd as bpf
        from badger_amcl_amd.local_world import LocalShardedFilter
        n = sc.samples.shape[0]
        self.cuts = _even_cuts(n, W)
        self.engines = [bpf.Engine(0) for _ in range(W)]
        self.keep, pfs = [], []
        for r, e in enumerate(self.engines):
            m, scn, pf, data = _shard_of(sc, self.cuts[r], self.cuts[r + 1]).gpu_objects(
                e, beams, model, min_samples=100, max_samples=n, seed=seed, alpha=alpha, model_kw=model_kw)
            pf.setResampleModel(resampler)
            bpf.Odom(e).setModel(*ODOM)
            self.keep.append((m, scn, data))
            pfs.append(pf)
        self.data = self.keep[0][2]
        self.f = LocalShardedFilter(pfs, kld_count=kld, timeout_ms=timeout_ms)
        self.f.load([sc.samples[self.cuts[r]:self.cuts[r + 1]] for r in range(W)])

    def close(self):
        self.f.close()
        for e in self.engines:
            e.close()


def _single(sc, model="lf", resampler=0, kld=None, alpha=(0.0, 0.0), model_kw=None, seed=SEED, beams=BEAMS):
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    m, scn, pf, data = sc.gpu_objects(e, beams, model, min_samples=100, max_samples=sc.samples.shape[0], seed=seed,
                                      alpha=alpha, model_kw=model_kw)
    pf.setResampleModel(resampler)
    if kld is not None:
        pf.setKldCount(kld)
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    return e, scn, pf, data, od


def _single_cycles(pf, cycles, step):
    """step(cycle) moves and scores the single engine; the records _check_cycles compares against."""
    out = []
    for c in range(cycles):
        conv_before = pf.getState().converged
        step(c)
        w = pf.getCurrentSet().samples.copy()
        pf.updateResample()
        st = pf.getState()
        out.append(dict(w=w, samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                        bins=st.bin_count, rng=pf.getRngState(), conv=st.converged, conv_before=conv_before,
                        w_diff=st.w_diff, w_slow=st.w_slow))
    return out


def _world_cycles(f, cycles, step):
    out, last = [], f.exchange_counts()
    for c in range(cycles):
        step(c)
        w = np.concatenate(f.local_sets())
        f.update_resample()
        sets = f.local_sets()
        exch = f.exchange_counts()
        assert all(a > b for a, b in zip(exch, last))  # every step exchanges, on every rank
        last = exch
        out.append(dict(w=w, sets=sets, M=f.sample_count, leaf=f.leaf_count, bins=f.bin_count, rng=f.rng_states(),
                        conv=[s.converged for s in f.rank_states()], miss=f.cdf_miss,
                        w_slow=[s.w_slow for s in f.rank_states()]))
    return out


def _check_cycles(got, ref, W, weights=True):
    """tests/test_gpu_cpp_shard_node.py::_check_cycles over the records above."""
    assert len(got) == len(ref)
    for g, one in zip(got, ref):
        if weights:
            assert g["w"].shape == one["w"].shape and np.array_equal(g["w"][:, :3], one["w"][:, :3])
            assert np.allclose(g["w"][:, 3], one["w"][:, 3], rtol=1e-12, atol=0)
        M = one["M"]
        assert (g["M"], g["leaf"], g["bins"]) == (M, one["leaf"], one["bins"])  # (the ranks agreed: update_resample)
        assert g["rng"] == [one["rng"]] * W
        assert g["conv"] == [one["conv"]] * W
        assert not g["miss"]
        assert [s.shape[0] for s in g["sets"]] == [(M * (r + 1)) // W - (M * r) // W for r in range(W)]
        new = np.concatenate(g["sets"])
        assert new.shape == one["samples"].shape == (M, 4)
        assert np.flatnonzero(np.any(new[:, :3] != one["samples"][:, :3], axis=1)).size <= 1
        assert np.all(new[:, 3] == 1.0 / M)


# ------------------------------------------------------------------------------------------------ the transport itself
@pytest.mark.parametrize("W", [2, 3, 8, 16])
def test_selftest_every_exchange_every_cell(W):
    """bpf_shard_local_selftest: ragged int64 gathers (one rank contributes nothing, spans and sources off the 16-byte
    grid), f64 all-gathers, int64 and int32 sums in place at every offset within 16 bytes, at 0, 1, 255, 256, 257 and
    6 * 4096 + 3 words; every cell and the guard words around the destinations are compared inside the call."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import EXCHANGE_LOCAL, LocalShardedFilter
    engines = [bpf.Engine(0) for _ in range(W)]
    try:
        pfs = [bpf.ParticleFilter(e, 100, N, 0.0, 0.0, 85.0) for e in engines]
        f = LocalShardedFilter(pfs, connect=False)
        assert f.exchange_mode() == [0] * W
        f.connect()
        assert f.exchange_mode() == [EXCHANGE_LOCAL] * W
        f.selftest(2)  # two rounds: the empty rank moves on
        f.shutdown()
        assert f.exchange_mode() == [0] * W
        f.close()
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ cycles
_REF = {}


def _cycle_scenario(orc):
    if "sc" not in _REF:
        _REF["sc"] = Scenario(orc, size=200, n=N, beams=BEAMS, cloud="converged")
    return _REF["sc"]


def _cycle_reference(orc, resampler, kld):
    """One engine, three cycles of motion, sensor, resample: computed once per (resampler, count mode)."""
    import badger_amcl_amd as bpf
    key = ("cycles", resampler, kld)
    if key not in _REF:
        sc = _cycle_scenario(orc)
        e, scn, pf, data, od = _single(sc, resampler=resampler, kld=kld)
        try:
            def step(c):
                od.updateAction(pf, bpf.OdomData(*ODATA))
                scn.updateSensor(pf, data)
            _REF[key] = _single_cycles(pf, 3, step)
        finally:
            e.close()
    return _REF[key]


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("kld", [0, 1])
@pytest.mark.parametrize("resampler", [0, 1])
def test_three_cycles_equal_the_single_engine(orc, resampler, kld, W):
    """Slices loaded on the ranks, then motion, sensor, resample three times; both resamplers, both KLD count modes."""
    import badger_amcl_amd as bpf
    ref = _cycle_reference(orc, resampler, kld)
    w = World(_cycle_scenario(orc), W, resampler=resampler, kld=kld)
    try:
        def step(c):
            w.f.update_action(None, bpf.OdomData(*ODATA))
            w.f.update_sensor(w.data)
        _check_cycles(_world_cycles(w.f, 3, step), ref, W)
    finally:
        w.close()


INIT_SIGMA = (0.2, 0.2, 0.05)


def _init_reference(orc, resampler):
    """One engine: initWithGaussian, then three cycles; computed once per resampler."""
    import badger_amcl_amd as bpf
    key = ("init", resampler)
    if key not in _REF:
        sc = _cycle_scenario(orc)
        e, scn, pf, data, od = _single(sc, resampler=resampler)
        try:
            pf.initWithGaussian(sc.pose, np.eye(3), INIT_SIGMA)
            st0 = pf.getState()
            start = dict(samples=pf.getCurrentSet().samples.copy(), leaf=st0.leaf_count, bins=st0.bin_count,
                         rng=pf.getRngState())

            def step(c):
                od.updateAction(pf, bpf.OdomData(*ODATA))
                scn.updateSensor(pf, data)
            _REF[key] = (start, _single_cycles(pf, 3, step))
        finally:
            e.close()
    return _REF[key]


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("resampler", [0, 1])
def test_init_on_the_ranks_then_three_cycles(orc, resampler, W):
    """bpf_shard_init_with_gaussian_all over the local world: the slices concatenate to what one engine's
    initWithGaussian draws, the tree counts and the rng agree, and three cycles of motion, sensor, resample from there
    equal the single engine's.  (The same start -- the oracle's initWithGaussian of seed 21 -- went through the CPU
    backend at W = 2, 3, 8 with both resamplers before the cap of one pose per cycle was asserted here.)"""
    import badger_amcl_amd as bpf
    sc = _cycle_scenario(orc)
    start, ref = _init_reference(orc, resampler)
    w = World(sc, W, resampler=resampler)
    try:
        w.f.init_with_gaussian(sc.pose, np.eye(3), INIT_SIGMA)
        assert np.array_equal(np.concatenate(w.f.local_sets()), start["samples"])
        assert (w.f.leaf_count, w.f.bin_count) == (start["leaf"], start["bins"])
        assert w.f.rng_states() == [start["rng"]] * W

        def step(c):
            w.f.update_action(None, bpf.OdomData(*ODATA))
            w.f.update_sensor(w.data)
        _check_cycles(_world_cycles(w.f, 3, step), ref, W)
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ W = 8: the other updates
def test_prob_model_with_beam_skipping_at_eight_ranks(orc):
    """The prob model's beam skipping (tests/test_gpu_cpp_shard_node.py): the first resample reports "converged", so
    the updates of cycles 1 and 2 sum the per-beam int32 counts over the local world between their two passes."""
    from badger_amcl_amd import synth
    sc = Scenario(orc, size=200, n=N, beams=BEAMS, cloud="converged", frac_max=0.0, frac_nan=0.0)
    sc.samples = synth.converged_cloud(N, sc.pose, seed=12, sigma=(0.05, 0.05, 0.02))
    kw = dict(do_beamskip=1, beam_skip_distance=0.5, beam_skip_threshold=0.3, beam_skip_error_threshold=0.9)
    e, scn, pf, data, od = _single(sc, model="prob", model_kw=kw, seed=3)
    w = World(sc, 8, model="prob", model_kw=kw, seed=3)
    try:
        ref = _single_cycles(pf, 3, lambda c: scn.updateSensor(pf, data))
        assert [r["conv_before"] for r in ref[1:]] == [1, 1]  # beam skipping was armed: not the plain prob model
        _check_cycles(_world_cycles(w.f, 3, lambda c: w.f.update_sensor(w.data)), ref, 8)
    finally:
        w.close()
        e.close()


def test_cloud3d_update_at_eight_ranks(orc):
    """bpf_shard_update_sensor_cloud over the local world, and the resample accepts the totals it left."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    from test_gpu_cloud import _setup
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, N, 8, 16, seed=6)  # 128 points
    W = 8
    cuts = _even_cuts(N, W)
    engines = [bpf.Engine(0) for _ in range(W + 1)]
    try:
        keep, pfs = [], []
        for e in engines:
            om = bpf.OctoMap(e, 0.05)
            om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
            scn = bpf.PointCloudScanner(e)
            scn.init(128, om)
            scn.setPointCloudModel(0.5, 0.05, 0.1)
            scn.setMapFactors(0.95, 0.95, 0.3)
            scn.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
            pf = bpf.ParticleFilter(e, 100, N, 0.0, 0.0, 85.0)
            pf.srand48(5)
            keep.append((om, scn))
            pfs.append(pf)
        pf1, scn1 = pfs[W], keep[W][1]
        pf1.initWithSamples(s)
        data = bpf.PointCloudData(pts)
        f = LocalShardedFilter(pfs[:W])
        f.load([s[cuts[r]:cuts[r + 1]] for r in range(W)])
        ref = _single_cycles(pf1, 2, lambda c: scn1.updateSensor(pf1, data))
        _check_cycles(_world_cycles(f, 2, lambda c: f.update_sensor(data)), ref, W)
        f.close()
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("resampler", [0, 1])
def test_recovery_draws_at_eight_ranks(orc, resampler):
    """w_diff > 0 (the node's default decay rates and a worsening scan): every rank resolves the same draw chain, shard
    0 writes the random free-space poses; sets, counts, rng and w_slow as the single engine's
    (tests/test_gpu_sharded.py::test_two_ranks_recovery_random_poses)."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    sc = Scenario(orc, size=200, n=N, beams=BEAMS, cloud="mixture")
    alpha = (0.001, 0.1)
    scans = [sc.ranges, np.clip(sc.ranges * 0.6, 0.05, 29.0), np.full(sc.ranges.shape[0], 1.0)]
    e, scn, pf, data, od = _single(sc, resampler=resampler, alpha=alpha)
    w = World(sc, 8, resampler=resampler, alpha=alpha)
    try:
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        w.f.set_random_pose_generator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        ref = _single_cycles(pf, 3, lambda c: scn.updateSensor(pf, bpf.PlanarData(scans[c], sc.angles, sc.range_max)))
        assert max(r["w_diff"] for r in ref) > 0.01  # the recovery branch really ran
        got = _world_cycles(w.f, 3, lambda c: w.f.update_sensor(bpf.PlanarData(scans[c], sc.angles, sc.range_max)))
        for g, one in zip(got, ref):
            assert (g["M"], g["leaf"]) == (one["M"], one["leaf"]) and g["rng"] == [one["rng"]] * 8
            # w_slow follows the set's total weight, which the shards sum in rank order and one engine in its own: the
            # bound of the normalised weights (rtol 1e-12, as tests/test_sharded_cpu.py has it for w_slow)
            assert np.allclose(g["w_slow"], one["w_slow"], rtol=1e-12, atol=0)
            assert np.array_equal(np.concatenate(g["sets"])[:, :3], one["samples"][:, :3])
    finally:
        w.close()
        e.close()


# ------------------------------------------------------------------------------------------------ W = 8: the global pose
def _world_stats(f):
    """What test_gpu_shard_stats.read_stats reads, from every rank's engine; the ranks must hold the same bits."""
    n, mean, cov = f.compute_cluster_stats()
    bw, bp = f.get_max_weight_pose()
    per_rank = []
    for pf in f.pfs:
        cl = [pf.getClusterStats(k) for k in range(n)]
        assert pf.getClusterStats(n) is None
        per_rank.append(dict(n=np.array([n]), set_mean=np.array(mean), set_cov=np.array(cov),
                             weight=np.array([c[0] for c in cl]), mean=np.array([c[1] for c in cl]).reshape(n, 3),
                             count=np.array([c[2] for c in cl]), cov=np.array([c[3] for c in cl]).reshape(n, 5),
                             best_w=np.array([bw]), best_pose=np.array(bp)))
    return per_rank


def _stats_set(orc, name):
    from test_gpu_shard_stats import three_blobs
    if name == "host":
        return three_blobs(orc), True
    cloud = "spread" if name == "distributed" else "converged"
    return Scenario(orc, size=200, n=N, beams=BEAMS, cloud=cloud).samples, False


@pytest.mark.parametrize("name,cuts", [("gathered", None), ("distributed", None), ("host", None),
                                       ("gathered", [0, 0, 700, 700, 1500, 1501, 2999, 3000, 3000]),
                                       ("distributed", [0, 0, 0, 1000, 1000, 1000, 2500, 3000, 3000])])
def test_global_pose_and_particle_cloud_equal_one_engine_bit_for_bit(orc, name, cuts):
    """bpf_shard_compute_cluster_stats / bpf_shard_get_max_weight_pose / bpf_shard_get_pose_array on a loaded set with
    non-uniform weights at W = 8: the gathered, the distributed and the host route, even splits and splits with empty
    shards; the same bits on every rank as ONE engine holding the concatenation; the second query makes no exchange."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    from test_gpu_shard_stats import assert_same_bits, reference_stats
    W = 8
    whole, host = _stats_set(orc, name)
    n = whole.shape[0]
    cuts = cuts or _even_cuts(n, W)
    engines = [bpf.Engine(0) for _ in range(W + 1)]
    try:
        pfs = [bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0) for e in engines[:W]]
        for e in engines[:W]:
            e.set_option(hpf.OPT_STATS_HOST, 1 if host else 0)
        f = LocalShardedFilter(pfs)
        f.load([whole[cuts[r]:cuts[r + 1]] for r in range(W)], tree=False)
        want = reference_stats(engines[W], whole, host=host)
        before = f.exchange_counts()
        got = _world_stats(f)
        assert f.stats_route == name
        for r in range(W):
            assert_same_bits(got[r], want, (name, r))
        first = f.exchange_counts()
        assert all(a > b for a, b in zip(first, before))
        again = _world_stats(f)  # nothing changed: the same bits and no exchange
        assert f.exchange_counts() == first
        for r in range(W):
            assert_same_bits(again[r], want, (name, r, "lazy"))
        # the particle cloud: one engine's message, on one root and on every rank, whole and strided
        pf1 = bpf.ParticleFilter(engines[W], 100, n, 0.0, 0.0, 85.0)
        pf1.initWithSamples(whole)
        for root, first_i, stride in [(0, 0, 1), (5, 3, 7), (-1, 0, 1), (-1, 2999, 4), (2, 3000, 1)]:
            one = pf1.getPoseArray(first_i, stride)
            arr = f.get_pose_array(root, first_i, stride)
            assert arr.shape == one.shape and arr.tobytes() == one.tobytes(), (root, first_i, stride)
        f.close()
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ refusals, a missing rank
def _connect(lib, engines):
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    return lib.bpf_shard_connect_local(arr, len(engines), 0)


def test_refusals_leave_every_engine_as_it_was():
    """W = 16 is accepted; 17 engines, a duplicate engine, an engine without a filter, different bounds and unknown
    flags are refused, and a world connected before goes on working."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import EXCHANGE_LOCAL, LocalShardedFilter
    engines = [bpf.Engine(0) for _ in range(18)]
    try:
        lib = engines[0].lib
        pfs = [bpf.ParticleFilter(e, 100, N, 0.0, 0.0, 85.0) for e in engines[:17]]  # engines[17]: no filter
        f = LocalShardedFilter(pfs[:2])
        f.selftest(1)
        mode, count = f.exchange_mode(), f.exchange_counts()
        assert _connect(lib, engines[:17]) == BPF_ERR_INVALID_ARGUMENT
        assert _connect(lib, [engines[0], engines[1], engines[0]]) == BPF_ERR_INVALID_ARGUMENT
        assert _connect(lib, [engines[0], engines[17]]) == BPF_ERR_INVALID_ARGUMENT
        assert lib.bpf_shard_connect_local((C.c_void_p * 2)(engines[0].h, engines[1].h), 0, 0) == BPF_ERR_INVALID_ARGUMENT
        assert lib.bpf_shard_connect_local((C.c_void_p * 2)(engines[0].h, engines[1].h), 2, 1) == BPF_ERR_INVALID_ARGUMENT
        other = bpf.ParticleFilter(engines[16], 100, N + 1, 0.0, 0.0, 85.0)  # not the same global bounds
        assert _connect(lib, [engines[0], engines[16]]) == BPF_ERR_INVALID_ARGUMENT
        assert other is not None
        assert f.exchange_mode() == mode == [EXCHANGE_LOCAL] * 2 and f.exchange_counts() == count
        f.selftest(1)  # the world of two still stands
        f.close()
        f16 = LocalShardedFilter(pfs[:16])  # ranks of the old world move into the new one
        assert f16.exchange_mode() == [EXCHANGE_LOCAL] * 16
        f16.selftest(1)
        f16.close()
    finally:
        for e in engines:
            e.close()


def test_a_rank_that_does_not_arrive(orc):
    """Rank 2 of 3 stays away from a sensor update (time-out 300 ms): the ranks that came return BPF_ERR_EXCHANGE, every
    later exchange fails at once, on all three; after bpf_shard_connect_local and a reload a full cycle equals the
    single engine again.  The codes are asserted, not the time; nothing waits on the GPU while the ranks do."""
    import badger_amcl_amd as bpf
    sc = _cycle_scenario(orc)
    ref = _cycle_reference(orc, 0, 0)[:1]
    W = 3
    w = World(sc, W, kld=0, timeout_ms=300)
    try:
        f = w.f
        ranges, angles = w.data.pointers()

        def sensor(r, h, lib):
            return lib.bpf_shard_update_sensor_planar(h, ranges, angles, w.data.range_count_, w.data.range_max_, N)
        assert f.codes(sensor, ranks=[0, 1]) == [BPF_ERR_EXCHANGE] * 2
        f.set_timeout_ms(600000)  # from here on a wait that was entered would outlast the test: none is
        assert f.codes(sensor) == [BPF_ERR_EXCHANGE] * 3
        assert f.codes(lambda r, h, lib: lib.bpf_shard_local_selftest(h, 1)) == [BPF_ERR_EXCHANGE] * 3
        # a new world over the same engines; the slices and the rng as at the start
        f.set_timeout_ms(5000)
        f.connect()
        for pf in f.pfs:
            pf.srand48(SEED)
        f.load([sc.samples[w.cuts[r]:w.cuts[r + 1]] for r in range(W)])

        def step(c):
            f.update_action(None, bpf.OdomData(*ODATA))
            f.update_sensor(w.data)
        _check_cycles(_world_cycles(f, 1, step), ref, W)
    finally:
        w.close()
