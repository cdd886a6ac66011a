"""The regimes of the two resample drivers that no other file identifies by name.  Each case asserts WHICH regime ran
(bpf_pf_get_state's resample_windows / kld_on_device for the single engine; the window count of the one-call form and
the launches per kernel class for the sharded filter) and exact agreement with the reference: sample count, leaf and
bin counts, bit-equal poses, weights 1/M and the RNG state.  The single engine is checked against the oracle, the
sharded filter (all ranks in this process, tests/test_gpu_local_world.py::World, W = 2 and 3) against the single engine
on the same input.  Serial CDF everywhere, so that no draw sits on a summation-order edge.

How the sharded regimes show in the launch counts (the local world exchanges through collectives, so a window's draws
and their consumer are separate launches): every window is one launch of class "draw"; k_shard_stop_block is one of
class "finalize", and so is the tail that adopts a host-replayed set (k_shard_tail_small, every M here is <= 8192).
A set adopted by the stop block therefore shows finalize == 1, a declined stop block followed by the host's replay
finalize == 2, and windows that never try the stop block finalize == 1 (the tail alone).

The window counts are those of the code before the drivers were split by regime; where the count that reading the
schedule suggested differs from what ran, the docstring of the case says so."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_local_world.py

from scenario import Scenario
from test_gpu_local_world import SEED, World, _single

pytestmark = pytest.mark.gpu

BEAMS = 61
DEVICE_MIN_DEFAULT = 8192


def _options(engines, serial=1, device_min=DEVICE_MIN_DEFAULT):
    import badger_amcl_amd.pf as hpf
    for e in engines:
        e.set_option(hpf.OPT_CDF_SERIAL, serial)
        e.set_option(hpf.OPT_KLD_DEVICE_MIN, device_min)
        e.profile_enable(2)  # launches of every kernel class


def _oracle_check(orc, pf, max_s, resampler=0, pop=None):
    """One updateResample of the single engine against the oracle on the same set, stream state and averages; the
    record the sharded cases compare with."""
    before, st0, rng0 = pf.getCurrentSet().samples.copy(), pf.getState(), pf.getRngState()
    pf.e.profile_reset()
    pf.updateResample()
    st1, after, rng1 = pf.getState(), pf.getCurrentSet().samples.copy(), pf.getRngState()
    prof = pf.e.profile_get()
    opf = orc.ParticleFilter(100, max_s, 0.0, 0.0, 85.0)
    opf.pf.rng = rng0
    opf.set_resample_model(resampler)
    opf.set_samples(before, leaf_count=st0.leaf_count)
    opf.pf.w_slow, opf.pf.w_fast = st0.w_slow, st0.w_fast
    if pop:
        opf.set_population_size_parameters(*pop)
    out = opf.update_resample()
    M = out.sample_count
    print("single: M %d/%d leaf %d/%d bins %d/%d windows %d on_device %d draw launches %d" %
          (st1.sample_count, M, st1.leaf_count, out.leaf_count, st1.bin_count, out.node_count, st1.resample_windows,
           st1.kld_on_device, prof["draw"]["launches"]))
    assert out.status == 0
    assert (st1.sample_count, st1.leaf_count, st1.bin_count) == (M, out.leaf_count, out.node_count)
    assert np.array_equal(after[:, :3], opf.samples[:M, :3])
    assert np.all(after[:, 3] == 1.0 / M)
    assert rng1 == opf.pf.rng
    assert st1.last_status == 0
    return dict(M=M, leaf=st1.leaf_count, bins=st1.bin_count, samples=after, rng=rng1, windows=st1.resample_windows,
                on_device=st1.kld_on_device, draws=prof["draw"]["launches"])


def _world_resample(w):
    for e in w.engines:
        e.profile_reset()
    w.f.update_resample()
    prof = [e.profile_get() for e in w.engines]
    got = dict(M=w.f.sample_count, leaf=w.f.leaf_count, bins=w.f.bin_count, samples=np.concatenate(w.f.local_sets()),
               rng=w.f.rng_states(), windows=w.f.windows_used, miss=w.f.cdf_miss,
               draws=[p["draw"]["launches"] for p in prof], finalize=[p["finalize"]["launches"] for p in prof])
    print("world: M %d leaf %d bins %d windows %d draw launches %s finalize launches %s" %
          (got["M"], got["leaf"], got["bins"], got["windows"], got["draws"], got["finalize"]))
    return got


def _same_as_single(got, one, W):
    differing = -1
    if got["samples"].shape == one["samples"].shape:
        differing = int(np.any(got["samples"][:, :3] != one["samples"][:, :3], axis=1).sum())
    print("world against single: M %d/%d leaf %d/%d bins %d/%d differing poses %d" %
          (got["M"], one["M"], got["leaf"], one["leaf"], got["bins"], one["bins"], differing))
    assert (got["M"], got["leaf"], got["bins"]) == (one["M"], one["leaf"], one["bins"])
    assert np.array_equal(got["samples"][:, :3], one["samples"][:, :3])
    assert np.all(got["samples"][:, 3] == 1.0 / one["M"])
    assert got["rng"] == [one["rng"]] * W
    assert not got["miss"]


def _far_scenario(orc):
    """tests/test_gpu_parity.py::test_one_block_resample_declines_keys_beyond_its_packing: poses 5e6 m from the origin,
    whose histogram key floor(x / 0.5) fits neither the one-block kernels' 24 bits nor the device tree's packing."""
    sc = Scenario(orc, size=200, n=2000, beams=BEAMS, cloud="converged")
    sc.samples[:, 0] += 5.0e6
    sc.samples[:, 3] /= sc.samples[:, 3].sum()
    return sc


_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ------------------------------------------------------------------------------------------- the single engine, multinomial
def test_a_single_device_tree_declines_once_and_the_host_replays(orc):
    """(a) KLD_DEVICE_MIN = 1 and a first window that covers the whole stream (hint 4096 >= max 2000): the tracking
    attempt is skipped for the long stream, the whole-stream device tree is tried at m0 == 0 and declines the keys
    (more than the one launch of class "draw" a plain host window takes), the latch keeps it from being tried again and
    the host replay finishes in the same window: kld_on_device == 0.  (The issue's table expected the one-block kernel
    to decline first; with the hint at or above the maximum the driver does not try it.)"""
    sc = _far_scenario(orc)
    e, scn, pf, data, od = _single(sc, beams=BEAMS)
    try:
        _options([e], device_min=1)
        assert pf.getKldCount() == 0  # leaves mode
        one = _oracle_check(orc, pf, 2000)
        assert one["on_device"] == 0 and one["windows"] == 1
        assert one["draws"] > 1  # the device attempt's launches besides the replayed window's one
    finally:
        e.close()


def _spread_single(orc, n):
    """(b): a spread cloud, KLD_DEVICE_MIN = 1, two cycles, the second from the whole cloud again with the hint the
    first one left.  The records of both cycles, each checked against the oracle."""
    def make():
        sc = Scenario(orc, size=400, n=n, beams=BEAMS, cloud="spread")
        e, scn, pf, data, od = _single(sc, beams=BEAMS)
        try:
            _options([e], device_min=1)
            out = []
            for cycle in range(2):
                scn.updateSensor(pf, data)
                out.append(_oracle_check(orc, pf, n))
                pf.initWithSamples(sc.samples)
            return sc, out
        finally:
            e.close()
    return _cached(("spread", n), make)


def test_b_single_device_tree_after_the_first_window_then_at_the_start(orc):
    """(b) n = 6000, more than the 4096 draws of a first window: cycle 1 replays the first window on the host (the
    one-block kernel finds no stop in it) and hands the whole stream to the device tree after it (windows == 2,
    kld_on_device == 1); cycle 2 starts from hint >= max and takes the device tree at m0 == 0 (windows == 1)."""
    sc, (c1, c2) = _spread_single(orc, 6000)
    assert (c1["windows"], c1["on_device"]) == (2, 1)
    assert (c2["windows"], c2["on_device"]) == (1, 1)


def test_b_single_at_the_issue_size_takes_the_device_tree_at_the_start_in_both_cycles(orc):
    """(b) at n = 3000, the size the issue names: the first window max(1024, min(4096, 3000)) already covers the whole
    stream and the hint 4096 is >= max, so cycle 1 takes the device tree at m0 == 0 as well: windows == 1 in both
    cycles, where the issue's table expected 2 for the first."""
    sc, (c1, c2) = _spread_single(orc, 3000)
    assert (c1["windows"], c1["on_device"]) == (1, 1)
    assert (c2["windows"], c2["on_device"]) == (1, 1)


# ------------------------------------------------------------------------------------------- the sharded one-call form, multinomial
def _converged_single(orc):
    def make():
        sc = Scenario(orc, size=400, n=5000, beams=BEAMS, cloud="converged")
        e, scn, pf, data, od = _single(sc, beams=BEAMS)
        try:
            _options([e])
            scn.updateSensor(pf, data)
            return sc, _oracle_check(orc, pf, 5000)
        finally:
            e.close()
    return _cached("converged", make)


@pytest.mark.parametrize("W", [2, 3])
def test_c_sharded_tracking_window_is_adopted_by_the_stop_block(orc, W):
    """(c) converged n = 5000, fused resample on: one window, and k_shard_stop_block does the stop rule, the adoption
    and updateConverged -- the only launch of class "finalize"."""
    sc, one = _converged_single(orc)
    assert one["on_device"] == 2  # the single engine tracked too
    w = World(sc, W, beams=BEAMS)
    try:
        _options(w.engines)
        w.f.update_sensor(w.data)
        got = _world_resample(w)
        assert got["windows"] == 1 and got["draws"] == [1] * W and got["finalize"] == [1] * W
        _same_as_single(got, one, W)
    finally:
        w.close()


def _far_single(orc):
    def make():
        sc = _far_scenario(orc)
        e, scn, pf, data, od = _single(sc, beams=BEAMS)
        try:
            _options([e])
            scn.updateSensor(pf, data)
            return sc, _oracle_check(orc, pf, 2000)
        finally:
            e.close()
    return _cached("far", make)


@pytest.mark.parametrize("W", [2, 3])
def test_d_sharded_stop_block_declines_and_the_host_replays_the_same_window(orc, W):
    """(d) the far cloud of (a): the stop block reports keys beyond its packing, the host replays the same window and
    the tail adopts the set: one window, two launches of class "finalize"."""
    sc, one = _far_single(orc)
    assert one["on_device"] == 0
    w = World(sc, W, beams=BEAMS)
    try:
        _options(w.engines)
        w.f.update_sensor(w.data)
        got = _world_resample(w)
        assert got["windows"] == 1 and got["draws"] == [1] * W and got["finalize"] == [2] * W
        _same_as_single(got, one, W)
    finally:
        w.close()


POP_LOOSE, POP_DEFAULT = (0.05, 0.99), (0.01, 3.0)


def _two_step_single(orc):
    """tests/test_gpu_parity.py::test_stop_beyond_the_first_window_takes_sized_follow_up_windows"""
    def make():
        sc = Scenario(orc, size=400, n=20000, beams=BEAMS, cloud="converged")
        e, scn, pf, data, od = _single(sc, beams=BEAMS)
        try:
            _options([e], device_min=0)  # 0 = never
            pf.setPopulationSizeParameters(*POP_LOOSE)
            scn.updateSensor(pf, data)
            first = _oracle_check(orc, pf, 20000, pop=POP_LOOSE)
            pf.setPopulationSizeParameters(*POP_DEFAULT)
            pf.initWithSamples(sc.samples)
            scn.updateSensor(pf, data)
            return sc, first, _oracle_check(orc, pf, 20000, pop=POP_DEFAULT)
        finally:
            e.close()
    return _cached("two_step", make)


@pytest.mark.parametrize("W", [2, 3])
def test_e_sharded_stop_in_the_second_window_is_adopted_from_the_kept_buffer(orc, W):
    """(e) a loose bound first (a set below 800, so the next hint is the minimum window of 1024), then the default
    bound on the full cloud, whose stop lies beyond 1024 draws, device tree off: the stop block finds no stop in the
    first window, the host replays it and a follow-up window, both windows' poses are kept (d_shard_out) and the tail
    adopts the set from there: two windows, two launches of class "finalize"."""
    sc, first, one = _two_step_single(orc)
    assert first["M"] < 800 and one["M"] > 1024 and (one["windows"], one["on_device"]) == (2, 0)
    w = World(sc, W, beams=BEAMS)
    try:
        _options(w.engines, device_min=0)
        for pf in w.f.pfs:
            pf.setPopulationSizeParameters(*POP_LOOSE)
        w.f.update_sensor(w.data)
        _same_as_single(_world_resample(w), first, W)
        hint = list(w.f.window_hint)
        assert hint == [1024] * W
        for pf in w.f.pfs:
            pf.setPopulationSizeParameters(*POP_DEFAULT)
        w.f.load([sc.samples[w.cuts[r]:w.cuts[r + 1]] for r in range(W)])
        w.f.window_hint = hint  # (load starts a new filter's hint; the single engine's initWithSamples keeps it)
        w.f.update_sensor(w.data)
        got = _world_resample(w)
        assert got["windows"] == 2 and got["draws"] == [2] * W and got["finalize"] == [2] * W
        _same_as_single(got, one, W)
    finally:
        w.close()


def _spread_world_cycles(orc, n, W):
    """(f), (g): the input of (b) through the sharded filter, both cycles against the single engine's."""
    sc, ref = _spread_single(orc, n)
    w = World(sc, W, beams=BEAMS)
    try:
        _options(w.engines, device_min=1)
        out = []
        for cycle in range(2):
            w.f.update_sensor(w.data)
            got = _world_resample(w)
            _same_as_single(got, ref[cycle], W)
            out.append(got)
            hint = list(w.f.window_hint)
            w.f.load([sc.samples[w.cuts[r]:w.cuts[r + 1]] for r in range(W)])
            w.f.window_hint = hint
        return out, ref
    finally:
        w.close()


@pytest.mark.parametrize("W", [2, 3])
def test_f_g_sharded_whole_stream_device_window_only_after_a_first_window(orc, W):
    """(f) n = 6000, cycle 1: the stop block declines the first window of 4096, the host replays it, and the whole
    stream goes to the device tree in a second window (windows == 2, three launches of class "draw" at least: two
    windows and the tree).
    (g) cycle 2 starts from hint >= max, where the single engine takes the device tree at m0 == 0 with windows == 1
    (case b).  The sharded driver does NOT: it never hands the stream to the device before a first host window, so it
    replays a first window of 4096 (no stop block: the hint is beyond its size) and then takes the whole-stream window:
    windows == 2.  A known difference between the two drivers; the results are the same."""
    (c1, c2), ref = _spread_world_cycles(orc, 6000, W)
    assert c1["windows"] == 2 and c1["finalize"] == [2] * W and min(c1["draws"]) >= 3
    assert ref[1]["windows"] == 1
    assert c2["windows"] == 2 and c2["finalize"] == [1] * W and min(c2["draws"]) >= 3


@pytest.mark.parametrize("W", [2, 3])
def test_f_g_sharded_at_the_issue_size_never_reaches_the_device_tree(orc, W):
    """(f), (g) at n = 3000, the size the issue names: the first window covers the whole stream, so the loop ends
    after the host's replay of it in both cycles (windows == 1, where the issue's table expected 2 for (f)): the stop
    block is tried and declines, the tail adopts.  The single engine took the device tree for the same input."""
    (c1, c2), ref = _spread_world_cycles(orc, 3000, W)
    for got in (c1, c2):
        assert got["windows"] == 1 and got["draws"] == [1] * W and got["finalize"] == [2] * W


# ------------------------------------------------------------------------------------------- w_diff > 0: the stream account
N_RECOVERY = 2500
ALPHA = (0.001, 0.1)


def _recovery_scans(sc):
    # scan 1 fits the map, scans 2 and 3 are progressively worse: w_fast falls below w_slow
    return [sc.ranges, np.clip(sc.ranges * 0.6, 0.05, 29.0), np.full(sc.ranges.shape[0], 1.0)]


def _recovery_single(orc, resampler):
    """tests/test_gpu_parity.py::test_recovery_random_poses_match_oracle at n = 2500: three cycles of the single engine,
    every resample against the oracle (which scores nothing: it resamples the device's set)."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf

    def make():
        sc = Scenario(orc, size=200, n=N_RECOVERY, beams=BEAMS, cloud="mixture")
        e, scn, pf, data, od = _single(sc, resampler=resampler, alpha=ALPHA, beams=BEAMS)
        try:
            _options([e])
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            opf = orc.ParticleFilter(100, N_RECOVERY, ALPHA[0], ALPHA[1], 85.0, seed=SEED)
            opf.set_resample_model(resampler)
            opf.set_samples(sc.samples)
            assert opf.set_random_pose_source(sc.omap, sc.map_factors[2]) > 1000
            out = []
            for ranges in _recovery_scans(sc):
                scn.updateSensor(pf, bpf.PlanarData(ranges, sc.angles, sc.range_max))
                st0 = pf.getState()
                opf.set_samples(pf.getCurrentSet().samples, leaf_count=st0.leaf_count)
                opf.pf.w_slow, opf.pf.w_fast = st0.w_slow, st0.w_fast
                opf.pf.rng = pf.getRngState()
                pf.updateResample()
                res = opf.update_resample()
                st1, after = pf.getState(), pf.getCurrentSet().samples.copy()
                M = res.sample_count
                print("recovery single: w_diff %.4f M %d/%d rng equal %d" %
                      (res.w_diff, st1.sample_count, M, pf.getRngState() == opf.pf.rng))
                assert res.status == 0 and abs(st1.w_diff - res.w_diff) <= 1e-12
                assert (st1.sample_count, st1.leaf_count, st1.bin_count) == (M, res.leaf_count, res.node_count)
                assert np.array_equal(after[:, :3], opf.samples[:M, :3]) and np.all(after[:, 3] == 1.0 / M)
                assert pf.getRngState() == opf.pf.rng  # the stream account with random pose calls
                out.append(dict(M=M, leaf=st1.leaf_count, bins=st1.bin_count, samples=after, rng=pf.getRngState(),
                                w_diff=res.w_diff, n_random=int((opf.last_idx < 0).sum())))
            assert max(r["w_diff"] for r in out) > 0.01  # the recovery branch really ran ...
            assert max(r["n_random"] for r in out) > 0    # ... and made random pose calls
            return sc, out
        finally:
            e.close()
    return _cached(("recovery", resampler), make)


@pytest.mark.parametrize("resampler", [1, 0])
def test_h_single_recovery_rng_state_equals_the_oracle(orc, resampler):
    """(h) w_diff > 0: the systematic resampler's account (1 + (2 retries + 2) n_random elements) and, beside what the
    issue lists, the multinomial one's (the chain word of the last draw)."""
    _recovery_single(orc, resampler)


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("resampler", [1, 0])
def test_h_sharded_recovery_rng_state_equals_the_single_engine(orc, resampler, W):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    sc, ref = _recovery_single(orc, resampler)
    w = World(sc, W, resampler=resampler, alpha=ALPHA, beams=BEAMS)
    try:
        _options(w.engines)
        w.f.set_random_pose_generator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        for one, ranges in zip(ref, _recovery_scans(sc)):
            w.f.update_sensor(bpf.PlanarData(ranges, sc.angles, sc.range_max))
            _same_as_single(_world_resample(w), one, W)
    finally:
        w.close()
