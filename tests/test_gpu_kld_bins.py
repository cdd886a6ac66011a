"""The opt-in occupied-bin KLD count (BPF_KLD_COUNT_BINS) on the device: every form of the stop rule -- the
single-block kernel, the host's window replay, the lean device pipeline for long streams -- against the Python
restatement in kld_bins_ref.py, bit for bit (sample count, poses, counts, drand48 state), with the form asserted.
LEAVES steps around BINS steps still equal the oracle, and ranks on one GPU equal the single engine in BINS mode."""
import os
import socket
import sys

import numpy as np
import pytest

from badger_amcl_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kld_bins_ref as kref  # noqa: E402
import pose_check_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu
CELL_TH = 10 * np.pi / 180
FORM_HOST, FORM_DEVICE, FORM_BLOCK = 0, 1, 2  # bpf_pf_state.kld_on_device
ALPHA = (0.001, 0.1)  # the node's default recovery decay rates


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _cells_set(n, n_bins, seed):
    """n poses at the centres of n_bins distinct histogram cells (pose i in cell i mod n_bins), random weights."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(200 * 200 * 36, size=n_bins, replace=False)
    cells = np.stack([flat % 200, (flat // 200) % 200, flat // 40000], 1)
    k = np.arange(n) % n_bins
    s = np.empty((n, 4))
    s[:, 0] = (cells[k, 0] + 0.5) * 0.5
    s[:, 1] = (cells[k, 1] + 0.5) * 0.5
    s[:, 2] = (cells[k, 2] + 0.5) * CELL_TH - np.pi
    s[:, 3] = rng.uniform(0.5, 1.5, n)
    s[:, 3] /= s[:, 3].sum()
    return s


def _weighted(s, seed):
    s = s.copy()
    s[:, 3] = np.random.default_rng(seed).uniform(0.5, 1.5, s.shape[0])
    s[:, 3] /= s[:, 3].sum()
    return s


def _step(orc, pf, opf, samples, resampler, mode):
    """One updateResample of `samples` (the filter's current set) against the restatement; returns the state."""
    count0 = kref.set_count(samples, mode, orc.KDTree)
    r = kref.Rng(pf.getRngState())
    pf.updateResample()
    st = pf.getState()
    out = pf.getCurrentSet().samples
    want, k, leaf, nodes, _ = kref.resample(samples, count0, 0.0, r, None, resampler, opf, orc.KDTree, mode)
    assert st.sample_count == len(want)
    assert np.array_equal(out[:, :3], np.array(want))
    assert st.bin_count == nodes and st.leaf_count == k
    assert st.leaf_count == (nodes if mode == kref.BINS else leaf)
    assert pf.getRngState() == r.s
    return st


def _run(engine, orc, samples, resampler, min_s, max_s, mode=kref.BINS, fused=1, kld_min=8192, pop=None, seed=11):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)  # the restatement's serial CDF
    engine.set_option(hpf.OPT_FUSED_RESAMPLE, fused)
    engine.set_option(hpf.OPT_KLD_DEVICE_MIN, kld_min)
    try:
        pf = bpf.ParticleFilter(engine, min_s, max_s, 0.0, 0.0, 85.0)
        opf = orc.ParticleFilter(min_s, max_s, seed=seed)
        if pop is not None:
            pf.setPopulationSizeParameters(*pop)
            opf.set_population_size_parameters(*pop)
        pf.setResampleModel(resampler)
        pf.srand48(seed)
        pf.setKldCount(mode)
        assert pf.getKldCount() == mode
        pf.initWithSamples(samples)
        return _step(orc, pf, opf, samples, resampler, mode), engine.kld_last_form()
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
        engine.set_option(hpf.OPT_FUSED_RESAMPLE, 1)
        engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 8192)


@pytest.mark.parametrize("resampler", [0, 1])
def test_block_form(engine, orc, resampler):
    s = _weighted(synth.converged_cloud(3000, (5.0, 5.0, 0.3), seed=3), 4)
    st, _ = _run(engine, orc, s, resampler, 100, 3000)
    assert st.kld_on_device == FORM_BLOCK


@pytest.mark.parametrize("resampler", [0, 1])
def test_host_window_form(engine, orc, resampler):
    s = _weighted(synth.converged_cloud(3000, (5.0, 5.0, 0.3), seed=5), 6)
    st, _ = _run(engine, orc, s, resampler, 100, 3000, fused=0)
    assert st.kld_on_device == FORM_HOST


def test_block_form_more_than_1024_bins(engine, orc):
    """A window with > 1 024 distinct bins that stops inside 4 096 draws: the LEAVES block declines such a window
    (kFusedMaxBins), the BINS block takes it, reading the limits beyond the LDS table from the global one."""
    s = _cells_set(3000, 2000, 7)
    st, _ = _run(engine, orc, s, 0, 100, 4096, pop=(0.3, 0.99))
    assert st.kld_on_device == FORM_BLOCK
    assert 1024 < st.bin_count and st.sample_count < 4096


def test_device_long_stream_spread_100k(engine, orc):
    s = _weighted(synth.spread_cloud(100_000, 400, 0.05, seed=8), 9)
    st, form = _run(engine, orc, s, 0, 500, 100_000, kld_min=1)
    assert st.kld_on_device == FORM_DEVICE and form == 4


def test_device_long_stream_stops_inside(engine, orc):
    """A looser bound (pop_err 0.3) puts the BINS stop inside the device stream: k_kld_bins_scan's stop test and the
    count at the stop, not just the count of a whole stream."""
    s = _weighted(synth.spread_cloud(100_000, 400, 0.05, seed=8), 9)
    st, form = _run(engine, orc, s, 0, 500, 100_000, kld_min=1, pop=(0.3, 0.99))
    assert st.kld_on_device == FORM_DEVICE and form == 4
    assert 4096 < st.sample_count < 100_000


def test_invalid_mode_leaves_the_mode(engine):
    import badger_amcl_amd as bpf
    pf = bpf.ParticleFilter(engine, 100, 500, 0.0, 0.0, 85.0)
    pf.setKldCount(kref.BINS)
    for bad in (2, -1):
        with pytest.raises(bpf.BpfError) as ei:
            pf.setKldCount(bad)
        assert ei.value.code == 1  # BPF_ERR_INVALID_ARGUMENT
        assert pf.getKldCount() == kref.BINS
    pf.setKldCount(kref.LEAVES)


def test_switch_marks_the_count_stale(engine, orc):
    """LEAVES resample, switch to BINS, then a systematic resample of the SAME set: its size must come from the bin
    count of the current set (computed again after the switch), not from the leaf count the last resample left."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = 3000
    s = _weighted(synth.spread_cloud(n, 200, 0.05, seed=16), 17)
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    try:
        pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
        opf = orc.ParticleFilter(100, n, seed=1)
        opf.set_population_size_parameters(0.3, 0.99)
        pf.setPopulationSizeParameters(0.3, 0.99)
        pf.srand48(5)
        pf.initWithSamples(s)
        st0 = _step(orc, pf, opf, s, 0, kref.LEAVES)
        cur = pf.getCurrentSet().samples.copy()
        assert st0.leaf_count < st0.bin_count
        pf.setKldCount(kref.BINS)
        pf.setResampleModel(1)
        assert pf.getState().leaf_count == st0.bin_count == kref.set_count(cur, kref.BINS, orc.KDTree)
        _step(orc, pf, opf, cur, 1, kref.BINS)
        pf.setKldCount(kref.LEAVES)
        cur = pf.getCurrentSet().samples.copy()
        _step(orc, pf, opf, cur, 1, kref.LEAVES)  # and back: the leaf count of the current set
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)


def _check_recovery(orc, pf, opf, fs, g0, m, resampler):
    """One BINS pf.updateResample() with recovery draws against the restatement (AS_REFERENCE pose check);
    returns (w_diff, state)."""
    cur = pf.getCurrentSet().samples.copy()
    st0 = pf.getState()
    assert st0.leaf_count == st0.bin_count == kref.set_count(cur, kref.BINS, orc.KDTree)
    w_diff = 1.0 - st0.w_fast / st0.w_slow if st0.w_slow != 0.0 else 0.0
    if not (w_diff >= 0.0):
        w_diff = 0.0
    r = kref.Rng(pf.getRngState())
    pf.updateResample()
    st1 = pf.getState()
    want, k, leaf, nodes, rnd = kref.resample(cur, st0.leaf_count, w_diff, r, pref.FastGen(fs, g0, m), resampler, opf,
                                              orc.KDTree, kref.BINS)
    M = len(want)
    assert st1.w_diff == w_diff
    assert st1.sample_count == M
    assert st1.leaf_count == st1.bin_count == nodes == k
    after = pf.getCurrentSet().samples
    assert np.array_equal(after[:, :3], np.array(want))
    assert np.all(after[:, 3] == 1.0 / M)
    assert pf.getRngState() == r.s
    if w_diff > 0:
        assert sum(rnd) > 0
    return w_diff, st1


@pytest.mark.parametrize("resampler,device_kld,n", [(0, False, 2500), (0, True, 2500), (1, False, 2500),
                                                    (1, False, 10000)])
def test_recovery_with_pose_check(engine, orc, resampler, device_kld, n):
    """w_diff > 0 with BPF_POSE_CHECK_AS_REFERENCE and K = 4: the BINS stop over the recovery draw chain (host
    windows, and the device stream), the systematic resampler's random poses with the new set counted on the host
    (2 500) and on the device (10 000), against the restatement."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    g0, mult = 10.0, 0.5
    assert pref.retries(g0, mult) == 4
    sc_ = Scenario(orc, size=200, n=n, beams=61, cloud="mixture")
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 1 if device_kld else 8192)
    try:
        m_, sc, pf, data = sc_.gpu_objects(engine, 61, "lf", min_samples=100, seed=31, alpha=ALPHA)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
        pf.setUniformPoseCheck(g0, mult)
        pf.setKldCount(kref.BINS)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=31)
        fs = pref.FreeSpace.planar(pref.free_cells_2d(sc_.cells, sc_.lut, sc_.map_factors[2]), sc_.size, sc_.size,
                                   sc_.origin, sc_.res)
        scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0)]
        seen = []
        for ranges in scans:
            sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
            w_diff, st = _check_recovery(orc, pf, opf, fs, g0, mult, resampler)
            seen.append((w_diff, st.kld_on_device, engine.kld_last_form()))
        assert max(w for w, _, _ in seen) > 0.01
        recovered = [(f, lf) for w, f, lf in seen if w > 0.0]
        if device_kld:
            assert all(f == FORM_DEVICE and lf == 4 for f, lf in recovered)
        if resampler == 1 and n >= 8192:
            assert any(f == FORM_DEVICE and lf == 4 for f, lf in recovered)  # the new set counted on the device
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)
        engine.set_option(hpf.OPT_KLD_DEVICE_MIN, 8192)


@pytest.mark.parametrize("resampler", [0, 1])
def test_point_cloud_steps(orc, resampler):
    """3-D steps in BINS mode: point-cloud updates on the 3-D map, recovery draws from its free space (K = 4)."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_pose_check import _cloud_setup
    e = bpf.Engine(0)
    try:
        n = 2000
        g0, mult = 10.0, 0.5
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        om, sc, pts, s, fs = _cloud_setup(e, orc, n)
        pf = bpf.ParticleFilter(e, 100, n, ALPHA[0], ALPHA[1], 85.0)
        pf.srand48(11)
        pf.setResampleModel(resampler)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.setUniformPoseCheck(g0, mult)
        pf.setKldCount(kref.BINS)
        pf.initWithSamples(s)
        opf = orc.ParticleFilter(100, n, ALPHA[0], ALPHA[1], 85.0, seed=11)
        w_diffs = []
        for scan in (pts, pts * np.float32(0.5), pts * np.float32(0.3)):
            assert sc.updateSensor(pf, bpf.PointCloudData(np.ascontiguousarray(scan)))
            w_diffs.append(_check_recovery(orc, pf, opf, fs, g0, mult, resampler)[0])
        assert max(w_diffs) > 0.01
    finally:
        e.close()


def test_keys_outside_the_packing_range(engine, orc):
    """x far off the 24-bit key packing: block and device decline, the host replay takes the stream."""
    s = _weighted(synth.spread_cloud(20_000, 400, 0.05, seed=10), 11)
    s[::7, 0] += 1.0e7
    st, _ = _run(engine, orc, s, 0, 500, 20_000, kld_min=1)
    assert st.kld_on_device == FORM_HOST


def test_systematic_spread_1m(engine, orc):
    """A spread 1 M set: its count on the device (the key hash and one scan), then the systematic draws."""
    s = _weighted(synth.spread_cloud(1_000_000, 1000, 0.05, seed=12), 13)
    st, form = _run(engine, orc, s, 1, 500, 1_000_000)
    assert form == 4 and st.kld_on_device == FORM_DEVICE  # the new set's count came from the device too


def test_leaves_bins_leaves_on_one_engine(engine, orc):
    """LEAVES -> BINS -> LEAVES on one filter: the LEAVES steps equal the oracle, the BINS step the restatement."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = 3000
    cur = _weighted(synth.converged_cloud(n, (5.0, 5.0, 0.3), seed=14), 15)
    engine.set_option(hpf.OPT_CDF_SERIAL, 1)
    try:
        pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
        opf = orc.ParticleFilter(100, n, seed=1)
        pf.srand48(21)
        pf.initWithSamples(cur)
        for step, mode in enumerate((kref.LEAVES, kref.BINS, kref.LEAVES)):
            pf.setKldCount(mode)
            o = orc.ParticleFilter(100, n, seed=1)
            o.set_samples(cur)
            o.pf.rng = pf.getRngState()
            st = _step(orc, pf, opf, cur, 0, mode)
            if mode == kref.LEAVES:
                out = o.update_resample()
                M = out.sample_count
                assert st.sample_count == M and st.leaf_count == out.leaf_count and st.bin_count == out.node_count
                assert np.array_equal(pf.getCurrentSet().samples[:, :3], o.samples[:M, :3])
                assert int(o.pf.rng) == pf.getRngState()
            cur = _weighted(pf.getCurrentSet().samples, 30 + step)
            pf.initWithSamples(cur)
        assert pf.getKldCount() == kref.LEAVES
    finally:
        engine.set_option(hpf.OPT_CDF_SERIAL, 0)


# ---- ranks on one GPU against the single engine, BINS mode
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scenario(cloud):
    from oracle import pyoracle as orc
    from scenario import Scenario
    return orc, Scenario(orc, size=400, n=6000, beams=181, cloud=cloud)


def _shard_worker(rank, world, port, out_dir, resampler, exchange, cloud, device_min=None, pop=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    from scenario import Scenario
    _, sc = _scenario(cloud)
    n = sc.samples.shape[0]
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world
    e = bpf.Engine(0)
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    m, scn, pf, data = shard.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21)
    pf.setResampleModel(resampler)
    if pop is not None:
        pf.setPopulationSizeParameters(*pop)
    b = HipShardBackend(e, scn, pf, torch.device("cuda", 0))
    if device_min is not None:
        b.kld_device_min = device_min
    sf = ShardedFilter(b, dist, first_window=1024, exchange=exchange, kld_count=hpf.KLD_COUNT_BINS)
    recs = []
    for _ in range(2):
        sf.update_sensor(data)
        sf.update_resample()
        st = sf.state()
        recs.append(dict(samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                         bins=st.bin_count, rng=pf.getRngState(), form=e.kld_last_form()))
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(recs, dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


@pytest.mark.parametrize("world,exchange,cloud,resampler,device_min", [(2, "mailbox", "converged", 0, None),
                                                                       (2, "mailbox", "converged", 1, None),
                                                                       (3, "collective", "spread", 0, None),
                                                                       (2, "collective", "spread", 1, None),
                                                                       (3, "mailbox", "spread", 0, None),
                                                                       (2, "collective", "spread", 0, 512)])
def test_ranks_equal_single_engine_bins(tmp_path, engine, world, exchange, cloud, resampler, device_min):
    """device_min: the stage path's stop on the device (bpf_kld_stop_dev) with a looser bound (pop_err 0.3), so that
    it stops inside the stream."""
    import torch.multiprocessing as mp
    import badger_amcl_amd.pf as hpf
    pop = (0.3, 0.99) if device_min is not None else None
    orc, sc = _scenario(cloud)
    n = sc.samples.shape[0]
    m, scn, pf, data = sc.gpu_objects(engine, 181, "lf", min_samples=100, max_samples=n, seed=21)
    pf.setResampleModel(resampler)
    if pop is not None:
        pf.setPopulationSizeParameters(*pop)
    pf.setKldCount(hpf.KLD_COUNT_BINS)
    ref = []
    for _ in range(2):
        scn.updateSensor(pf, data)
        pf.updateResample()
        st = pf.getState()
        ref.append(dict(samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                        bins=st.bin_count, rng=pf.getRngState()))
    mp.spawn(_shard_worker, args=(world, _free_port(), str(tmp_path), resampler, exchange, cloud, device_min, pop),
             nprocs=world, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r), allow_pickle=True) for r in range(world)]
    for cycle in range(2):
        want = ref[cycle]
        assert want["leaf"] == want["bins"]
        for r in range(world):
            got = recs[r][cycle]
            assert (got["M"], got["leaf"], got["bins"], got["rng"]) == (want["M"], want["leaf"], want["bins"],
                                                                        want["rng"])
        merged = np.concatenate([recs[r][cycle]["samples"] for r in range(world)])
        assert np.array_equal(merged[:, :3], want["samples"][:, :3])
    if device_min is not None:
        # every rank stopped on the device (the BINS pipeline) inside the stream, in at least one cycle
        assert any(all(recs[r][c]["form"] == 4 for r in range(world)) and ref[c]["M"] < n for c in range(2)), \
            [(ref[c]["M"], [recs[r][c]["form"] for r in range(world)]) for c in range(2)]
