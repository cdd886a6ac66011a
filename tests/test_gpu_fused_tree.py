"""The single-block resample's histogram tree of at most 64 keys: grown in wave 0's registers (default) against the
LDS form with atomics (BPF_OPT_FUSED_LDS_TREE = 1) and against the general path (BPF_OPT_FUSED_RESAMPLE = 0), on the
same windows.  Sets, counts, convergence and the drand48 state must be equal bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

N = 3000            # set size = max_samples: the whole candidate stream is one window of the single-block kernel
CELL_TH = 10 * np.pi / 180


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _bins_set(n_bins, layout, seed):
    """n poses (equal weights) on exactly n_bins histogram cells: cell centres, cell k = pose index mod n_bins."""
    rng = np.random.default_rng(seed)
    if layout == "line":
        # keys along one axis in index order: drawn in that order (systematic) the tree is a chain of n_bins levels
        cells = np.stack([np.arange(n_bins), np.zeros(n_bins, int), np.zeros(n_bins, int)], 1)
    else:
        flat = rng.choice(12 * 12 * 6, size=n_bins, replace=False)
        cells = np.stack([flat % 12, (flat // 12) % 12, flat // 144], 1)
    k = np.arange(N) % n_bins
    s = np.empty((N, 4))
    s[:, 0] = (cells[k, 0] + 0.5) * 0.5 + 1.0
    s[:, 1] = (cells[k, 1] + 0.5) * 0.5 + 1.0
    s[:, 2] = (cells[k, 2] + 0.5) * CELL_TH
    s[:, 3] = 1.0 / N
    return s


def _resample(engine, samples, resampler, min_s, fused, lds_tree, cycles=2):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    engine.set_option(hpf.OPT_FUSED_RESAMPLE, fused)
    engine.set_option(hpf.OPT_FUSED_LDS_TREE, lds_tree)
    try:
        pf = bpf.ParticleFilter(engine, min_s, N, 0.0, 0.0, 85.0)
        pf.setResampleModel(resampler)
        pf.srand48(11)
        pf.initWithSamples(samples)
        log = []
        for _ in range(cycles):
            pf.updateResample()
            st = pf.getState()
            log.append((pf.getCurrentSet().samples.copy(), st.sample_count, st.leaf_count, st.bin_count,
                        st.converged, pf.getRngState(), st.kld_on_device))
            cur = pf.getCurrentSet().samples
            cur[:, 3] = 1.0 / cur.shape[0]
            pf.initWithSamples(cur)  # (the next cycle draws from the new set again)
        return log
    finally:
        engine.set_option(hpf.OPT_FUSED_RESAMPLE, 1)
        engine.set_option(hpf.OPT_FUSED_LDS_TREE, 0)


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1:6] == b[1:6]


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("min_s", [10, N])   # an early stop, and the whole window (bins = every key of the window)
@pytest.mark.parametrize("n_bins,layout", [(1, "grid"), (2, "grid"), (63, "grid"), (64, "grid"), (65, "grid"),
                                           (64, "line"), (40, "line")])
def test_register_tree_equals_lds_tree(engine, resampler, min_s, n_bins, layout):
    s = _bins_set(n_bins, layout, seed=n_bins)
    reg = _resample(engine, s, resampler, min_s, 1, 0)
    lds = _resample(engine, s, resampler, min_s, 1, 1)
    gen = _resample(engine, s, resampler, min_s, 0, 0)
    for c in range(len(reg)):
        _same(reg[c], lds[c])
        _same(reg[c], gen[c])
        assert reg[c][6] == 2 and lds[c][6] == 2  # the single-block kernel ran
    if min_s == N and resampler == 0:
        assert reg[0][1] == N and reg[0][3] == n_bins  # the window held exactly n_bins distinct keys


def test_register_tree_random_windows(engine):
    """Converged clouds of varying width: windows of 1 .. ~100 distinct bins, both tree forms and both resamplers."""
    from badger_amcl_amd import synth
    for k, sig in enumerate([0.01, 0.1, 0.3, 0.6, 1.0, 1.5]):
        s = synth.converged_cloud(N, (5.0, 5.0, 0.3), seed=300 + k, sigma=(sig, sig, sig / 3))
        s[:, 3] = np.random.default_rng(k).uniform(0.5, 1.5, N)
        s[:, 3] /= s[:, 3].sum()
        for resampler in (0, 1):
            reg = _resample(engine, s, resampler, 10, 1, 0, cycles=3)
            lds = _resample(engine, s, resampler, 10, 1, 1, cycles=3)
            for c in range(3):
                _same(reg[c], lds[c])


def test_register_tree_after_a_recovery_step(engine, orc):
    """w_diff > 0 on the middle cycle (general path with random poses), single-block resamples around it: the two tree
    forms give the same filter throughout."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from scenario import Scenario
    sc_ = Scenario(orc, size=200, n=2500, beams=61, cloud="mixture")
    runs = []
    for lds_tree in (0, 1):
        engine.set_option(hpf.OPT_FUSED_LDS_TREE, lds_tree)
        try:
            m, sc, pf, data = sc_.gpu_objects(engine, 61, "lf", min_samples=100, seed=31, alpha=(0.001, 0.1))
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            scans = [sc_.ranges, np.clip(sc_.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0), sc_.ranges, sc_.ranges]
            log = []
            for ranges in scans:
                sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max))
                pf.updateResample()
                st = pf.getState()
                log.append((pf.getCurrentSet().samples.copy(), st.sample_count, st.leaf_count, st.bin_count,
                            st.converged, pf.getRngState(), st.w_diff, st.kld_on_device))
            runs.append(log)
        finally:
            engine.set_option(hpf.OPT_FUSED_LDS_TREE, 0)
    for a, b in zip(*runs):
        _same(a, b)
        assert a[6] == b[6]
    assert max(r[6] for r in runs[0]) > 0.01          # the recovery branch ran
    assert sum(r[7] == 2 for r in runs[0]) >= 1       # and so did the single-block kernel


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, out_dir, lds_tree, resampler):
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
    from oracle import pyoracle as orc
    from scenario import Scenario
    sc = Scenario(orc, size=400, n=6000, beams=181, cloud="converged")
    n = sc.samples.shape[0]
    lo, hi = (n * rank) // world, (n * (rank + 1)) // world
    e = bpf.Engine(0)
    e.set_option(hpf.OPT_FUSED_LDS_TREE, lds_tree)
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    m, scn, pf, data = shard.gpu_objects(e, 181, "lf", min_samples=100, max_samples=n, seed=21)
    pf.setResampleModel(resampler)
    sf = ShardedFilter(HipShardBackend(e, scn, pf, torch.device("cuda", 0)), dist, first_window=1024,
                       exchange="mailbox")
    recs = []
    for cycle in range(3):
        sf.update_sensor(data)
        sf.update_resample()
        st = sf.state()
        recs.append(dict(samples=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count,
                         bins=st.bin_count, rng=pf.getRngState(), conv=st.converged))
    np.save(os.path.join(out_dir, "rank%d_lds%d.npy" % (rank, lds_tree)), np.array(recs, dtype=object),
            allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


@pytest.mark.parametrize("resampler", [0, 1])
def test_register_tree_sharded_stop_block_two_ranks(tmp_path, resampler):
    """k_shard_resample_block / k_shard_stop_block share the stop rule: two ranks on one GPU, both tree forms."""
    import torch.multiprocessing as mp
    for lds_tree in (0, 1):
        mp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path), lds_tree, resampler), nprocs=2, join=True)
    recs = {(r, t): np.load(os.path.join(str(tmp_path), "rank%d_lds%d.npy" % (r, t)), allow_pickle=True)
            for r in range(2) for t in range(2)}
    for cycle in range(3):
        for r in range(2):
            a, b = recs[(r, 0)][cycle], recs[(r, 1)][cycle]
            assert np.array_equal(a["samples"], b["samples"])
            assert (a["M"], a["leaf"], a["bins"], a["rng"], a["conv"]) == (b["M"], b["leaf"], b["bins"], b["rng"],
                                                                           b["conv"])
        assert recs[(0, 0)][cycle]["M"] == recs[(1, 0)][cycle]["M"]
