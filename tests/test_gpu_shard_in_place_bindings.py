"""The in-place systematic resample through the two Python bindings that take the engine's one-call form
(bpf_shard_update_resample with BPF_SHARD_RESAMPLE_IN_PLACE): local_world.LocalShardedFilter with all ranks in this
process, and ShardedFilter over the mailbox in two processes.  Each: sensor update, resample, then a motion update on
the uneven slices, against one engine whose set is rotated in between (shard_in_place_ref.rotate)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import shard_in_place_ref as ipr  # noqa: E402
from scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu

ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion
SEED, N, BEAMS = 21, 3000, 60  # the scenario, seed and even splits tests/cpp/shard_in_place.cpp runs


def _scenario(orc):
    return Scenario(orc, size=200, n=N, beams=BEAMS, cloud="converged")


def _shard_of(sc, lo, hi):
    shard = Scenario.__new__(Scenario)
    shard.__dict__.update(sc.__dict__)
    shard.samples = np.ascontiguousarray(sc.samples[lo:hi])
    return shard


def _rank_objects(sc, e, lo, hi):
    import badger_amcl_amd as bpf
    m, scn, pf, data = _shard_of(sc, lo, hi).gpu_objects(e, BEAMS, "lf", min_samples=100, max_samples=N, seed=SEED)
    pf.setResampleModel(1)
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    return m, scn, pf, data, od


def _single_reference(sc):
    """One engine: (rotated new set, M, rng after the resample, leaf, bins, converged, the rotated set after a motion
    update on it)."""
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    try:
        m, scn, pf, data, od = _rank_objects(sc, e, 0, N)
        scn.updateSensor(pf, data)
        rng0 = pf.getRngState()
        pf.updateResample()
        st = pf.getState()
        S = pf.getCurrentSet().samples
        M = st.sample_count
        _, i_wrap, _ = ipr.target_chain(rng0, M)
        want = ipr.rotate(S, 0, i_wrap)
        rng = pf.getRngState()
        pf.initWithSamples(want, -1)  # the rotated set: what the ranks hold
        pf.setRngState(rng)
        st2 = pf.getState()
        od.updateAction(pf, bpf.OdomData(*ODATA))
        moved = pf.getCurrentSet().samples
        return dict(want=want, M=M, rng=rng, leaf=st2.leaf_count, bins=st2.bin_count, conv=st.converged, moved=moved,
                    rng_moved=pf.getRngState())
    finally:
        e.close()


def _sets(parts):
    return np.concatenate([p for p in parts if p.shape[0] > 0])


def test_local_sharded_filter_in_place(orc):
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    sc, W = _scenario(orc), 8
    ref = _single_reference(sc)
    cuts = [(N * r) // W for r in range(W + 1)]
    engines = [bpf.Engine(0) for _ in range(W)]
    f = None
    try:
        keep = [_rank_objects(sc, e, cuts[r], cuts[r + 1]) for r, e in enumerate(engines)]
        f = LocalShardedFilter([k[2] for k in keep], resample_form="in_place", max_share=float(W))
        f.load([sc.samples[cuts[r]:cuts[r + 1]] for r in range(W)])
        with pytest.raises(bpf.BpfError):
            f.slice(0)  # slices loaded by hand: nobody has told the engine where they sit
        f.update_sensor(keep[0][3])
        before = f.exchange_counts()
        f.update_resample()
        assert [a - b for a, b in zip(f.exchange_counts(), before)] == [4] * W
        got = _sets(f.local_sets())
        assert got.shape == ref["want"].shape and np.array_equal(got[:, :3], ref["want"][:, :3])
        assert np.all(got[:, 3] == 1.0 / ref["M"])
        assert f.form_used == "in_place" and f.windows_used == 0 and not f.cdf_miss
        assert (f.sample_count, f.leaf_count, f.bin_count) == (ref["M"], ref["leaf"], ref["bins"])
        assert sum(f.counts) == ref["M"]
        for r in range(W):
            assert f.slice(r) == (sum(f.counts[:r]), f.counts[r], ipr.IN_PLACE)
            assert f.pfs[r].getState().sample_count == f.counts[r]
        assert set(f.rng_states()) == {ref["rng"]} and f.state().converged == ref["conv"]
        # the step after it takes the slices where they are
        f.update_action(None, bpf.OdomData(*ODATA))
        moved = _sets(f.local_sets())
        assert np.array_equal(moved, ref["moved"]) and set(f.rng_states()) == {ref["rng_moved"]}
        # a restored set is no longer the slice the engine recorded
        f.pfs[0].snapshot()
        f.pfs[0].restore()
        with pytest.raises(bpf.BpfError) as ei:
            f.slice(0)
        assert ei.value.code == 2
    finally:
        if f is not None:
            f.shutdown()
            f.close()
        for e in engines:
            e.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mailbox_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    from oracle import pyoracle as orc
    sc = _scenario(orc)
    e = bpf.Engine(0)
    lo, hi = (N * rank) // world, (N * (rank + 1)) // world
    m, scn, pf, data, od = _rank_objects(sc, e, lo, hi)
    b = HipShardBackend(e, scn, pf, torch.device("cuda", 0))
    sf = ShardedFilter(b, dist, exchange="mailbox", resample_form="in_place", max_share=float(world))
    assert sf.mailbox
    sf.update_sensor(data)
    sf.update_resample()
    st = sf.state()
    rec = dict(set=pf.getCurrentSet().samples.copy(), M=st.sample_count, leaf=st.leaf_count, bins=st.bin_count,
               rng=pf.getRngState(), conv=st.converged, miss=st.cdf_miss, counts=list(sf.counts), form=sf.form_used,
               windows=sf.windows_used, slice=b.slice())
    sf.update_action(od, bpf.OdomData(*ODATA))
    rec.update(moved=pf.getCurrentSet().samples.copy(), rng_moved=pf.getRngState())
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([rec], dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


def test_sharded_filter_over_the_mailbox_in_place(tmp_path, orc):
    import torch.multiprocessing as mp
    W = 2
    mp.spawn(_mailbox_worker, args=(W, _free_port(), str(tmp_path)), nprocs=W, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r), allow_pickle=True)[0] for r in range(W)]
    ref = _single_reference(_scenario(orc))
    got = np.concatenate([r["set"] for r in recs])
    assert got.shape == ref["want"].shape and np.array_equal(got[:, :3], ref["want"][:, :3])
    assert np.all(got[:, 3] == 1.0 / ref["M"])
    for k, r in enumerate(recs):
        assert r["form"] == "in_place" and r["windows"] == 0 and not r["miss"]
        assert (r["M"], r["leaf"], r["bins"], r["rng"], r["conv"]) == (ref["M"], ref["leaf"], ref["bins"], ref["rng"],
                                                                      ref["conv"])
        assert r["counts"] == [x["set"].shape[0] for x in recs]
        assert r["slice"] == (sum(r["counts"][:k]), r["counts"][k], ipr.IN_PLACE)
        assert r["rng_moved"] == ref["rng_moved"]
    assert np.array_equal(np.concatenate([r["moved"] for r in recs]), ref["moved"])
