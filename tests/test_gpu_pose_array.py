"""The particle-cloud message formed on the device (include/badger_pf.h, bpf_pf_get_pose_array and the sharded forms).
The reference value everywhere is the route a caller had before, on the same engine: bpf_pf_get_samples and the host loop
bpf_wire_samples_to_pose_array (the oracle's orc_wire_pose_array bit for bit, tests/test_wire.py).  x, y and the three
zeros are compared as bit patterns; the quaternion's sin / cos are the device's, compared with QUAT_BOUND.  Everything
sharded is compared with the single engine's call bit for bit in all seven columns: the same kernel on the same bits."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch  # before the engine library: torch brings a HIP runtime of its own, the first one loaded serves both

from scenario import Scenario

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu

MAX_N = 100000
# Twice the largest absolute difference of columns 5-6 from bpf_wire_samples_to_pose_array (host libm) measured over
# the edge headings below and 1 000 000 random headings in [-4 pi, 4 pi] (tools/time_pose_array.py,
# profiles/pose_array.json: max_abs_dev_vs_host_libm = 1.1102230246251565e-16, half a unit in the last place of 1.0).
# The values are bounded by 1, so this is a rounding budget with room for inputs the measurement did not see.
QUAT_BOUND = 2 * 1.1102230246251565e-16
EDGE_HEADINGS = [0.0, -0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 7.5, -9.0]


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def make_samples(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    s = np.zeros((n, 4))
    s[:, 0] = rng.uniform(-30, 30, n)
    s[:, 1] = rng.uniform(-30, 30, n)
    s[:, 2] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    k = min(n, len(EDGE_HEADINGS))
    s[:k, 2] = EDGE_HEADINGS[:k]
    s[:, 3] = 1.0 / n
    s[n // 2, 0] = -0.0
    if n > 2:
        assert (s[:, 0] < 0).any() and (s[:, 1] < 0).any()
    return s


def old_route(pf):
    from badger_amcl_amd import wire
    return wire.samples_to_pose_array(pf.getCurrentSet().samples)


def assert_poses(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(u64(got[:, :5]), u64(want[:, :5])), what
    if got.shape[0]:
        dev = np.abs(got[:, 5:] - want[:, 5:]).max()
        print("pose array %s: max |quaternion - host libm| = %.3e" % (what, dev))
        assert dev <= QUAT_BOUND, (what, dev)


@pytest.fixture(scope="module")
def engines():
    import badger_amcl_amd as bpf
    torch.cuda.set_device(0)  # torch's context first, as in the sharded workers; the engines run on its stream
    torch.zeros(1, device="cuda")
    pool = [bpf.Engine(0) for _ in range(10)]  # [0]: the single engine; [1 .. 8]: the ranks; [9]: never gets a filter
    yield pool
    for e in pool:
        e.close()


@pytest.fixture(scope="module")
def single(engines):
    import badger_amcl_amd as bpf
    return bpf.ParticleFilter(engines[0], 1, MAX_N, 0.0, 0.0, 85.0)


# ------------------------------------------------------------------------------------------ shapes and edge values
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_pose_array_equals_the_host_route(single, n):
    """Wave, block and LDS-tile edges; selections from the whole set to a single pose and to none."""
    s = make_samples(n)
    single.initWithSamples(s)
    want = old_route(single)
    assert np.array_equal(u64(want[:, :2]), u64(s[:, :2]))
    for first, stride in [(0, 1), (0, 3), (2, 7), (n - 1, 1), (n, 1), (0, n + 5)]:
        got = single.getPoseArray(first, stride)
        assert got.shape == (len(range(first, n, stride)), 7)
        assert_poses(got, want[first::stride], (n, first, stride))
        assert not np.signbit(got[:, 2:5]).any()  # +0.0


# ------------------------------------------------------------------------------------------ after a real cycle
def _read_all(pf):
    st = pf.getState()
    fields = tuple(getattr(st, f[0]) for f in st._fields_)
    w, pose = pf.getMaxWeightPose()
    return fields, pf.getCurrentSet().samples.copy(), pf.getRngState(), w, np.array(pose)


def test_query_after_a_cycle_leaves_the_filter_alone(orc):
    """updateSensor, updateResample, getPoseArray: state, set, rng and max-weight pose read the same before and after,
    and the next resample gives the set of an engine that never made the call."""
    import badger_amcl_amd as bpf
    sc_ = Scenario(orc, size=200, n=2000, beams=61)
    es = [bpf.Engine(0), bpf.Engine(0)]
    try:
        sets = []
        for k, e in enumerate(es):
            m, sc, pf, data = sc_.gpu_objects(e, 61, "lf", min_samples=100, seed=42)
            assert sc.updateSensor(pf, data)
            pf.updateResample()
            before = _read_all(pf)  # (on both engines: the getters evaluate the statistics)
            if k == 0:
                got = pf.getPoseArray()
                assert_poses(got, old_route(pf), "after a cycle")
                assert got.shape[0] == pf.getState().sample_count
            after = _read_all(pf)
            assert before[0] == after[0] and before[2] == after[2] and before[3] == after[3]
            assert np.array_equal(before[1], after[1]) and np.array_equal(before[4], after[4])
            assert sc.updateSensor(pf, data)
            if k == 0:
                pf.getPoseArray(1, 3)  # between the sensor update and the resample: the CDF hand-over stays
            pf.updateResample()
            sets.append((pf.getCurrentSet().samples.copy(), pf.getRngState(), pf.getState().leaf_count))
        assert np.array_equal(sets[0][0], sets[1][0]) and sets[0][1:] == sets[1][1:]
    finally:
        for e in es:
            e.close()


# ------------------------------------------------------------------------------------------ registered / pageable
@pytest.mark.parametrize("n", [4097, 80000])
def test_registered_and_pageable_output_give_the_same_bits(engines, single, n):
    """80 000 poses are 4.5 MB: a pageable destination takes three pieces of the bounce buffer."""
    e = engines[0]
    single.initWithSamples(make_samples(n, seed=1))
    reg = np.full((n + 3, 7), 7.25)
    page = np.full((n + 3, 7), 7.25)
    e.registerHostBuffer(reg)
    try:
        assert e.isHostBufferRegistered(reg) and not e.isHostBufferRegistered(page)
        a = single.getPoseArray(out=reg)
        b = single.getPoseArray(out=page)
        assert a.shape == b.shape == (n, 7) and np.array_equal(u64(a), u64(b))
        assert np.all(reg[n:] == 7.25) and np.all(page[n:] == 7.25)
        assert_poses(a, old_route(single), ("registered", n))
    finally:
        e.unregisterHostBuffer(reg)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(engines, single):
    e, lib = engines[0], engines[0].lib
    n = 257
    single.initWithSamples(make_samples(n))
    dp = C.POINTER(C.c_double)
    sentinel = np.full((n, 7), -123.456)
    out = sentinel.copy()
    cnt = C.c_int(-1)
    for first, stride in [(0, 1), (2, 7)]:
        count = len(range(first, n, stride))
        assert lib.bpf_pf_get_pose_array(e.h, first, stride, out.ctypes.data_as(dp), count - 1, C.byref(cnt)) == 8
        assert np.array_equal(u64(out), u64(sentinel))
    assert lib.bpf_pf_get_pose_array(e.h, 0, 0, out.ctypes.data_as(dp), n, C.byref(cnt)) == 1
    assert lib.bpf_pf_get_pose_array(e.h, -1, 1, out.ctypes.data_as(dp), n, C.byref(cnt)) == 1
    assert lib.bpf_pf_get_pose_array(e.h, 0, 1, None, n, C.byref(cnt)) == 1
    assert np.array_equal(u64(out), u64(sentinel))
    # an empty selection is no error, whatever the capacity
    assert lib.bpf_pf_get_pose_array(e.h, n, 1, out.ctypes.data_as(dp), 0, C.byref(cnt)) == 0 and cnt.value == 0
    # the stage forms
    p, k = C.c_void_p(), C.c_int()
    assert lib.bpf_shard_pose_rows_dev(e.h, 0, 0, 0, C.byref(p), C.byref(k)) == 1
    assert lib.bpf_shard_pose_rows_dev(e.h, 0, -1, 1, C.byref(p), C.byref(k)) == 1
    assert lib.bpf_shard_pose_rows_dev(e.h, 0, 0, 1, C.byref(p), C.byref(k)) == 0 and k.value == n
    assert lib.bpf_pose_array_from_rows_dev(e.h, p, n, n, out.ctypes.data_as(dp), n - 1) == 8
    assert np.array_equal(u64(out), u64(sentinel))
    # no filter: BPF_ERR_NOT_CONFIGURED; no exchange: the one-call form says so as well
    bare = engines[9]
    assert bare.lib.bpf_pf_get_pose_array(bare.h, 0, 1, out.ctypes.data_as(dp), n, C.byref(cnt)) == 2
    assert bare.lib.bpf_shard_pose_rows_dev(bare.h, 0, 0, 1, C.byref(p), C.byref(k)) == 2
    assert bare.lib.bpf_shard_get_pose_array(bare.h, 0, 0, 1, out.ctypes.data_as(dp), n, C.byref(cnt)) == 2
    assert lib.bpf_shard_get_pose_array(e.h, 0, 0, 1, out.ctypes.data_as(dp), n, C.byref(cnt)) == 2
    assert lib.bpf_shard_get_pose_array(e.h, 0, 0, 0, out.ctypes.data_as(dp), n, C.byref(cnt)) == 1
    assert np.array_equal(u64(out), u64(sentinel))


# ------------------------------------------------------------------------------------------ stage forms
def make_ranks(engines, samples, cuts):
    """One backend per slice [cuts[r], cuts[r + 1]) on device 0; an empty slice is an engine that adopted 0 samples."""
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend
    n = samples.shape[0]
    out = []
    for r in range(len(cuts) - 1):
        e = engines[1 + r]
        lo, hi = cuts[r], cuts[r + 1]
        pf = bpf.ParticleFilter(e, 100, MAX_N, 0.0, 0.0, 85.0)
        if hi > lo:
            pf.initWithSamples(np.ascontiguousarray(samples[lo:hi]))
        else:
            e.check(e.lib.bpf_shard_adopt_dev(e.h, None, None, None, 0, n, 0, 0))
        assert pf.getState().sample_count == hi - lo
        out.append(HipShardBackend(e, None, pf, torch.device("cuda", 0)))
    return out


STAGE_CUTS = [[int(v) for v in np.linspace(0, n, W + 1)] for W, n in [(1, 1000), (2, 1000), (3, 1000), (8, 1001)]] + \
             [[0, 0, 1, 1000], [0, 500, 500, 1000]]


@pytest.mark.parametrize("cuts", STAGE_CUTS, ids=lambda c: "-".join(str(v) for v in c))
def test_stage_forms_equal_the_single_engine_bit_for_bit(engines, single, cuts):
    """W engines in one process, the rows concatenated on the device by torch: the array formed from the gathered rows
    (by a rank's engine and by an engine that never had a filter) is the single engine's on the concatenated set."""
    from badger_amcl_amd.sharded import pose_selection
    n = cuts[-1]
    s = make_samples(n, seed=len(cuts))
    single.initWithSamples(s)
    bs = make_ranks(engines, s, cuts)
    counts = [b - a for a, b in zip(cuts, cuts[1:])]
    bare = engines[9]
    for stride in (1, 7):
        for first in (0, 3):
            want = single.getPoseArray(first, stride).copy()
            parts = [b.pose_rows(cuts[r], first, stride) for r, b in enumerate(bs)]
            assert [int(p.shape[1]) for p in parts] == [k for _, k in pose_selection(counts, first, stride)]
            rows = torch.cat(parts, dim=1).contiguous()  # the exchange: all-gather of the rows
            assert rows.shape == (3, want.shape[0])
            got = bs[-1].pose_array_from_rows(rows, rows.shape[1])
            assert np.array_equal(u64(got), u64(want)), (cuts, first, stride)
            # gathered rows with a row stride of their own, formed by an engine without a filter
            wide = torch.zeros((3, rows.shape[1] + 5), dtype=torch.int64, device=rows.device)
            wide[:, :rows.shape[1]] = rows
            torch.cuda.synchronize()
            out = np.zeros((rows.shape[1], 7))
            bare.check(bare.lib.bpf_pose_array_from_rows_dev(bare.h, C.c_void_p(wide.data_ptr()), wide.stride(0),
                                                             rows.shape[1], out.ctypes.data_as(C.POINTER(C.c_double)),
                                                             out.shape[0]))
            assert np.array_equal(u64(out), u64(want)), (cuts, first, stride)


# ------------------------------------------------------------------------------------------ across processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


N_PROC = 2000
ROT = ((0.8, -0.6, 0.0), (0.6, 0.8, 0.0), (0.0, 0.0, 1.0))
SIGMA = (0.15, 0.1, 0.05)
ODOM = (2, 0.05, 0.04, 0.03, 0.02, 0.0)                         # diff-corrected
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))  # pose, delta, absolute motion
QUERIES = [(0, 0, 1), (-1, 3, 7)]  # (root, first, stride) at every state


def _scenario():
    from oracle import pyoracle as orc
    return orc, Scenario(orc, size=200, n=256, beams=61)


def _worker(rank, world, port, out_dir, exchange):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import badger_amcl_amd as bpf
    from badger_amcl_amd.sharded import HipShardBackend, ShardedFilter
    orc, sc = _scenario()
    e = bpf.Engine(0)
    m, scn, _, data = sc.gpu_objects(e, 61, "lf")
    pf = bpf.ParticleFilter(e, 100, N_PROC, 0.0, 0.0, 85.0)
    pf.srand48(21)
    b = HipShardBackend(e, scn, pf, torch.device("cuda", 0))
    sf = ShardedFilter(b, dist, first_window=1024, exchange=exchange, init_follows=True)
    assert sf.mailbox == (exchange == "mailbox")
    exchanges = [0]
    for name in ("_all_gather", "_all_reduce_sum"):
        def wrap(fn=getattr(sf, name)):
            def f(*a, **k):
                exchanges[0] += 1
                return fn(*a, **k)
            return f
        setattr(sf, name, wrap())

    def engine_exchanges():
        if not sf.mailbox:
            return 0
        x = C.c_longlong()
        e.check(e.lib.bpf_shard_exchange_count(e.h, C.byref(x)))
        return x.value

    def counted(fn):
        a, c = exchanges[0], engine_exchanges()
        res = fn()
        return res, exchanges[0] - a, engine_exchanges() - c

    recs = {}

    def query(tag):
        for q, (root, first, stride) in enumerate(QUERIES):
            got, by_dist, by_engine = counted(lambda: sf.get_pose_array(root=root, first=first, stride=stride))
            assert (got is not None) == (root < 0 or root == rank)
            # mailbox: the one-call form, two exchanges of the engine's own; collective: one ragged gather
            assert (by_dist, by_engine) == ((0, 2) if sf.mailbox else (1, 0)), (tag, by_dist, by_engine)
            recs["%s.q%d" % (tag, q)] = np.zeros((0, 0)) if got is None else got

    sf.init_with_gaussian(sc.pose, ROT, SIGMA)
    query("init")
    od = bpf.Odom(e)
    od.setModel(*ODOM)
    cost = []
    for cycle in range(2):
        sf.update_action(od, bpf.OdomData(*ODATA))
        sf.update_sensor(data)
        if cycle == 0:
            query("sensor")
        # the statistics evaluated afresh: as many exchanges behind a pose-array query as without one ...
        first_pose, by_dist, by_engine = counted(sf.get_max_weight_pose)
        assert by_dist > 0
        cost.append((by_dist, by_engine))
        # ... and once in force they stay in force across a query
        query("sensor%d.valid" % cycle)
        again, by_dist, by_engine = counted(sf.get_max_weight_pose)
        assert (by_dist, by_engine) == (0, 0)
        assert again[0] == first_pose[0] and np.array_equal(again[1], first_pose[1])
        sf.update_resample()
        if cycle == 0:
            query("resample")
    assert cost[0] == cost[1], cost
    recs["M"] = np.array([sf.sample_count])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **recs)
    dist.barrier()
    dist.destroy_process_group()
    e.close()


@pytest.mark.parametrize("exchange", ["mailbox", "collective"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_filter_pose_array(tmp_path, world, exchange):
    """ShardedFilter.get_pose_array in 2 and 3 processes on the one GPU, over the mailbox (the engine's one-call form)
    and over gloo: after an init, a sensor update and a resample the root's array -- and every rank's with root = -1 --
    is the unsharded engine's, bit for bit."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), exchange), nprocs=world, join=True)
    recs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    import badger_amcl_amd as bpf
    orc, sc = _scenario()
    e = bpf.Engine(0)
    try:
        m, scn, _, data = sc.gpu_objects(e, 61, "lf")
        pf = bpf.ParticleFilter(e, 100, N_PROC, 0.0, 0.0, 85.0)
        pf.srand48(21)
        od = bpf.Odom(e)
        od.setModel(*ODOM)

        def check(tag):
            for q, (root, first, stride) in enumerate(QUERIES):
                want = pf.getPoseArray(first, stride)
                assert want.shape[0] == len(range(first, pf.getState().sample_count, stride)) > 0
                for r in range(world):
                    got = recs[r]["%s.q%d" % (tag, q)]
                    if root < 0 or root == r:
                        assert got.shape == want.shape and np.array_equal(u64(got), u64(want)), (tag, q, r)
                    else:
                        assert got.shape == (0, 0)

        pf.initWithGaussian(sc.pose, ROT, SIGMA)
        check("init")
        for cycle in range(2):
            od.updateAction(pf, bpf.OdomData(*ODATA))
            scn.updateSensor(pf, data)
            if cycle == 0:
                check("sensor")
            check("sensor%d.valid" % cycle)
            pf.updateResample()
            if cycle == 0:
                check("resample")
        assert all(int(r["M"][0]) == pf.getState().sample_count for r in recs)
    finally:
        e.close()
