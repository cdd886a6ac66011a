"""The particle-cloud message of a sharded filter without a GPU: which samples of every slice a (first, stride)
selection of the global index space picks (sharded.pose_selection), and ShardedFilter.get_pose_array over gloo with a
numpy backend -- the exchange logic (ragged gather, global order, root / every rank) is the product's, the forming is
wire.samples_to_pose_array."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from shard_backends import OracleShardBackend  # noqa: E402


# ---------------------------------------------------------------------------------------------- pose_selection
@pytest.mark.parametrize("stride", [1, 2, 3, 11])
@pytest.mark.parametrize("first", [0, 1, 6, 50])
@pytest.mark.parametrize("counts", [(5,), (3, 4), (0, 7, 0, 2), (1,) * 8])
def test_pose_selection_equals_enumeration(counts, first, stride):
    from badger_amcl_amd.sharded import pose_selection
    got = pose_selection(counts, first, stride)
    assert len(got) == len(counts)
    at = 0
    for r, n in enumerate(counts):
        picked = [i for i in range(n) if at + i >= first and (at + i - first) % stride == 0]
        i0, n_sel = got[r]
        assert n_sel == len(picked), (r, got[r], picked)
        if picked:
            assert i0 == picked[0] and picked == list(range(i0, n, stride))
        at += n
    total = sum(counts)
    assert sum(n for _, n in got) == len(range(first, total, stride))


def test_pose_selection_refuses_bad_arguments():
    from badger_amcl_amd.sharded import pose_selection
    with pytest.raises(ValueError):
        pose_selection((3, 4), 0, 0)
    with pytest.raises(ValueError):
        pose_selection((3, 4), -1, 1)


# ---------------------------------------------------------------------------------------------- over gloo
class PoseBackend(OracleShardBackend):
    """OracleShardBackend with the two pose-array stages in numpy."""

    def pose_rows(self, global_first, first, stride):
        g = global_first + np.arange(self.samples.shape[0])
        keep = (g >= first) & ((g - first) % stride == 0)
        return torch.from_numpy(np.ascontiguousarray(self.samples[keep, :3].T).view(np.int64).copy())

    def pose_array_from_rows(self, rows, n):
        from badger_amcl_amd import wire
        s = np.zeros((n, 4))
        s[:, :3] = rows.numpy().view(np.float64)[:, :n].T
        return wire.samples_to_pose_array(s)


def all_samples(n=1200):
    rng = np.random.default_rng(31)
    s = np.zeros((n, 4))
    s[:, 0] = rng.uniform(-20, 20, n)
    s[:, 1] = rng.uniform(-20, 20, n)
    s[:, 2] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    s[:, 3] = 1.0 / n
    s[5, 0] = -0.0
    s[6, 2] = -0.0
    return s


def queries(n, world):
    return [(0, 0, 1), (world - 1, 3, 7), (-1, 0, 1), (-1, 2, 5), (0, n, 1), (-1, 0, n + 5), (0, n - 1, 1)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, split):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from badger_amcl_amd.sharded import ShardedFilter
    from oracle import pyoracle as orc
    s = all_samples()
    n = s.shape[0]
    b = PoseBackend(orc, None, None, s[split[rank]:split[rank + 1]], 100, n, seed=9)
    sf = ShardedFilter(b, dist, first_window=256)
    out = {}
    for q, (root, first, stride) in enumerate(queries(n, world)):
        got = sf.get_pose_array(root=root, first=first, stride=stride)
        out["q%d" % q] = np.zeros((0, 0)) if got is None else got  # (a [0, 0] array stands for None)
    with pytest.raises(ValueError):
        sf.get_pose_array(root=world)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("split", [(0, 137, 1200), (0, 100, 650, 1200), (0, 400, 400, 1200)])
def test_sharded_filter_pose_array_over_gloo(tmp_path, split):
    """World size 2 and 3 (one split with an empty shard): the root's array is wire.samples_to_pose_array of the
    selected global samples bit for bit, the other ranks get None, root = -1 gives it to every rank."""
    from badger_amcl_amd import wire
    world = len(split) - 1
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), split), nprocs=world, join=True)
    s = all_samples()
    n = s.shape[0]
    got = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for q, (root, first, stride) in enumerate(queries(n, world)):
        want = wire.samples_to_pose_array(s[first::stride])
        assert want.shape == (len(range(first, n, stride)), 7)
        for r in range(world):
            a = got[r]["q%d" % q]
            if root < 0 or root == r:
                assert a.shape == want.shape, (q, r, a.shape)
                assert np.array_equal(a.view(np.uint64), want.view(np.uint64)), (q, r)
            else:
                assert a.shape == (0, 0), (q, r)
