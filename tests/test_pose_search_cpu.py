"""The exhaustive pose search's host pieces (no GPU): the window constant, the merge of hit lists against a numpy
stable sort, the layout of bpf_pose_hit, and the numpy model of the candidate enumeration (pose_search_ref.py, which
tests/test_gpu_pose_search.py holds the device to) against pose_check_ref.FreeSpace.planar."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_check_ref as ref  # noqa: E402
import pose_search_ref as psr  # noqa: E402


def _hits(scores, cands):
    import badger_amcl_amd.pf as hpf
    h = np.zeros(len(scores), dtype=hpf.POSE_HIT_DTYPE)
    h["score"] = scores
    h["candidate"] = cands
    h["pose"] = np.asarray(cands, dtype=np.float64)[:, None] * [1.0, 2.0, 3.0]
    h["i"] = np.asarray(cands) % 7
    h["j"] = np.asarray(cands) % 11
    h["heading"] = np.asarray(cands) % 5
    return h


def test_window_is_positive():
    import badger_amcl_amd.pf as hpf
    assert hpf.pose_search_window() > 0


def test_struct_layout():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    assert C.sizeof(_lib.PoseHit) == 56
    assert hpf.POSE_HIT_DTYPE.itemsize == 56
    for name, off in (("pose", 0), ("score", 24), ("candidate", 32), ("i", 40), ("j", 44), ("heading", 48),
                      ("reserved", 52)):
        assert getattr(_lib.PoseHit, name).offset == off
        assert hpf.POSE_HIT_DTYPE.fields[name][1] == off


@pytest.mark.parametrize("k", [1, 5, 64, 1024])
def test_merge_is_the_stable_sort(k):
    """lists of disjoint candidate ranges, each in the search's order, with many equal scores (ties go by candidate),
    a NaN and both zeros"""
    import badger_amcl_amd.pf as hpf
    rng = np.random.default_rng(7)
    n = 700
    scores = rng.integers(0, 12, n).astype(np.float64) / 4.0  # few distinct values: ties within and across lists
    scores[[3, 250, 699]] = np.nan
    scores[[10, 300]] = -0.0
    scores[[11, 301]] = 0.0
    cands = 5 + np.arange(n, dtype=np.int64)
    cuts = [0, 130, 131, 400, n]
    lists = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = psr.order(scores[a:b], cands[a:b])
        lists.append(_hits(scores[a:b][o], cands[a:b][o]))
    got = hpf.merge_pose_hits(lists, k)
    o = psr.order(scores, cands)[:k]
    want = _hits(scores[o], cands[o])
    assert got.shape[0] == min(k, n)
    assert np.array_equal(got["candidate"], want["candidate"])
    assert got.tobytes() == want.tobytes()  # whole rows, NaN and the sign of zero included
    # the lists in another order, and unsorted inside: the same result
    shuffled = [lst[rng.permutation(lst.shape[0])] for lst in lists[::-1]]
    assert hpf.merge_pose_hits(shuffled, k).tobytes() == want.tobytes()


def test_merge_edge_cases():
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    assert hpf.merge_pose_hits([], 4).shape[0] == 0
    empty = np.zeros(0, dtype=hpf.POSE_HIT_DTYPE)
    assert hpf.merge_pose_hits([empty, empty], 4).shape[0] == 0
    a = _hits([3.0, 1.0], [4, 2])
    got = hpf.merge_pose_hits([empty, a, empty], 1024)  # k larger than the total
    assert got.tobytes() == a.tobytes()
    for k in (0, -1, 1025):
        with pytest.raises(bpf.BpfError) as ei:
            hpf.merge_pose_hits([a], k)
        assert ei.value.code == 1


def test_order_model():
    s = np.array([1.0, np.nan, 2.0, 2.0, -0.0, 0.0, np.inf])
    c = np.array([9, 8, 7, 3, 2, 1, 0])
    assert list(c[psr.order(s, c)]) == [0, 3, 7, 9, 1, 2, 8]
    assert list(psr.top_k(np.array([1.0, 3.0, 3.0, 0.5]), 100, 3)) == [101, 102, 100]


@pytest.mark.parametrize("name", ["G2", "G3"])
@pytest.mark.parametrize("headings,stride", [(1, 1), (5, 3), (8, 2)])
def test_enumeration_model_agrees_with_the_free_space_restatement(orc, name, headings, stride):
    """cell poses of the model = convertMapToWorld as pose_check_ref.FreeSpace.planar forms it (scalar Python), over
    the strided free list, cell-major with the heading inner; theta as the scalar expression"""
    from map_geometry import GeoScenario
    geo = GeoScenario.named(orc, name)
    cells = geo.free_cells()
    assert cells == ref.free_cells_2d(geo.cells, geo.lut, geo.map_factors[2])
    fs = ref.FreeSpace.planar(cells, geo.size_x, geo.size_y, geo.origin, geo.res)
    sp = psr.Space.of(geo, headings, stride)
    kept = [(i, j) for i, j in cells if i % stride == 0 and j % stride == 0]
    assert sp.total == len(kept) * headings and sp.total > 0
    i, j, h, poses = sp.rows(np.arange(sp.total))
    want = []
    for (ci, cj) in kept:
        x, y = fs.to_world(ci, cj)
        for hh in range(headings):
            want.append((ci, cj, hh, x, y, (2.0 * np.pi * hh) / headings - np.pi))
    want = np.array(want)
    assert np.array_equal(i, want[:, 0]) and np.array_equal(j, want[:, 1]) and np.array_equal(h, want[:, 2])
    assert poses.tobytes() == np.ascontiguousarray(want[:, 3:]).tobytes()
    s = sp.samples(3, 10)
    assert np.array_equal(s[:, :3], poses[3:13]) and np.all(s[:, 3] == 1.0)


def test_pose_search_smoke_compiles_against_the_c_abi(tmp_path):
    """the adapter's searchPoses / searchSpace / mergePoseHits are valid C++17 and link against the library"""
    from badger_amcl_amd import build
    import cpp_driver
    build.build()
    cpp_driver.compile_driver(tmp_path, "pose_search_smoke")
    assert subprocess.run([str(tmp_path / "pose_search_smoke")], capture_output=True).returncode == 2  # usage
