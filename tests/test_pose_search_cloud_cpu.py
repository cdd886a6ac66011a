"""The cloud pose search's host pieces (no GPU): the numpy model of the candidate enumeration
(pose_search_cloud_ref.py, which tests/test_gpu_pose_search_cloud.py holds the device to) against scalar Python over
pose_check_ref.free_cells_3d / FreeSpace.octo, the binding's prototypes, and the C++ smoke program against the
adapter's OctoMap / PointCloudScanner."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_check_ref as ref  # noqa: E402
import pose_search_cloud_ref as pscr  # noqa: E402

# the room of tests/test_gpu_cloud.py (negative minima, extents 86 x 66), bounds that straddle zero on one axis only,
# and all-positive bounds that start off a multiple of every stride used
BOUNDS = [((-43, -33, -3), (43, 33, 50)), ((-7, 2, 0), (5, 9, 4)), ((3, 5, 0), (14, 12, 2))]


def _scalar_rows(mn, mx, res, headings, stride):
    fs = ref.FreeSpace.octo(mn, mx, res)
    assert fs.cells == ref.free_cells_3d(mn, mx)
    want = []
    for (ci, cj) in fs.cells:
        if ci % stride == 0 and cj % stride == 0:  # Python's %: divisible, also for negative cells
            x, y = fs.to_world(ci, cj)
            for hh in range(headings):
                want.append((ci, cj, hh, x, y, (2.0 * np.pi * hh) / headings - np.pi))
    return np.array(want, dtype=np.float64).reshape(-1, 6)


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("headings,stride", [(1, 1), (5, 3), (8, 2)])
def test_enumeration_model_agrees_with_the_free_space_restatement(bounds, headings, stride):
    mn, mx = bounds
    res = 0.05
    sp = pscr.Space(mn, mx, res, headings, stride)
    want = _scalar_rows(mn, mx, res, headings, stride)
    assert sp.total == want.shape[0] and sp.total > 0 and sp.columns * headings == sp.total
    if stride == 3:
        assert (mx[0] - mn[0]) % stride != 0 or (mx[1] - mn[1]) % stride != 0  # a stride that does not divide the extent
    i, j, h, poses = sp.rows(np.arange(sp.total))
    assert np.array_equal(i, want[:, 0]) and np.array_equal(j, want[:, 1]) and np.array_equal(h, want[:, 2])
    assert poses.tobytes() == np.ascontiguousarray(want[:, 3:]).tobytes()
    s = sp.samples(3, 10)
    assert np.array_equal(s[:, :3], poses[3:13]) and np.all(s[:, 3] == 1.0)


@pytest.mark.parametrize("bounds,stride,columns", [
    (((-43, -33, 0), (43, 33, 1)), 100, 1),   # larger than either extent: the column (0, 0) alone
    (((-7, 2, 0), (5, 9, 1)), 12, 0),         # ... and no multiple of it inside the j bounds
    (((3, 5, 0), (14, 12, 1)), 15, 0),
    (((3, 5, 0), (14, 12, 1)), 11, 1),        # (11, 11)
    (((-5, -5, 0), (-5, 4, 1)), 1, 0),        # empty bounds in i
])
def test_strides_larger_than_the_extent(bounds, stride, columns):
    mn, mx = bounds
    sp = pscr.Space(mn, mx, 0.1, 4, stride)
    want = _scalar_rows(mn, mx, 0.1, 4, stride)
    assert sp.columns == columns and sp.total == want.shape[0] == 4 * columns
    if columns:
        i, j, h, poses = sp.rows(np.arange(sp.total))
        assert np.array_equal(i, want[:, 0]) and np.array_equal(j, want[:, 1])
        assert poses.tobytes() == np.ascontiguousarray(want[:, 3:]).tobytes()


def test_first_multiple():
    for s in (1, 2, 3, 7):
        for a in range(-15, 16):
            m = pscr.first_multiple_at_or_above(a, s)
            assert m % s == 0 and a <= m < a + s


def test_binding_has_the_two_calls_and_the_methods():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    assert "bpf_cloud_search_poses" in _lib.SIGNATURES and "bpf_cloud_search_space" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "bpf_cloud_search_poses") and hasattr(lib, "bpf_cloud_search_space")
    assert callable(hpf.PointCloudScanner.searchPoses) and callable(hpf.PointCloudScanner.searchSpace)


def test_pose_search_cloud_smoke_compiles_against_the_c_abi(tmp_path):
    """the adapter's OctoMap / PointCloudData / PointCloudScanner are valid C++17 and link against the library"""
    from badger_amcl_amd import build
    import cpp_driver
    build.build()
    cpp_driver.compile_driver(tmp_path, "pose_search_cloud_smoke")
    assert subprocess.run([str(tmp_path / "pose_search_cloud_smoke")], capture_output=True).returncode == 2  # usage
