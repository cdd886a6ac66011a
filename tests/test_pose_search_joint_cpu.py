"""The joint pose search's host pieces (no GPU): the heading table of the library against the numpy model
(pose_search_joint_ref.py, which the GPU tests hold the device to), the model's composition at S = 1 and a zero
offset against the base poses of both single-scan models, the binding, and the C++ program against the adapter."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_cloud_ref as pscr  # noqa: E402
import pose_search_joint_ref as psj  # noqa: E402
import pose_search_ref as psr  # noqa: E402


@pytest.mark.parametrize("headings", [1, 5, 8, 23, 211, 65536])
def test_heading_table_is_the_models_bit_for_bit(headings):
    import badger_amcl_amd.pf as hpf
    c, s = hpf.pose_search_heading_table(headings)
    mc, ms = psj.heading_table(headings)
    assert c.shape == (headings,) and s.shape == (headings,)
    assert c.tobytes() == mc.tobytes()
    assert s.tobytes() == ms.tobytes()
    assert abs(float(c[0]) + 1.0) < 1e-15 and abs(float(s[0])) < 1e-15  # theta_0 = -pi


@pytest.mark.parametrize("headings", [0, -1, 65537, 1 << 20])
def test_heading_table_refuses(headings):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    with pytest.raises(bpf.BpfError) as ei:
        hpf.pose_search_heading_table(headings)
    assert ei.value.code == (1 if headings < 1 else 8)


@pytest.mark.parametrize("name", ["G2", "G3"])
@pytest.mark.parametrize("headings,stride", [(1, 1), (5, 3), (8, 2)])
def test_one_scan_at_zero_offset_is_the_planar_base_pose(orc, name, headings, stride):
    from map_geometry import GeoScenario
    sp = psr.Space.of(GeoScenario.named(orc, name), headings, stride)
    cands = np.arange(sp.total)
    poses = psj.compose(sp, cands, [(0.0, 0.0, 0.0)])
    assert poses.shape == (sp.total, 1, 3) and sp.total > 0
    assert np.array_equal(poses[:, 0], sp.rows(cands)[3])  # (==: x + 0 may turn -0.0 into +0.0)


@pytest.mark.parametrize("bounds", [((-43, -33, -3), (43, 33, 50)), ((-7, 2, 0), (5, 9, 4)), ((3, 5, 0), (14, 12, 2))])
@pytest.mark.parametrize("headings,stride", [(1, 1), (5, 3), (8, 2)])
def test_one_scan_at_zero_offset_is_the_cloud_base_pose(bounds, headings, stride):
    sp = pscr.Space(bounds[0], bounds[1], 0.05, headings, stride)
    cands = np.arange(sp.total)
    poses = psj.compose(sp, cands, [(0.0, 0.0, 0.0)])
    assert poses.shape == (sp.total, 1, 3) and sp.total > 0
    assert np.array_equal(poses[:, 0], sp.rows(cands)[3])


def test_composition_is_coord_add():
    """against scalar Python for every candidate of a small space: pose (+) D with the heading's own cos / sin"""
    sp = pscr.Space((-7, 2, 0), (5, 9, 4), 0.05, 5, 1)
    offsets = [(0.0, 0.0, 0.0), (0.35, -0.15, 0.4), (0.37, -1.9, 7.5)]
    cands = np.arange(sp.total)
    poses = psj.compose(sp, cands, offsets)
    base = sp.rows(cands)[3]
    for c in cands:
        for s, d in enumerate(offsets):
            assert poses[c, s].tobytes() == psj.pose_add(base[c], d).tobytes()
    assert np.all(poses[:, 2, 2] > np.pi)  # theta is not normalised


def test_sequential_scores_carry_the_weight():
    poses = np.zeros((4, 3, 3))
    factors = np.array([[0.5, 0.25, 3.0], [1.0, 1.0, 1.0], [0.1, 0.1, 0.1], [2.0, 0.0, 5.0]])
    seen = []

    def apply_scan(s, samples):
        seen.append(samples[:, 3].copy())
        samples[:, 3] *= factors[:, s]

    w = psj.sequential_scores(poses, apply_scan)
    assert np.all(seen[0] == 1.0) and np.array_equal(seen[1], factors[:, 0])
    assert np.array_equal(w, (factors[:, 0] * factors[:, 1]) * factors[:, 2])


def test_binding_has_the_calls_and_the_methods():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    lib = _lib.load()
    for name in ("bpf_pose_search_heading_table", "bpf_planar_search_poses_joint", "bpf_cloud_search_poses_joint",
                 "bpf_planar_search_joint_poses", "bpf_cloud_search_joint_poses"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for cls in (hpf.PlanarScanner, hpf.PointCloudScanner):
        assert callable(cls.searchPosesJoint) and callable(cls.searchJointPoses)


def test_pose_search_joint_program_compiles_against_the_c_abi(tmp_path):
    """the adapter's two searchPosesJoint are valid C++17 and link against the library"""
    from badger_amcl_amd import build
    import cpp_driver
    build.build()
    cpp_driver.compile_driver(tmp_path, "pose_search_joint")
    assert subprocess.run([str(tmp_path / "pose_search_joint")], capture_output=True).returncode == 2  # usage
