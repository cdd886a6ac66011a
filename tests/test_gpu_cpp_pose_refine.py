"""Pose refinement through the C++ adapter's PlanarScanner / PointCloudScanner (tests/cpp/pose_refine_smoke.cpp)
against the Python binding, which passes the C call's rows on as they are: rows and trace byte for byte, from packed
poses and through the overload that takes a search's hits."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

LATTICE = (1, 1, 3)  # R, A, L


def _run(exe, tmp_path, head, poses, xy_step, theta_step, rows, trace):
    R, A, L = LATTICE
    out = {name: str(tmp_path / (name + ".bin")) for name in ("rows", "trace", "hits_rows")}
    res = subprocess.run([str(exe)] + head + [poses, str(R), repr(xy_step), str(A), repr(theta_step), str(L),
                                              out["rows"], out["trace"], out["hits_rows"]],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert [int(v) for v in res.stdout.split()] == [rows.shape[0], rows.shape[0] * L]
    assert open(out["rows"], "rb").read() == rows.tobytes()
    assert open(out["trace"], "rb").read() == np.ascontiguousarray(trace, dtype=np.int32).tobytes()
    assert open(out["hits_rows"], "rb").read() == rows.tobytes()
    assert (rows["moved"] > 0).any()


def test_planar_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    import pose_refine_ref as prr
    from test_gpu_pose_search import MAX_BEAMS, scanner_on
    geo, poses, xy_step, theta_step = prr.planar_case(orc, "lf", LATTICE)
    R, A, L = LATTICE
    e = bpf.Engine(0)
    try:
        m, sc = scanner_on(e, geo, "lf")
        rows, trace = sc.refinePoses(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), poses, R, xy_step, A,
                                     theta_step, L, trace=True)
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_refine_smoke")
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(cells=geo.cells.astype(np.int32),
                                                                lut=np.asarray(geo.lut, dtype=np.float32),
                                                                ranges=geo.ranges, angles=geo.angles, poses=poses))
    head = ["planar", paths["cells"], paths["lut"], paths["ranges"], paths["angles"], str(geo.size_x), str(geo.size_y),
            repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])), str(MAX_BEAMS)]
    _run(exe, tmp_path, head, paths["poses"], xy_step, theta_step, rows, trace)


def test_cloud_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    from test_gpu_pose_refine import _room_poses
    from test_gpu_pose_search_cloud import RES, room, scanner_on
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    poses = _room_poses()
    R, A, L = LATTICE
    xy_step, theta_step = 2 * RES, 0.4
    e = bpf.Engine(0)
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        rows, trace = sc.refinePoses(bpf.PointCloudData(pts), poses, R, xy_step, A, theta_step, L, trace=True)
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_refine_smoke")
    cells6 = np.concatenate([np.asarray(lut.min_cells), np.asarray(lut.max_cells)]).astype(np.int32)
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(
        pose_indices=np.asarray(lut.pose_indices, dtype=np.uint32),
        ratios=np.asarray(lut.distance_ratios, dtype=np.uint8), cells6=cells6, points=np.array(pts), poses=poses,
        tf7=np.array(list(tf_xyz) + list(tf_quat), dtype=np.float64)))
    head = ["cloud", paths["pose_indices"], paths["ratios"], paths["cells6"], paths["points"], paths["tf7"], repr(RES),
            repr(float(max_dist)), "128"]
    _run(exe, tmp_path, head, paths["poses"], xy_step, theta_step, rows, trace)
