"""Pose moments through the C++ adapter's PlanarScanner / PointCloudScanner and PoseMixture::mixtureApplyMoments
(tests/cpp/pose_moments_smoke.cpp) against the Python binding, which passes the C calls' rows on as they are: rows,
scores and components byte for byte, from packed poses and through the overloads that take hits and refined rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

LATTICE = (2, 2)  # R, A
BASELINE = 0.5
# the mixture both sides build (tests/cpp/pose_moments_smoke.cpp has the same numbers)
TOTAL, CAP = 1000, 8
SIGMA, FLOOR, CEIL = (0.05, 0.05, 0.03), (0.01, 0.01, 0.005), (0.1, 0.1, 0.06)


def _components(poses, rows, xy_step, theta_step):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    refined = np.zeros(poses.shape[0], dtype=hpf.POSE_REFINED_DTYPE)
    refined["pose"] = poses
    refined["score"] = rows["score_max"]
    mixture = bpf.mixtureFromHits(refined, TOTAL, xy_step, theta_step, CAP, SIGMA)
    return bpf.mixtureApplyMoments(mixture, rows, FLOOR, CEIL, take_mean=True)


def _run(exe, tmp_path, head, poses_path, poses, xy_step, theta_step, rows, scores):
    R, A = LATTICE
    names = ("rows", "scores", "hits_rows", "refined_rows", "comps")
    out = {name: str(tmp_path / (name + ".bin")) for name in names}
    res = subprocess.run([str(exe)] + head + [poses_path, str(R), repr(xy_step), str(A), repr(theta_step),
                                              repr(BASELINE)] + [out[name] for name in names],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    comps = _components(poses, rows, xy_step, theta_step)
    assert [int(v) for v in res.stdout.split()] == [rows.shape[0], scores.size, comps.shape[0]]
    assert open(out["rows"], "rb").read() == rows.tobytes()
    assert open(out["scores"], "rb").read() == scores.tobytes()
    assert open(out["hits_rows"], "rb").read() == rows.tobytes()
    assert open(out["refined_rows"], "rb").read() == rows.tobytes()
    assert open(out["comps"], "rb").read() == comps.tobytes()
    assert (rows["flags"] & 1).all() and comps.shape[0] > 1
    assert not np.all(comps["sigma"] == np.array(SIGMA)) and not np.all(comps["rotation"] == np.eye(3))


def test_planar_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    import pose_refine_ref as prr
    from test_gpu_pose_search import MAX_BEAMS, scanner_on
    geo, poses, xy_step, theta_step = prr.planar_case(orc, "lf", (1, 1, 3))
    xy_step, theta_step = xy_step / 4.0, theta_step / 8.0
    R, A = LATTICE
    e = bpf.Engine(0)
    try:
        m, sc = scanner_on(e, geo, "lf")
        rows, scores = sc.poseMoments(bpf.PlanarData(geo.ranges, geo.angles, geo.range_max), poses, R, xy_step, A,
                                      theta_step, BASELINE, scores=True)
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_moments_smoke")
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(cells=geo.cells.astype(np.int32),
                                                                lut=np.asarray(geo.lut, dtype=np.float32),
                                                                ranges=geo.ranges, angles=geo.angles, poses=poses))
    head = ["planar", paths["cells"], paths["lut"], paths["ranges"], paths["angles"], str(geo.size_x), str(geo.size_y),
            repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])), str(MAX_BEAMS)]
    _run(exe, tmp_path, head, paths["poses"], poses, xy_step, theta_step, rows, scores)


def test_cloud_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    from test_gpu_pose_refine import _room_poses
    from test_gpu_pose_search_cloud import RES, room, scanner_on
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc)
    poses = _room_poses()
    R, A = LATTICE
    xy_step, theta_step = RES, 0.1
    e = bpf.Engine(0)
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        rows, scores = sc.poseMoments(bpf.PointCloudData(pts), poses, R, xy_step, A, theta_step, BASELINE,
                                      scores=True)
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_moments_smoke")
    cells6 = np.concatenate([np.asarray(lut.min_cells), np.asarray(lut.max_cells)]).astype(np.int32)
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(
        pose_indices=np.asarray(lut.pose_indices, dtype=np.uint32),
        ratios=np.asarray(lut.distance_ratios, dtype=np.uint8), cells6=cells6, points=np.array(pts), poses=poses,
        tf7=np.array(list(tf_xyz) + list(tf_quat), dtype=np.float64)))
    head = ["cloud", paths["pose_indices"], paths["ratios"], paths["cells6"], paths["points"], paths["tf7"], repr(RES),
            repr(float(max_dist)), "128"]
    _run(exe, tmp_path, head, paths["poses"], poses, xy_step, theta_step, rows, scores)
