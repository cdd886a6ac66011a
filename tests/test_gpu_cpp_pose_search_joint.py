"""The joint pose search through the C++ adapter's PlanarScanner::searchPosesJoint and
PointCloudScanner::searchPosesJoint (tests/cpp/pose_search_joint.cpp) against the Python binding: the rows byte for
byte, one planar and one cloud case of three scans each."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_planar_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    from test_gpu_pose_search import MAX_BEAMS, scanner_on
    from test_gpu_pose_search_joint import scans_of
    geo, offs, datas = scans_of(orc, "G1")
    headings, stride, k = 4, 1, 64  # three windows
    e = bpf.Engine(0)
    try:
        m, sc = scanner_on(e, geo, "lf")
        want = sc.searchPosesJoint(datas, offs, headings, stride, k)
        assert want.shape[0] == k
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_search_joint")
    arrays = dict(cells=geo.cells.astype(np.int32), lut=np.asarray(geo.lut, dtype=np.float32), offsets=offs)
    for s, d in enumerate(datas):
        arrays["ranges%d" % s] = d.ranges_
        arrays["angles%d" % s] = d.angles_
    paths = cpp_driver.write_case(tmp_path / "case", None, arrays)
    out = str(tmp_path / "hits.bin")
    scans = [paths[n + str(s)] for s in range(len(datas)) for n in ("ranges", "angles")]
    res = subprocess.run([str(exe), "planar", paths["cells"], paths["lut"], str(geo.size_x), str(geo.size_y),
                          repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])), str(MAX_BEAMS),
                          repr(float(geo.range_max)), str(headings), str(stride), str(k), str(len(datas)),
                          paths["offsets"], out] + scans, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout.split()[0]) == k
    assert open(out, "rb").read() == want.tobytes()


def test_cloud_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    from test_gpu_pose_search_cloud import H, RES, S, room, scanner_on
    from test_gpu_pose_search_cloud_joint import OFFSETS, clouds_of
    lut, pts, tf_xyz, tf_quat, max_dist = room(orc, True)  # the pitched mounting: the general kernel
    datas = clouds_of(orc, True)
    k = 64
    e = bpf.Engine(0)
    try:
        om, sc = scanner_on(e, lut, tf_xyz, tf_quat, max_dist, "gompertz")
        want = sc.searchPosesJoint(datas, OFFSETS, H, S, k)
        assert want.shape[0] == k
    finally:
        e.close()
    exe = cpp_driver.compile_driver(tmp_path, "pose_search_joint")
    cells6 = np.concatenate([np.asarray(lut.min_cells), np.asarray(lut.max_cells)]).astype(np.int32)
    arrays = dict(pose_indices=np.asarray(lut.pose_indices, dtype=np.uint32),
                  ratios=np.asarray(lut.distance_ratios, dtype=np.uint8), cells6=cells6, offsets=OFFSETS,
                  tf7=np.array(list(tf_xyz) + list(tf_quat), dtype=np.float64))
    for s, d in enumerate(datas):
        arrays["points%d" % s] = d.points_
    paths = cpp_driver.write_case(tmp_path / "case", None, arrays)
    out = str(tmp_path / "hits.bin")
    res = subprocess.run([str(exe), "cloud", paths["pose_indices"], paths["ratios"], paths["cells6"], paths["tf7"],
                          repr(RES), repr(float(max_dist)), "128", "1", str(H), str(S), str(k), str(len(datas)),
                          paths["offsets"], out] + [paths["points%d" % s] for s in range(len(datas))],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout.split()[0]) == k
    assert open(out, "rb").read() == want.tobytes()
