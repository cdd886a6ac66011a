"""The pruned cloud pose search through the C++ adapter (tests/cpp/pose_search_cloud_pruned_smoke.cpp) against the
Python binding: the pruned rows, the exhaustive rows and three merged ranges of the block list byte for byte, the
stats, the bounds and the pooled volume."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gompertz", [0, 1])
def test_adapter_equals_python(orc, tmp_path, gompertz):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    import cpp_driver
    from test_gpu_pose_search_cloud_pruned import cloud, hall, scanner_on, tf_of
    lut, _, max_dist = hall(orc)
    pts = np.array(cloud(orc, "cast2"))
    tf_xyz, tf_quat = tf_of(0.05)
    headings, stride, k, block = 6, 1, 64, 2  # 2 016 block candidates: a seed, pruned and expanded ones
    e = bpf.Engine(0)
    try:
        # (the adapter program sets sigma 0.1 and the factors 0.95, as scanner_on does at resolution 0.05)
        om, sc = scanner_on(e, lut, max_dist, 0.05, "gompertz" if gompertz else "plain")
        data = bpf.PointCloudData(pts)
        nb = sc.searchBlocks(stride, block)
        whole, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
        assert whole.shape[0] == k
        assert whole.tobytes() == sc.searchPoses(data, headings, stride, k).tobytes()
        assert st["seed_candidates"] == 1024 and st["block_candidates"] == nb * headings
        bounds = sc.searchBounds(data, headings, stride, block)
        pooled, ntx, nty, planes = sc.searchPooledLut(block)
    finally:
        e.close()
    cut1, cut2 = nb // 3, nb // 2
    exe = cpp_driver.compile_driver(tmp_path, "pose_search_cloud_pruned_smoke")
    cells6 = np.concatenate([np.asarray(lut.min_cells), np.asarray(lut.max_cells)]).astype(np.int32)
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(
        pose_indices=np.asarray(lut.pose_indices, dtype=np.uint32),
        ratios=np.asarray(lut.distance_ratios, dtype=np.uint8), cells6=cells6, points=pts,
        tf7=np.array(list(tf_xyz) + list(tf_quat), dtype=np.float64)))
    out = {name: str(tmp_path / (name + ".bin")) for name in ("pruned", "exhaustive", "merged", "bounds", "pooled")}
    res = subprocess.run([str(exe), paths["pose_indices"], paths["ratios"], paths["cells6"], paths["points"],
                          paths["tf7"], repr(0.05), repr(float(max_dist)), "128", str(gompertz), str(headings),
                          str(stride), str(k), str(block), str(cut1), str(cut2), out["pruned"], out["exhaustive"],
                          out["merged"], out["bounds"], out["pooled"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert [int(v) for v in res.stdout.split()] == [nb, ntx, nty, planes] + \
        [st[name] for name in hpf.POSE_SEARCH_STATS_FIELDS]
    for name in ("pruned", "exhaustive", "merged"):
        assert open(out[name], "rb").read() == whole.tobytes(), name
    assert open(out["bounds"], "rb").read() == bounds.tobytes()
    assert open(out["pooled"], "rb").read() == pooled.tobytes()
