"""The pruned pose search through the C++ adapter (tests/cpp/pose_search_pruned_smoke.cpp) against the Python
binding: the pruned rows, the exhaustive rows and three merged ranges of the block list byte for byte, and the
stats."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_adapter_equals_python(orc, tmp_path):
    import badger_amcl_amd as bpf
    import cpp_driver
    from test_gpu_pose_search import MAX_BEAMS, geometry, scanner_on
    geo = geometry(orc, "G1")
    headings, stride, k, block = 4, 1, 64, 8
    e = bpf.Engine(0)
    try:
        m, sc = scanner_on(e, geo, "lf")
        data = bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)
        nb = sc.searchBlocks(stride, block)
        whole, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
        assert whole.shape[0] == k
        assert whole.tobytes() == sc.searchPoses(data, headings, stride, k).tobytes()
    finally:
        e.close()
    cut1, cut2 = nb // 3, nb // 2
    exe = cpp_driver.compile_driver(tmp_path, "pose_search_pruned_smoke")
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(cells=geo.cells.astype(np.int32),
                                                                lut=np.asarray(geo.lut, dtype=np.float32),
                                                                ranges=geo.ranges, angles=geo.angles))
    out = {name: str(tmp_path / (name + ".bin")) for name in ("pruned", "exhaustive", "merged")}
    res = subprocess.run([str(exe), paths["cells"], paths["lut"], paths["ranges"], paths["angles"], str(geo.size_x),
                          str(geo.size_y), repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])),
                          str(MAX_BEAMS), str(headings), str(stride), str(k), str(block), str(cut1), str(cut2),
                          out["pruned"], out["exhaustive"], out["merged"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    import badger_amcl_amd.pf as hpf
    assert [int(v) for v in res.stdout.split()] == [nb] + [st[name] for name in hpf.POSE_SEARCH_STATS_FIELDS]
    for name in out:
        assert open(out[name], "rb").read() == whole.tobytes(), name
