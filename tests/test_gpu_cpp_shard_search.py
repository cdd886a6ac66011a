"""Pose search over a sharded filter through the C++ adapter (include/badger_amcl_amd/adapter.hpp,
LocalShardedParticleFilter::searchPoses / searchPosesPruned / localize; tests/cpp/shard_search_local.cpp): W = 2 on
G1, the rows and the set localize() leaves compared with the Python side byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine library, as in test_gpu_shard_stats.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cpp_driver  # noqa: E402
from test_gpu_pose_search import MAX_BEAMS, ORACLE_SPACES, geometry, scanner_on  # noqa: E402
from test_gpu_pose_search_pruned import scan_of  # noqa: E402

pytestmark = pytest.mark.gpu


def test_local_world_searches_and_localize_through_the_adapter(orc, tmp_path):
    import badger_amcl_amd as bpf
    from badger_amcl_amd.local_world import LocalShardedFilter
    W, n, k, block = 2, 1000, 64, 8
    geo = geometry(orc, "G1")
    headings, stride = ORACLE_SPACES["G1"]
    exe = cpp_driver.compile_driver(tmp_path, "shard_search_local")
    paths = cpp_driver.write_case(tmp_path / "case", None, dict(cells=geo.cells.astype(np.int32),
                                                                lut=np.asarray(geo.lut, dtype=np.float32),
                                                                ranges=geo.ranges, angles=geo.angles))
    outs = [str(tmp_path / name) for name in ("rows.bin", "pruned.bin", "sets.bin")]
    res = subprocess.run([str(exe), paths["cells"], paths["lut"], paths["ranges"], paths["angles"], str(geo.size_x),
                          str(geo.size_y), repr(geo.res), repr(float(geo.origin[0])), repr(float(geo.origin[1])),
                          str(MAX_BEAMS), str(headings), str(stride), str(k), str(block), str(W), str(n)] + outs,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr

    # the Python side: one engine for the rows, a local world for the set
    data = scan_of(geo)
    engines = [bpf.Engine(0) for _ in range(W + 1)]
    try:
        keep = [scanner_on(e, geo, "lf") for e in engines]
        sc = keep[0][1]
        want = sc.searchPoses(data, headings, stride, k)
        total, _ = sc.searchSpace(headings, stride)
        assert open(outs[0], "rb").read() == want.tobytes()
        assert open(outs[1], "rb").read() == want.tobytes()
        pfs = []
        for e in engines[1:]:
            pf = bpf.ParticleFilter(e, 100, n, 0.0, 0.0, 85.0)
            pf.srand48(7)
            pfs.append(pf)
        f = LocalShardedFilter(pfs, kld_count=0)
        try:
            _, stats = f.search_poses_pruned(data, headings, stride, k, block)
            comps = f.localize([kp[1] for kp in keep[1:]], data, headings, stride, k,
                               (2, geo.res / 2, 2, 0.02, 2),
                               (2, geo.res / 2, 2, 0.02, 0.5, (0.01, 0.01, 0.01), (1.0, 1.0, 1.0)),
                               (0.5, 0.5, 8, (0.1, 0.1, 0.05)), pruned=True, block=block)
            sets = np.concatenate(f.local_sets())
        finally:
            f.close()
        figures = [int(v) for v in res.stdout.split()]
        assert figures == [k, k, k, total, sum(st["scored_candidates"] for st in stats), comps.shape[0], n]
        assert open(outs[2], "rb").read() == sets.tobytes()
    finally:
        for e in engines:
            e.close()
