"""Pruned pose search with the cloud scanner on the device (bpf_cloud_search_poses_pruned): the pooled volume against
the numpy model byte for byte, the bound above every member's score as doubles, the rows of the exhaustive search as
bytes, ranges of the block list that compose, every stats field against the replay, refusals, and a filter left as
it was.

Maps: "the hall", occupied voxels (-18, -12, 0) .. (21, 17, 5) with two interior walls, cell bounds (-19, -13, 0) ..
(22, 18, 5): 41 x 31 columns of the rectangle, 42 x 32 x 6 cells, none of the bounds a multiple of 2; and "the wide
hall", 121 x 101 columns (one window of candidates and a part at H = 7).  Resolution 0.05 takes the exact-reciprocal
kernel, 0.03 the other.  Clouds: ray-cast from a pose inside the hall (300 points, and 2048 + 77: two LDS chunks, the
second with padding lanes), a ring of points 0.12 m around the scanner (in the open every point is beyond max_dist:
many equal scores), and the ray-cast cloud with NaN / inf coordinates."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_cloud_pruned_ref as pcr  # noqa: E402

pytestmark = pytest.mark.gpu

GZ = dict(gompertz_a=0.748, gompertz_b=5.0, gompertz_c=1.2, input_shift=-3.2, input_scale=6.7, output_shift=0.25)
TF_YAW = 0.3
TRUE = (-0.4, -0.3, 0.1)  # at resolution 0.05; scaled with the resolution
_MAPS, _CLOUDS = {}, {}


def hall_voxels(lo, hi):
    from badger_amcl_amd import synth
    occ = [synth.box_room_voxels(lo, hi, pillar=False)]
    extra = []
    for k in range(lo[2], hi[2] + 1):
        extra += [(2, j, k) for j in range(lo[1], 6) if not 0 <= j - lo[1] - 5 < 4]  # a wall with a door
        extra += [(i, 4, k) for i in range(8, hi[0] + 1) if not 0 <= i - 12 < 4]
        if hi[0] > 40:
            extra += [(i, -5, k) for i in range(lo[0], 60) if i % 17 > 3]
            extra += [(70, j, k) for j in range(lo[1], hi[1] + 1) if j % 23 > 4]
    occ.append(np.array(extra, dtype=np.int32))
    return np.unique(np.concatenate(occ), axis=0)


def hall(orc, res=0.05, wide=False):
    """(lut, occupied voxels, max_dist) of the hall, built once per (resolution, size)"""
    key = (res, wide)
    if key not in _MAPS:
        lo, hi = ((-18, -12, 0), (101, 87, 5)) if wide else ((-18, -12, 0), (21, 17, 5))
        occ = hall_voxels(lo, hi)
        mn = (lo[0] - 1, lo[1] - 1, lo[2])
        mx = (hi[0] + 1, hi[1] + 1, hi[2])
        max_dist = 6 * res
        lut = orc.OctoMapLUT(mn, mx, res, max_dist).build(occ)
        _MAPS[key] = (lut, occ, max_dist)
    return _MAPS[key]


def tf_of(res):
    s = res / 0.05
    return (0.1 * s, -0.05 * s, 0.12 * s), (0.0, 0.0, np.sin(TF_YAW / 2), np.cos(TF_YAW / 2))


def cloud(orc, kind, res=0.05):
    """float32 [n, 3] in the scanner frame, built once: "cast" 300 points, "cast2" 2048 + 77, "castw" 300 cast in
    the wide hall, "ring" 300, "nan" the 300 with non-finite coordinates among them"""
    key = (kind, res)
    if key not in _CLOUDS:
        from badger_amcl_amd import synth
        _, occ, _ = hall(orc, res, wide=(kind == "castw"))
        s = res / 0.05
        tf_xyz, _ = tf_of(res)
        x, y, yaw = TRUE[0] * s, TRUE[1] * s, TRUE[2]
        sx = x + np.cos(yaw) * tf_xyz[0] - np.sin(yaw) * tf_xyz[1]
        sy = y + np.sin(yaw) * tf_xyz[0] + np.cos(yaw) * tf_xyz[1]
        if kind in ("cast", "cast2", "castw", "nan"):
            rows, cols = (5, 425) if kind == "cast2" else (3, 100)
            pts = synth.sphere_cloud(rows, cols, (sx, sy, tf_xyz[2]), occ, res, seed=2)
            assert pts.shape[0] == rows * cols  # a closed hall: every ray ends on a voxel
            a = -(yaw + TF_YAW)
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            pts = (pts @ R.T).astype(np.float32)
            if kind == "nan":
                pts[5, 0] = np.nan
                pts[17, 1] = np.inf
                pts[40, 2] = -np.inf
                pts[77] = np.nan
                pts[120, :2] = (np.inf, np.inf)
        else:
            az = np.linspace(-np.pi, np.pi, 300, endpoint=False)
            pts = np.stack([0.12 * s * np.cos(az), 0.12 * s * np.sin(az), np.zeros(300)], axis=1).astype(np.float32)
        pts = np.ascontiguousarray(pts)
        pts.setflags(write=False)
        _CLOUDS[key] = pts
    return _CLOUDS[key]


def scanner_on(engine, lut, max_dist, res=0.05, model="plain", factor=0.95, max_beams=128, tf=None):
    """3-D map + cloud scanner on the engine, no filter"""
    import badger_amcl_amd as bpf
    om = bpf.OctoMap(engine, res)
    om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
    sc = bpf.PointCloudScanner(engine)
    sc.init(max_beams, om)
    if model == "plain":
        sc.setPointCloudModel(0.5, 0.05, 0.1 * (res / 0.05))
    else:
        sc.setPointCloudModelGompertz(0.5, 0.5, 0.1 * (res / 0.05), GZ["gompertz_a"], GZ["gompertz_b"],
                                      GZ["gompertz_c"], GZ["input_shift"], GZ["input_scale"], GZ["output_shift"])
    sc.setMapFactors(factor, factor, 0.3)
    tf_xyz, tf_quat = tf if tf is not None else tf_of(res)
    sc.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
    return om, sc


def space_of(lut, res, headings, stride):
    return pcr.Space(list(lut.min_cells), list(lut.max_cells), res, headings, stride)


def exact_scores(sc, data, sp):
    """[column f, heading] scores of every candidate through the seam (bit for bit the search's scores)"""
    s = sp.samples(0, sp.total)
    sc.applyModelToSampleSet(data, s)
    return s[:, 3].reshape(-1, sp.headings)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ 1. the pooled volume
def test_pooled_volume_on_the_device_is_the_model(engine, orc):
    """P_B as the bound pass reads it, byte for byte: B = 2, 4, 8 and B = 64, wider than the hall"""
    lut, _, max_dist = hall(orc)
    om, sc = scanner_on(engine, lut, max_dist)
    vol = pcr.ratios_volume(lut.pose_indices, lut.distance_ratios, lut.width, lut.height, lut.num_z)
    border, zero = pcr.free_codes(lut.distance_ratios)
    assert border >= 0 and (lut.width, lut.height, lut.num_z) == (42, 32, 6)
    for block in (2, 4, 8, 64):
        got, ntx, nty, planes = sc.searchPooledLut(block)
        want, wtx, wty = pcr.to_dense(pcr.pooled_planes(vol, block), border, zero)
        assert (ntx, nty, planes) == (wtx, wty, lut.num_z + 1)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (block, int(np.count_nonzero(got != want)))
    # the volume pools something: B = 2 differs from B = 8
    assert not np.array_equal(sc.searchPooledLut(2)[0], sc.searchPooledLut(8)[0])


# ------------------------------------------------------------------------------------ 2. the bound holds
@pytest.mark.parametrize("factor", [1.3, 0.8])
@pytest.mark.parametrize("res", [0.05, 0.03])
@pytest.mark.parametrize("model", ["plain", "gompertz"])
def test_bound_is_above_every_member(engine, orc, model, res, factor):
    """every block candidate of the hall, compared as doubles with no tolerance; poses near the edges put points off
    the map on every side, the anchors of the first block row and column lie outside the rectangle"""
    import badger_amcl_amd as bpf
    lut, _, max_dist = hall(orc, res)
    om, sc = scanner_on(engine, lut, max_dist, res, model, factor)
    headings = 5
    for kind, stride in (("cast", 1), ("cast2", 2), ("nan", 1)):
        data = bpf.PointCloudData(np.array(cloud(orc, kind, res)))
        sp = space_of(lut, res, headings, stride)
        scores = exact_scores(sc, data, sp)
        # EXACT_RINV (bit 0) at 0.05 only; PLANAR, DENSE and BORDER (bits 1 .. 3) always
        assert engine.cloud_last_form() & 15 == (15 if res == 0.05 else 14)
        assert np.all(np.isfinite(scores)) and len(np.unique(scores)) > 100
        for block in (2, 4, 8):
            blocks, start, member = pcr.block_list(sp, block)
            assert sc.searchBlocks(stride, block) == blocks.shape[0]
            bounds = sc.searchBounds(data, headings, stride, block)
            assert bounds.shape[0] == blocks.shape[0] * headings
            best = np.maximum.reduceat(scores[member], start[:-1], axis=0).reshape(-1)  # [block, heading] = q order
            assert np.all(bounds >= best), (model, res, factor, kind, block, float((best - bounds).max()))
            part = sc.searchBounds(data, headings, stride, block, 5, 17)
            assert part.tobytes() == bounds[5:22].tobytes()
        assert blocks[0, 0] * block < lut.min_cells[0] and blocks[0, 1] * block < lut.min_cells[1]


# ------------------------------------------------------------------------------------ 3. the same rows
@pytest.mark.parametrize("kind", ["cast", "cast2", "ring", "nan"])
@pytest.mark.parametrize("model", ["plain", "gompertz"])
def test_same_rows_as_the_exhaustive_search(engine, orc, model, kind):
    import badger_amcl_amd as bpf
    lut, _, max_dist = hall(orc)
    om, sc = scanner_on(engine, lut, max_dist, 0.05, model)
    data = bpf.PointCloudData(np.array(cloud(orc, kind)))
    headings = 6
    for stride in (1, 2):
        total, _ = sc.searchSpace(headings, stride)
        for k in (1, 7, 64, 1024):
            want = sc.searchPoses(data, headings, stride, k)
            assert want.shape[0] == min(k, total)
            if kind == "ring" and k >= 64:
                assert len(np.unique(want["score"])) < want.shape[0]  # ties, ordered by candidate
            for block in (2, 4, 8):
                got, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
                assert got.tobytes() == want.tobytes(), (model, kind, stride, k, block)
                assert st["candidates"] == total
                assert st["block_candidates"] == (st["seed_candidates"] + st["pruned_block_candidates"] +
                                                  st["expanded_block_candidates"])
                assert st["scored_candidates"] <= st["candidates"]


@pytest.mark.parametrize("model", ["plain", "gompertz"])
def test_same_rows_over_more_than_one_window(engine, orc, model):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    lut, _, max_dist = hall(orc, wide=True)
    om, sc = scanner_on(engine, lut, max_dist, 0.05, model)
    data = bpf.PointCloudData(np.array(cloud(orc, "cast")))
    headings, stride = 7, 1
    total, cols = sc.searchSpace(headings, stride)
    assert cols == 121 * 101 and hpf.pose_search_window() < total < 2 * hpf.pose_search_window()
    for k, block in ((64, 4), (1, 2), (1024, 8)):
        want = sc.searchPoses(data, headings, stride, k)
        got, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
        assert got.tobytes() == want.tobytes(), (model, k, block)
        print("pruned cloud search wide hall %s K=%d B=%d: scored %d of %d (%.3f), %d windows"
              % (model, k, block, st["scored_candidates"], total, st["scored_candidates"] / total, st["windows"]))
    # max_beams < 2: every score 1.0, nothing pruned, the first k candidates
    om, sc = scanner_on(engine, lut, max_dist, 0.05, model, max_beams=1)
    got, st = sc.searchPosesPruned(data, headings, stride, 64, 4, stats=True)
    assert got.tobytes() == sc.searchPoses(data, headings, stride, 64).tobytes()
    assert np.array_equal(got["candidate"], np.arange(64)) and np.all(got["score"] == 1.0)
    assert st["pruned_block_candidates"] == 0 and st["scored_candidates"] == total


# ------------------------------------------------------------------------------------ 4. ranges compose
def test_ranges_of_the_block_list_compose(engine, orc):
    import badger_amcl_amd.pf as hpf
    import badger_amcl_amd as bpf
    lut, _, max_dist = hall(orc)
    om, sc = scanner_on(engine, lut, max_dist)
    data = bpf.PointCloudData(np.array(cloud(orc, "cast")))
    headings, stride, k, block = 6, 1, 64, 4
    nb = sc.searchBlocks(stride, block)
    assert nb > 8
    whole = sc.searchPosesPruned(data, headings, stride, k, block)
    assert whole.tobytes() == sc.searchPoses(data, headings, stride, k).tobytes()
    cuts = [0, 1, nb // 2, nb - 1, nb]
    parts, scored = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        hits, st = sc.searchPosesPruned(data, headings, stride, k, block, a, b - a, stats=True)
        assert st["block_candidates"] == (b - a) * headings
        parts.append(hits)
        scored += st["candidates"]
    assert scored == sc.searchSpace(headings, stride)[0]
    assert hpf.merge_pose_hits(parts, k).tobytes() == whole.tobytes()
    assert sc.searchPosesPruned(data, headings, stride, k, block, nb, -1).shape[0] == 0  # the empty range at the end


# ------------------------------------------------------------------------------------ 5. stats
def _stats_case(engine, orc, wide, model, kind, headings, stride, k, block):
    import badger_amcl_amd as bpf
    lut, _, max_dist = hall(orc, wide=wide)
    om, sc = scanner_on(engine, lut, max_dist, 0.05, model)
    data = bpf.PointCloudData(np.array(cloud(orc, kind)))
    sp = space_of(lut, 0.05, headings, stride)
    blocks, start, member = pcr.block_list(sp, block)
    hits, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
    scores = exact_scores(sc, data, sp)
    assert hits["score"].tobytes() == scores.reshape(-1)[hits["candidate"]].tobytes()
    bounds = sc.searchBounds(data, headings, stride, block)
    want = pcr.replay(bounds, scores, start, member, headings, k)
    assert want["best"].tobytes() == hits["score"].tobytes()
    assert st["candidates"] == sp.total
    for field in ("block_candidates", "seed_candidates", "pruned_block_candidates", "expanded_block_candidates",
                  "scored_candidates", "windows"):
        assert st[field] == want[field], (field, st, {f: v for f, v in want.items() if f != "best"})
    return st


@pytest.mark.parametrize("wide,model,kind,headings,stride,k,block",
                         [(False, "plain", "cast", 6, 1, 64, 2), (False, "gompertz", "cast2", 6, 2, 7, 2),
                          (False, "plain", "ring", 6, 1, 1024, 8), (False, "plain", "nan", 5, 1, 1, 2),
                          (True, "gompertz", "cast", 7, 1, 64, 8)])
def test_stats_equal_the_replay(engine, orc, wide, model, kind, headings, stride, k, block):
    """every stats field against pose_search_cloud_pruned_ref.replay, from the device's bounds and the exact scores"""
    st = _stats_case(engine, orc, wide, model, kind, headings, stride, k, block)
    print("pruned cloud search stats wide=%d %s %s K=%d B=%d: %r" % (wide, model, kind, k, block, st))


def test_the_hall_with_interior_walls_prunes(engine, orc):
    """The wide hall (interior walls), the cloud ray-cast from a pose inside it, K = 1, B = 4: chosen so that the
    replay on the CPU, from the oracle's scores and the model's bounds, scores less than half of the candidates."""
    st = _stats_case(engine, orc, True, "plain", "castw", 7, 1, 1, 4)
    print("pruned cloud search, wide hall K=1 B=4: scored share %.4f (%d of %d)"
          % (st["scored_candidates"] / st["candidates"], st["scored_candidates"], st["candidates"]))
    assert st["scored_candidates"] < st["candidates"]


# ------------------------------------------------------------------------------------ 6. refusals, nothing else moves
def _refusals(e, sc, om, lut, max_dist, pts):
    """every refusal of the call on an engine with the hall-like map `lut`; leaves the scanner as scanner_on set it"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    data = bpf.PointCloudData(pts)

    def refused(code, d=data, **kw):
        args = dict(headings=4, cell_stride=1, k=8, block=8)
        args.update(kw)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchPosesPruned(d, **args)
        assert ei.value.code == code, (kw, ei.value.code)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchBounds(d, args["headings"], args["cell_stride"], args["block"])
        if code == 4:
            assert ei.value.code == 4

    tf_xyz, tf_quat = tf_of(0.05)
    # roll / pitch
    q = np.array([0.05, 0.07, np.sin(0.15), np.cos(0.15)])
    sc.setPointCloudScannerToFootprintTF(tf_xyz, tuple(q / np.linalg.norm(q)))
    refused(4)
    sc.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
    # the dense volume switched off; a LUT that leaves no two ratios free
    e.set_option(hpf.OPT_CLOUD_DENSE, 0)
    refused(4)
    e.set_option(hpf.OPT_CLOUD_DENSE, 1)
    full = np.concatenate([np.asarray(lut.distance_ratios, dtype=np.uint8), np.arange(256, dtype=np.uint8)])
    om.setDistancesLUT(lut.pose_indices, full, lut.min_cells, lut.max_cells, max_dist)
    refused(4)
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchPooledLut(8)
    assert ei.value.code == 4
    om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
    # a term table that rises with the distance; a negative factor; a Gompertz that falls
    sc.setPointCloudModel(-0.5, 0.05, 0.1)
    refused(4)
    sc.setPointCloudModelGompertz(0.5, 0.5, 0.1, GZ["gompertz_a"], -1.0, GZ["gompertz_c"], GZ["input_shift"],
                                  GZ["input_scale"], GZ["output_shift"])
    refused(4)
    sc.setPointCloudModel(0.5, 0.05, 0.1)
    sc.setMapFactors(-0.5, 0.95, 0.3)
    refused(4)
    sc.setMapFactors(0.95, 0.95, 0.3)
    # a cloud beyond the coordinate limit: (2e5 + ...) * 2^-21 > 0.05
    far = pts.copy()
    far[3, 0] = 2.0e5
    refused(4, d=bpf.PointCloudData(far))
    # arguments
    nb = sc.searchBlocks(1, 8)
    for kw in (dict(block=3), dict(block=0), dict(block=128), dict(first_block=nb + 1), dict(first_block=-1),
               dict(block_count=nb + 1), dict(first_block=1, block_count=nb), dict(block_count=-2), dict(k=0),
               dict(k=1025), dict(headings=0), dict(cell_stride=0)):
        args = dict(headings=4, cell_stride=1, k=8, block=8)
        args.update(kw)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchPosesPruned(data, **args)
        assert ei.value.code == 1, kw
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchBlocks(1, 3)
    assert ei.value.code == 1
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchPosesPruned(data, 1 << 29, 1, 8, 8)
    assert ei.value.code == 8
    # and the engine goes on
    assert sc.searchPosesPruned(data, 4, 1, 8, 8).tobytes() == sc.searchPoses(data, 4, 1, 8).tobytes()


def test_refusals(orc):
    import badger_amcl_amd as bpf
    lut, _, max_dist = hall(orc)
    pts = np.array(cloud(orc, "cast"))
    e = bpf.Engine(0)
    try:
        # no cloud model: not configured, with and without the 3-D map
        sc0 = bpf.PointCloudScanner(e)
        with pytest.raises(bpf.BpfError) as ei:
            sc0.searchPosesPruned(bpf.PointCloudData(pts), 4, 1, 8, 8)
        assert ei.value.code == 2
        om = bpf.OctoMap(e, 0.05)
        om.setDistancesLUT(lut.pose_indices, lut.distance_ratios, lut.min_cells, lut.max_cells, max_dist)
        assert sc0.searchBlocks(1, 8) > 0  # the block list needs the map only
        with pytest.raises(bpf.BpfError) as ei:
            sc0.searchPosesPruned(bpf.PointCloudData(pts), 4, 1, 8, 8)
        assert ei.value.code == 2
        om, sc = scanner_on(e, lut, max_dist)
        pf = bpf.ParticleFilter(e, 10, 100, 0.0, 0.0, 85.0)  # its state shows last_status and the evaluations
        before = bytes(pf.getState())
        _refusals(e, sc, om, lut, max_dist, pts)
        assert bytes(pf.getState()) == before
    finally:
        e.close()


def _filter_run(orc, with_search):
    """the 3-D cycle of tests/test_gpu_pose_search_cloud.py on a fresh engine, with pruned searches, bound calls and
    every refusal between its steps, or without them"""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_cloud import _setup
    from test_gpu_pose_search_cloud import _record
    from test_gpu_pose_search_cloud import scanner_on as room_scanner_on
    n = 2000
    lut, pts, s, tf_xyz, tf_quat, max_dist = _setup(orc, n, 8, 256, seed=4)
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        om, sc = room_scanner_on(e, lut, tf_xyz, tf_quat, max_dist)
        pf = bpf.ParticleFilter(e, 100, n, 0.001, 0.5, 85.0)
        pf.srand48(11)
        pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_3D)
        pf.initWithSamples(s)
        other = bpf.PointCloudData(np.ascontiguousarray(pts[::3] * np.float32(0.8)))  # not the filter's cloud
        recs, hits = [], []
        for step, scan in enumerate((pts, np.ascontiguousarray(pts * np.float32(0.5)))):
            assert sc.updateSensor(pf, bpf.PointCloudData(scan))
            if with_search:
                hits.append((sc.searchPosesPruned(other, 6, 2, 100, 8), sc.searchPoses(other, 6, 2, 100)))
                with pytest.raises(bpf.BpfError):
                    sc.searchPosesPruned(other, 6, 2, 100, 5)
                if step == 0:
                    sc.setPointCloudScannerToFootprintTF(tf_xyz, (0.05, 0.0, 0.0, np.sqrt(1 - 0.0025)))
                    with pytest.raises(bpf.BpfError):
                        sc.searchPosesPruned(other, 6, 2, 100, 8)
                    sc.setPointCloudScannerToFootprintTF(tf_xyz, tf_quat)
            recs.append(_record(e, pf))
            pf.updateResample()
            if with_search:
                hits.append((sc.searchPosesPruned(other, 24, 1, 100, 4), sc.searchPoses(other, 24, 1, 100)))
                assert sc.searchBounds(other, 24, 1, 4).shape[0] == sc.searchBlocks(1, 4) * 24
            recs.append(_record(e, pf))
        return recs, hits
    finally:
        e.close()


def test_pruned_search_leaves_the_filter_as_it_found_it(orc):
    a, hits = _filter_run(orc, True)
    b, _ = _filter_run(orc, False)
    assert len(hits) == 4
    for pruned, whole in hits:
        assert pruned.shape[0] == 100 and pruned.tobytes() == whole.tobytes()
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose", "form"):
            assert ra[key] == rb[key], (step, key)


def test_a_new_map_invalidates_the_pooled_volume_and_the_block_list(orc):
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    try:
        lut, _, max_dist = hall(orc)
        wide, _, _ = hall(orc, wide=True)
        om, sc = scanner_on(e, lut, max_dist)
        data = bpf.PointCloudData(np.array(cloud(orc, "cast")))
        first = sc.searchPosesPruned(data, 6, 1, 64, 4)
        assert first.tobytes() == sc.searchPoses(data, 6, 1, 64).tobytes()
        nb = sc.searchBlocks(1, 4)
        om.setDistancesLUT(wide.pose_indices, wide.distance_ratios, wide.min_cells, wide.max_cells, max_dist)
        assert sc.searchBlocks(1, 4) > nb
        second = sc.searchPosesPruned(data, 6, 1, 64, 4)
        assert second.tobytes() == sc.searchPoses(data, 6, 1, 64).tobytes()
        assert second.tobytes() != first.tobytes()
    finally:
        e.close()
