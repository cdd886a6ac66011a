"""Pruned pose search on the device (bpf_planar_search_poses_pruned): the rows of the exhaustive search byte for byte,
the bound above every member's score as doubles, ranges of the block list that compose, the accounting of the stats,
a filter left as it was, refusals, and the caches behind a new LUT.  Maps, beams and spaces are those of
tests/test_gpu_pose_search.py.

Pruning effect on these maps, scored_candidates / candidates with the scan ray-cast from the free centre pose, B = 8,
likelihood field (profiles/pose_search_pruned.md): see PRUNING_MEASURED below."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_search_pruned_ref as ppr  # noqa: E402
import pose_search_ref as psr  # noqa: E402
from test_gpu_pose_search import MAX_BEAMS, ORACLE_SPACES, _record, blind_scan, geometry, scanner_on  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = (2, 8, 64)
KS = (1, 64, 1024)
# (map, K) -> scored_candidates / candidates measured on an MI355X (B = 8, lf, the map's own scan); the cases below
# 0.5 are asserted to prune
PRUNING_MEASURED = {("G1", 1): 0.0882, ("G1", 64): 0.3803, ("G2", 1): 0.6510, ("G2", 64): 0.7843,
                    ("G3", 1): 1.0, ("G3", 64): 1.0}


def scan_of(geo):
    import badger_amcl_amd as bpf
    return bpf.PlanarData(geo.ranges, geo.angles, geo.range_max)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ 1. the same rows
@pytest.mark.parametrize("model", ["lf", "gompertz"])
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_same_rows_as_the_exhaustive_search(engine, orc, name, model):
    geo = geometry(orc, name)
    m, sc = scanner_on(engine, geo, model)
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES[name]
    total, _ = sc.searchSpace(headings, stride)
    for k in KS:
        want = sc.searchPoses(data, headings, stride, k)
        assert want.shape[0] == k
        for block in BLOCKS:
            got, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
            assert got.tobytes() == want.tobytes(), (name, model, k, block)
            assert st["candidates"] == total
            print("pruned search %s %s K=%d B=%d: scored %d of %d (%.3f), %d windows"
                  % (name, model, k, block, st["scored_candidates"], total, st["scored_candidates"] / total,
                     st["windows"]))


@pytest.mark.parametrize("model", ["lf", "gompertz"])
def test_stride_that_does_not_divide_the_block_and_k_above_the_space(engine, orc, model):
    geo = geometry(orc, "G3")
    m, sc = scanner_on(engine, geo, model)
    data = scan_of(geo)
    # stride 3 against B = 8 and 2: a block's members start at different offsets from its anchor
    for block in BLOCKS:
        for k in (1, 64):
            assert sc.searchPosesPruned(data, 9, 3, k, block).tobytes() == sc.searchPoses(data, 9, 3, k).tobytes()
    # fewer candidates than K: every candidate comes back, in order
    total, _ = sc.searchSpace(3, 7)
    assert 0 < total < 1024
    want = sc.searchPoses(data, 3, 7, 1024)
    assert want.shape[0] == total
    for block in BLOCKS:
        got, st = sc.searchPosesPruned(data, 3, 7, 1024, block, stats=True)
        assert got.tobytes() == want.tobytes()
        assert st["scored_candidates"] == total and st["pruned_block_candidates"] == 0


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_blind_scan_prunes_nothing_and_orders_by_candidate(engine, orc, name):
    geo = geometry(orc, name)
    m, sc = scanner_on(engine, geo, "lf")
    headings, stride = ORACLE_SPACES[name]
    sp = psr.Space.of(geo, headings, stride)
    for block in BLOCKS:
        for k in (1, 1024):
            got, st = sc.searchPosesPruned(blind_scan(geo), headings, stride, k, block, stats=True)
            assert np.all(got["score"] == 1.0)
            # (the exhaustive search's first k candidates are not the pruned call's seed: every block must be opened)
            assert np.array_equal(got["candidate"], np.arange(k))
            assert got.tobytes() == sc.searchPoses(blind_scan(geo), headings, stride, k).tobytes()
            assert st["pruned_block_candidates"] == 0 and st["scored_candidates"] == sp.total


# ------------------------------------------------------------------------------------ 2. the bound holds
def edge_scan(geo):
    """the map's scan with every third beam lengthened to 0.6 of the map's shorter side: from a pose within that
    distance of an edge -- every pose of these maps -- beams of all bearings leave the map"""
    import badger_amcl_amd as bpf
    ranges = geo.ranges.copy()
    long_beam = 0.6 * min(geo.size_x, geo.size_y) * geo.res
    assert long_beam < geo.range_max
    ranges[::3] = long_beam
    return bpf.PlanarData(ranges, geo.angles, geo.range_max)


@pytest.mark.parametrize("model", ["lf", "gompertz"])
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_bound_is_above_every_member(engine, orc, name, model):
    geo = geometry(orc, name)
    assert geo.map_factors[0] != 1.0 and geo.map_factors[1] != 1.0 and any(v != 0.0 for v in geo.scanner_pose)
    m, sc = scanner_on(engine, geo, model)
    headings, stride = ORACLE_SPACES[name]
    sp = psr.Space.of(geo, headings, stride)
    for data in (edge_scan(geo), scan_of(geo)):
        s = sp.samples(0, sp.total)
        sc.applyModelToSampleSet(data, s)
        scores = s[:, 3].reshape(-1, headings)  # [cell f, heading]
        assert np.all(np.isfinite(scores))
        for block in BLOCKS:
            blocks, start, member = ppr.block_list(sp.ij, block)
            assert sc.searchBlocks(stride, block) == blocks.shape[0]
            bounds = sc.searchBounds(data, headings, stride, block)
            assert bounds.shape[0] == blocks.shape[0] * headings
            best = np.maximum.reduceat(scores[member], start[:-1], axis=0).reshape(-1)  # [block, heading] = q order
            assert np.all(bounds >= best), (name, model, block, float((best - bounds).max()))
            # a range of the bounds is the same numbers
            part = sc.searchBounds(data, headings, stride, block, 5, 17)
            assert part.tobytes() == bounds[5:22].tobytes()


# ------------------------------------------------------------------------------------ 3. ranges compose
def test_ranges_of_the_block_list_compose(engine, orc):
    import badger_amcl_amd.pf as hpf
    geo = geometry(orc, "G1")
    m, sc = scanner_on(engine, geo, "lf")
    data = scan_of(geo)
    headings, stride = ORACLE_SPACES["G1"]
    k, block = 64, 8
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


# ------------------------------------------------------------------------------------ 4. stats
@pytest.mark.parametrize("name,model,k,block", [("G1", "lf", 1, 8), ("G1", "lf", 64, 8), ("G2", "gompertz", 64, 2),
                                                ("G3", "lf", 1024, 64), ("G2", "lf", 1, 8), ("G2", "lf", 64, 8),
                                                ("G3", "lf", 1, 8), ("G3", "lf", 64, 8)])
def test_stats_add_up(engine, orc, name, model, k, block):
    """Every stats field as an equality against pose_search_pruned_ref.replay: the call's decisions replayed in numpy
    from the bounds (searchBounds) and the members' exact scores (applyModelToSampleSet on the explicit poses)."""
    geo = geometry(orc, name)
    m, sc = scanner_on(engine, geo, model)
    headings, stride = ORACLE_SPACES[name]
    sp = psr.Space.of(geo, headings, stride)
    blocks, start, member = ppr.block_list(sp.ij, block)
    data = scan_of(geo)
    hits, st = sc.searchPosesPruned(data, headings, stride, k, block, stats=True)
    print("pruned search stats %s %s K=%d B=%d: %r ratio %.4f"
          % (name, model, k, block, st, st["scored_candidates"] / st["candidates"]))
    s = sp.samples(0, sp.total)
    sc.applyModelToSampleSet(data, s)
    scores = s[:, 3].reshape(-1, headings)
    assert np.all(np.isfinite(scores))
    # the explicit poses score as the search's candidates do, bit for bit: what the replay's tau rests on
    assert hits["score"].tobytes() == scores.reshape(-1)[hits["candidate"]].tobytes()
    bounds = sc.searchBounds(data, headings, stride, block)
    want = ppr.replay(bounds, scores, start, member, headings, k)
    assert want["best"].tobytes() == hits["score"].tobytes()
    assert st["candidates"] == sp.total
    for field in ("block_candidates", "seed_candidates", "pruned_block_candidates", "expanded_block_candidates",
                  "scored_candidates", "windows"):
        assert st[field] == want[field], (field, st, {f: v for f, v in want.items() if f != "best"})
    # the identities of the issue, which the replay satisfies by construction
    assert st["block_candidates"] == (st["seed_candidates"] + st["pruned_block_candidates"] +
                                      st["expanded_block_candidates"])
    assert st["scored_candidates"] <= st["candidates"]
    if PRUNING_MEASURED.get((name, k), 1.0) < 0.5 and model == "lf" and block == 8:
        assert st["scored_candidates"] < st["candidates"]


# ------------------------------------------------------------------------------------ 4b. the pooled image
@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_pooled_image_on_the_device_is_the_model(engine, orc, name):
    """P_B as the bound pass reads it against the numpy model, entry for entry, every B (B = 64 is wider than G3)"""
    geo = geometry(orc, name)
    m, sc = scanner_on(engine, geo, "lf")
    lut = np.asarray(geo.lut, dtype=np.float32).reshape(geo.size_y, geo.size_x)
    levels = np.unique(lut)  # ascending: the engine's level index
    codes = np.searchsorted(levels, lut).astype(np.int64) * 8
    off = levels.shape[0] * 8
    for block in ppr.BLOCKS:
        tiles, ltx, lty = sc.searchPooledLUT(block)
        assert (ltx, lty) == ppr.tile_shape(geo.size_x, geo.size_y)
        want = ppr.to_tiles(ppr.pooled(codes, off, block), off)
        assert tiles.shape == want.shape
        assert np.array_equal(tiles, want), (name, block, int(np.count_nonzero(tiles != want)))


# ------------------------------------------------------------------------------------ 5. nothing else moves
def _filter_run(orc, recovery, with_search):
    """likelihood field on G1, n = 2500; a fresh engine per run.  What the filter showed after every step, and the
    pruned search's hits."""
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from map_geometry import GeoScenario
    geo = GeoScenario.named(orc, "G1", n=2500, beams=61, frac_nan=0.0, cloud="mixture" if recovery else "converged")
    e = bpf.Engine(0)
    try:
        e.set_option(hpf.OPT_CDF_SERIAL, 1)
        alpha = (0.001, 0.5) if recovery else (0.0, 0.0)
        m, sc, pf, data = geo.gpu_objects(e, 61, "lf", min_samples=100, seed=31, alpha=alpha)
        scans = [geo.ranges, np.clip(geo.ranges * 0.6, 0.05, 29.0), np.full(61, 1.0)]
        if recovery:
            pf.setRandomPoseGenerator(hpf.RANDOM_POSE_FREE_SPACE_2D)
            pf.setUniformPoseCheck(1e-20, 0.5, hpf.POSE_CHECK_SENSOR_MODEL)  # scores against the remembered scan
        recs, hits = [], None
        sc.updateSensor(pf, bpf.PlanarData(scans[0], geo.angles, geo.range_max))
        if with_search:
            # another scan than the one the filter remembers for its pose check
            hits = sc.searchPosesPruned(bpf.PlanarData(scans[2], geo.angles, geo.range_max), 6, 2, 100, 8)
        recs.append(_record(pf))
        pf.updateResample()
        recs.append(_record(pf))
        for ranges in scans[1:]:
            sc.updateSensor(pf, bpf.PlanarData(ranges, geo.angles, geo.range_max))
            recs.append(_record(pf))
            pf.updateResample()
            recs.append(_record(pf))
        return recs, hits
    finally:
        e.close()


@pytest.mark.parametrize("recovery", [False, True])
def test_pruned_search_leaves_the_filter_as_it_found_it(orc, recovery):
    a, hits = _filter_run(orc, recovery, True)
    b, _ = _filter_run(orc, recovery, False)
    assert hits.shape[0] == 100 and np.all(np.isfinite(hits["score"]))
    assert len(a) == len(b)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["samples"], rb["samples"]), step
        for key in ("state", "rng", "max_w", "max_pose"):
            assert ra[key] == rb[key], (step, key)


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals(engine, orc):
    import badger_amcl_amd as bpf
    geo = geometry(orc, "G2")
    data = scan_of(geo)

    def refused(sc, code, **kw):
        args = dict(headings=4, cell_stride=1, k=8, block=8)
        args.update(kw)
        with pytest.raises(bpf.BpfError) as ei:
            sc.searchPosesPruned(data, **args)
        assert ei.value.code == code, (kw, ei.value.code)

    m, sc = scanner_on(engine, geo, "prob")
    refused(sc, 4)
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchBounds(data, 4, 1, 8)
    assert ei.value.code == 4
    m, sc = scanner_on(engine, geo, "beam")
    refused(sc, 4)
    for bad in (dict(gompertz_a=0.0), dict(gompertz_b=-1.0), dict(gompertz_c=0.0), dict(input_scale=-2.0)):
        m, sc = scanner_on(engine, geo, "gompertz", kw=bad)
        refused(sc, 4)
    m, sc = scanner_on(engine, geo, "lf")
    nb = sc.searchBlocks(1, 8)
    for kw in (dict(block=3), dict(block=0), dict(block=128), dict(first_block=nb + 1), dict(first_block=-1),
               dict(block_count=nb + 1), dict(first_block=1, block_count=nb), dict(block_count=-2), dict(k=0),
               dict(k=1025), dict(headings=0), dict(cell_stride=0)):
        refused(sc, 1, **kw)
    with pytest.raises(bpf.BpfError) as ei:
        sc.searchBlocks(1, 3)
    assert ei.value.code == 1
    # and the engine goes on
    assert sc.searchPosesPruned(data, 4, 1, 8, 8).tobytes() == sc.searchPoses(data, 4, 1, 8).tobytes()


# ------------------------------------------------------------------------------------ 7. caches
def test_a_new_lut_invalidates_the_pooled_image_and_the_block_list(orc):
    import badger_amcl_amd as bpf
    from map_geometry import GeoScenario
    e = bpf.Engine(0)
    try:
        geo = geometry(orc, "G2")
        other = GeoScenario.named(orc, "G2", beams=61, frac_nan=0.0, max_dist=0.7)
        assert not np.array_equal(np.asarray(geo.lut), np.asarray(other.lut))
        m, sc = scanner_on(e, geo, "lf")
        data = scan_of(geo)
        headings, stride = ORACLE_SPACES["G2"]
        first = sc.searchPosesPruned(data, headings, stride, 64, 8)
        assert first.tobytes() == sc.searchPoses(data, headings, stride, 64).tobytes()
        m.setDistancesLUT(other.lut, other.max_dist)
        second = sc.searchPosesPruned(data, headings, stride, 64, 8)
        want = sc.searchPoses(data, headings, stride, 64)
        assert second.tobytes() == want.tobytes()
        assert second.tobytes() != first.tobytes()
        # another radius: the block list follows the free list
        sc.setMapFactors(geo.map_factors[0], geo.map_factors[1], 0.1)
        assert sc.searchPosesPruned(data, headings, stride, 64, 8).tobytes() == \
            sc.searchPoses(data, headings, stride, 64).tobytes()
    finally:
        e.close()
