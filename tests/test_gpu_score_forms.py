"""The forms of the planar scoring driver that no other file reaches, against the oracle: the likelihood-field table
read from global memory (more table entries than kTableLdsMax = 2048 of engine_state.hpp), the refusal of a scan with
more than 4096 beams followed by a full turn of the scan staging ring (kRing = 4), and the staging shortcuts (every
beam kept; a NaN, a range at range_max and an absurdly long one) on a set of one wave plus one particle.

Weights: 1e-9 relative with the knife-edge budget of test_gpu_parity.py; totals 1e-9 relative."""
import numpy as np
import pytest

from badger_amcl_amd import synth
from scenario import Scenario, rel_err
from test_gpu_parity import W_TOL, _knife_edge_budget

pytestmark = pytest.mark.gpu

K_TABLE_LDS_MAX = 2048   # engine_state.hpp
K_RING = 4               # engine_state.hpp
ERR_CAPACITY = 8         # BPF_ERR_CAPACITY
BEAMSKIP = dict(do_beamskip=1, beam_skip_distance=0.5, beam_skip_threshold=0.3, beam_skip_error_threshold=0.9)


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def check_weights(got, want, n_evals, what):
    bad = rel_err(got, want) > W_TOL
    assert bad.sum() <= _knife_edge_budget(n_evals), (what, int(bad.sum()), np.flatnonzero(bad)[:10])


def check_total(total, want_total, what):
    assert abs(total - want_total) <= 1e-9 * abs(want_total), (what, total, want_total)


def oracle_update_sensor(orc, sc_, p, samples, ranges, angles, range_max):
    """The oracle's updateSensor on `samples`: (normalised weights, total)."""
    n = samples.shape[0]
    opf = orc.ParticleFilter(100, n, 0.0, 0.0, 85.0)
    opf.set_samples(samples, leaf_count=1)
    total = opf.update_sensor(lambda s, conv: orc.planar_apply(p, sc_.omap, s, ranges, angles, range_max, conv))
    return opf.samples[:n, 3].copy(), total


# ---------------------------------------------------------------------------------------------- a. table in global memory
class OpenFloor(Scenario):
    """128 x 128 free cells with two occupied ones far apart and a LUT out to 4.6 m: the distances to the nearer of
    the two take more than 2048 distinct values, where every map of synth.make_map gives a few hundred."""

    def __init__(self, orc, n, beams, seed=3):
        self.orc = orc
        self.size, self.res = 128, 0.05
        self.cells = np.full((128, 128), -1, dtype=np.int32)
        self.cells[3, 4] = 1
        self.cells[126, 123] = 1
        self.origin = (np.float32(64 * self.res), np.float32(64 * self.res))
        self.omap = orc.OccupancyMap(self.cells, self.res, self.origin)
        self.max_dist = 4.6
        self.lut = self.omap.update_distances_lut(self.max_dist)
        self.pose = synth.true_pose(self.size, self.res)
        self.range_max = 30.0
        self.ranges, self.angles = synth.cast_scan(self.cells, self.origin, self.res, self.pose, beams, range_max=30.0,
                                                   seed=seed, frac_max=0.1, frac_nan=0.1)
        a = synth.converged_cloud(n - n // 2, self.pose, seed=seed + 10)
        b = synth.spread_cloud(n // 2, self.size, self.res, seed=seed + 11)
        self.samples = np.ascontiguousarray(np.concatenate([a, b]))
        self.samples[:, 3] = 1.0 / n
        self.samples[:, 3] *= np.random.default_rng(seed + 20).uniform(0.5, 1.5, n)
        self.scanner_pose = (0.1, -0.05, 0.2)
        self.map_factors = synth.MAP_FACTORS


N_GLOBAL, BEAMS_GLOBAL, MAX_BEAMS_GLOBAL = 4100, 181, 61   # one over the records-seam threshold, a last wave of 4


@pytest.fixture(scope="module")
def open_floor(orc):
    sc_ = OpenFloor(orc, N_GLOBAL, BEAMS_GLOBAL)
    # the inputs are what the test is about
    assert np.unique(sc_.lut).size >= K_TABLE_LDS_MAX
    i = np.floor((sc_.samples[:, 0] - float(sc_.origin[0])) / sc_.res + 0.5).astype(np.int64) + 64
    j = np.floor((sc_.samples[:, 1] - float(sc_.origin[1])) / sc_.res + 0.5).astype(np.int64) + 64
    inside = (i >= 0) & (i < 128) & (j >= 0) & (j < 128)
    assert 100 < (~inside).sum() < N_GLOBAL // 2
    near = sc_.lut[j[inside], i[inside]].astype(np.float64) <= sc_.map_factors[2]
    assert near.sum() > 0                                        # some in non-free space
    kept = sc_.ranges[::(BEAMS_GLOBAL - 1) // (MAX_BEAMS_GLOBAL - 1)]
    assert kept.size == MAX_BEAMS_GLOBAL
    assert np.isnan(kept).sum() > 0 and (kept >= sc_.range_max).sum() > 0
    assert (kept < sc_.range_max).sum() > MAX_BEAMS_GLOBAL // 2
    return sc_


@pytest.mark.parametrize("model", ["lf", "gompertz", "prob"])
def test_table_in_global_memory_update_sensor_matches_oracle(engine, orc, open_floor, model):
    sc_ = open_floor
    m, sc, pf, data = sc_.gpu_objects(engine, MAX_BEAMS_GLOBAL, model)
    assert sc.updateSensor(pf, data) is True
    assert engine.score_last_form() == 0
    cur = pf.getCurrentSet().samples
    st = pf.getState()
    want, want_total = oracle_update_sensor(orc, sc_, sc_.oracle_planar(MAX_BEAMS_GLOBAL, model), sc_.samples,
                                            sc_.ranges, sc_.angles, sc_.range_max)
    assert np.isfinite(want_total) and want_total > 0.0 and want.std() > 0.0
    assert np.array_equal(cur[:, :3], sc_.samples[:, :3])
    check_weights(cur[:, 3], want, N_GLOBAL * MAX_BEAMS_GLOBAL, model)
    check_total(st.total, want_total, model)


def test_table_in_global_memory_beam_skipping_matches_oracle(engine, orc, open_floor):
    """The counting pass, then pass 2 over the kept beams, both with the table in global memory.  On this floor few
    end points lie near an obstacle: within 3 m, and with a fifth of the particles agreeing, some beams are skipped
    and enough are kept (the usual 0.5 m / 0.3 keep none, and the reference then zeroes every weight)."""
    sc_ = open_floor
    kw = dict(BEAMSKIP, beam_skip_distance=3.0, beam_skip_threshold=0.2)
    m, sc, pf, data = sc_.gpu_objects(engine, MAX_BEAMS_GLOBAL, "prob", model_kw=kw)
    p = sc_.oracle_planar(MAX_BEAMS_GLOBAL, "prob", kw)
    want = sc_.samples.copy()
    want_total = sc_.oracle_apply(p, want, 1)
    unarmed = sc_.samples.copy()
    sc_.oracle_apply(p, unarmed, 0)
    assert np.isfinite(want_total) and want_total > 0.0 and not np.array_equal(want[:, 3], unarmed[:, 3])
    got = sc_.samples.copy()
    total = sc.applyModelToSampleSet(data, got, 1)
    assert engine.seam_last_plan() == (0, False)
    assert np.array_equal(got[:, :3], want[:, :3])
    check_weights(got[:, 3], want[:, 3], N_GLOBAL * MAX_BEAMS_GLOBAL, "beamskip")
    check_total(total, want_total, "beamskip")


@pytest.mark.parametrize("model", ["lf", "gompertz", "prob"])
def test_table_in_global_memory_is_declined_by_both_seam_forms(engine, orc, open_floor, model):
    """A registered, 16-byte aligned buffer of more than 4096 records would be scored in place; with this table it
    goes up, is scored and comes down again -- with the same weights."""
    sc_ = open_floor
    m, sc, pf, data = sc_.gpu_objects(engine, MAX_BEAMS_GLOBAL, model)
    want = sc_.samples.copy()
    want_total = sc_.oracle_apply(sc_.oracle_planar(MAX_BEAMS_GLOBAL, model), want, 0)
    raw = np.empty(N_GLOBAL * 4 + 2, dtype=np.float64)
    got = raw[(raw.ctypes.data % 16) // 8:][:N_GLOBAL * 4].reshape(N_GLOBAL, 4)
    assert got.ctypes.data % 16 == 0
    got[:] = sc_.samples
    engine.registerHostBuffer(got)
    try:
        total = sc.applyModelToSampleSet(data, got, 0)
        assert engine.seam_last_plan() == (0, True)
    finally:
        engine.unregisterHostBuffer(got)
    assert np.array_equal(got[:, :3], want[:, :3])
    check_weights(got[:, 3], want[:, 3], N_GLOBAL * MAX_BEAMS_GLOBAL, model)
    check_total(total, want_total, model)


# ---------------------------------------------------------------------------------------------- b. refusal, then the ring
def test_too_many_beams_are_refused_and_the_ring_goes_on(engine, orc):
    """range_count = max_beams = 4200, every range valid: 4200 beams are left after decimation, 104 more than a scan
    may hold.  The staging slot taken for that scan goes back to the ring, which the five updates behind it use up
    once round and one further."""
    import badger_amcl_amd as bpf
    sc_ = Scenario(orc, size=200, n=300, beams=61, cloud="mixture", frac_max=0.0, frac_nan=0.0)
    m, sc, pf, data = sc_.gpu_objects(engine, 4200, "lf")
    long_scan = bpf.PlanarData(np.linspace(1.0, 6.0, 4200), np.linspace(-2.0, 2.0, 4200), sc_.range_max)
    with pytest.raises(bpf.pf.BpfError) as ei:
        sc.updateSensor(pf, long_scan)
    assert ei.value.code == ERR_CAPACITY
    assert np.array_equal(pf.getCurrentSet().samples, sc_.samples)
    got = sc_.samples.copy()
    with pytest.raises(bpf.pf.BpfError) as ei:
        sc.applyModelToSampleSet(long_scan, got, 0)
    assert ei.value.code == ERR_CAPACITY
    assert np.array_equal(got, sc_.samples)
    # ... and on a registered set large enough for the in-place form, which stages the scan itself
    big = np.ascontiguousarray(np.tile(sc_.samples, (14, 1)))
    assert big.shape[0] >= 4096 and big.ctypes.data % 16 == 0
    before = big.copy()
    engine.registerHostBuffer(big)
    try:
        with pytest.raises(bpf.pf.BpfError) as ei:
            sc.applyModelToSampleSet(long_scan, big, 0)
    finally:
        engine.unregisterHostBuffer(big)
    assert ei.value.code == ERR_CAPACITY
    assert np.array_equal(big, before)

    m, sc, pf, data = sc_.gpu_objects(engine, 61, "lf")
    p = sc_.oracle_planar(61, "lf")
    for k in range(K_RING + 1):
        ranges = np.clip(sc_.ranges * (1.0 - 0.15 * k), 0.05, 29.0)
        pf.initWithSamples(sc_.samples)
        assert sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, sc_.range_max)) is True
        want, want_total = oracle_update_sensor(orc, sc_, p, sc_.samples, ranges, sc_.angles, sc_.range_max)
        check_weights(pf.getCurrentSet().samples[:, 3], want, 300 * 61, k)
        check_total(pf.getState().total, want_total, k)


# ---------------------------------------------------------------------------------------------- c. scan edge cases
@pytest.fixture(scope="module")
def one_wave_and_one(orc):
    return Scenario(orc, size=200, n=65, beams=61, cloud="mixture", frac_max=0.0, frac_nan=0.0)


def _edge_scan(sc_, case):
    if case == "all_kept":
        assert np.all(sc_.ranges < sc_.range_max)
        return sc_.ranges, sc_.range_max
    # a NaN and a range beyond range_max are dropped; 1e12 m is a valid return of 2e13 cells, more than the 2^28 from
    # which a beam is off the map for every pose: it is not staged and its off-map term joins the sum all the same
    ranges = sc_.ranges.copy()
    ranges[5] = np.nan
    ranges[17] = 3.0e12
    ranges[40] = 1.0e12
    return ranges, 2.0e12


@pytest.mark.parametrize("case", ["all_kept", "dropped_and_huge"])
@pytest.mark.parametrize("model", ["lf", "prob", "gompertz"])
def test_scan_edge_cases_on_one_wave_and_one_particle(engine, orc, one_wave_and_one, model, case):
    import badger_amcl_amd as bpf
    sc_ = one_wave_and_one
    ranges, range_max = _edge_scan(sc_, case)
    m, sc, pf, _ = sc_.gpu_objects(engine, 61, model)
    assert sc.updateSensor(pf, bpf.PlanarData(ranges, sc_.angles, range_max)) is True
    want, want_total = oracle_update_sensor(orc, sc_, sc_.oracle_planar(61, model), sc_.samples, ranges, sc_.angles,
                                            range_max)
    assert np.isfinite(want_total) and want_total > 0.0
    cur = pf.getCurrentSet().samples
    assert np.array_equal(cur[:, :3], sc_.samples[:, :3])
    check_weights(cur[:, 3], want, 65 * 61, (model, case))
    check_total(pf.getState().total, want_total, (model, case))
