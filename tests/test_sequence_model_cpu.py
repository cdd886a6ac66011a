"""The cache-free sequence model (tests/sequence_model.py) without a GPU: it reproduces the committed golden cycles
when it steps them operation by operation, every committed sequence is legal on it, and the committed sequences fill
the coverage matrix (cached product x invalidating operation)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import sequence_model as sm  # noqa: E402
from scenario import Scenario  # noqa: E402


@pytest.fixture(scope="module")
def world(orc):
    return sm.World(orc)


class _CycleWorld:
    """The golden cycle's inputs in the shape Model.step reads them (make_golden.run_cycle's scenario)."""

    def __init__(self, orc, sc, scans):
        self.orc, self.sc = orc, sc
        self.omaps = [sc.omap]
        self.scans = {str(i): (r, sc.angles, sc.range_max) for i, r in enumerate(scans)}

    def planar(self, cfg):
        return self.sc.oracle_planar(61, "lf")


@pytest.mark.parametrize("resampler", [0, 1])
def test_model_steps_the_golden_cycle(orc, resampler, monkeypatch):
    import make_golden as mg
    g = np.load(os.path.join(HERE, "golden", "cycle_%s.npz" % ("multinomial", "systematic")[resampler]))
    sc = Scenario(orc, size=120, n=600, beams=61, cloud="mixture", max_dist=1.0, seed=23)
    assert np.array_equal(sc.samples, g["samples"])
    monkeypatch.setattr(sm, "ODOM", mg.CYCLE_ODOM)
    monkeypatch.setattr(sm, "ODATA", mg.CYCLE_ODATA)
    m = sm.Model(_CycleWorld(orc, sc, mg.cycle_scans(sc)), 600, seed=77, alpha=mg.CYCLE_ALPHA, min_samples=50,
                 samples=sc.samples)
    for c in range(2):
        m.step(("A",))
        # glibc's sincos differs from sin / cos by an ulp for a few arguments (test_oracle_reproduces_cycle_golden)
        assert np.abs(m.set - g["moved%d" % c]).max() <= 1e-14
        m.step(("S2", "lf", str(c)))
        assert np.array_equal(m.set[:, 3], g["weights%d" % c])
        m.step(("R", resampler))
        M, leaf, bins, _, conv = (int(v) for v in g["scalars%d" % c])
        st = m.state()
        assert (st["sample_count"], st["leaf_count"], st["bin_count"], st["converged"]) == (M, leaf, bins, conv)
        assert np.array_equal(m.set, g["resampled%d" % c]) and st["rng"] == int(g["rng%d" % c])
        assert m.opf.last.w_diff == float(g["w_diff%d" % c])
    assert m.opf.last.w_diff > 0.01 and st["w_slow"] == 0.0  # the recovery branch was stepped, averages reset


def test_leaf_count_has_the_reference_lifetime(world):
    """Built at init and at resample, NOT after updateAction; counted again in the new mode by setKldCount."""
    m = sm.Model(world, 257)
    leaf0 = m.leaf
    m.step(("A",))
    assert m.leaf == leaf0 and m._count(m.set)[0] != leaf0  # (the moved poses have another tree)
    m.step(("K", sm.BINS))
    assert m.leaf == m.bins == m._count(m.set)[1]
    m.step(("K", sm.LEAVES))
    m.step(("S2", "lf", "a"))
    m.step(("R", 1))
    assert (m.leaf, m.bins) == m._count(m.set)
    m.step(("C", "small"))
    assert (m.leaf, m.bins, m.n) == (0, 0, 257 // 2 + 1) and not m.legal(("RS",))


def test_systematic_resample_needs_a_sensor_update_first(world):
    """particle_filter.cpp:438-440 leaves w_diff = NaN while w_slow = 0 and resampleSystematic (:305) converts it to an
    int: undefined in the reference, so not a legal operation of the model; the multinomial sampler only compares."""
    m = sm.Model(world, 257)
    assert not m.legal(("R", 1)) and m.legal(("R", 0))
    with pytest.raises(sm.Invalid):
        m.step(("R", 1))
    m.step(("S2", "lf", "a"))
    assert m.legal(("R", 1))
    m.step(("C", "same"))
    assert not m.legal(("R", 1))


@pytest.mark.parametrize("name", sorted(sm.SEQUENCES))
def test_committed_sequence_is_legal_on_the_model(world, name):
    spec = sm.SEQUENCES[name]
    assert spec["n"] in sm.SIZES
    m = sm.Model(world, spec["n"], pop=spec.get("pop"))
    for i, op in enumerate(spec["ops"]):
        assert m.legal(op), (i, sm.op_str(op))
        if op[0] == "R":
            assert not m.zero_total and m.set[:, 3].sum() > 0.0, (i, "resample of a zero weight total")
        m.step(op)
        assert 0 < m.n <= m.max and m.opf.samples.shape[0] == m.max, (i, sm.op_str(op))
        assert np.isfinite(m.set).all()
    assert sm.parse(sm.seq_str(spec["ops"])) == spec["ops"]


def test_sequences_reach_every_form_boundary():
    """One-block everything, k_stats_block's limit, the general statistics form, a resampled set beyond 8192."""
    assert {s["n"] for s in sm.SEQUENCES.values()} == set(sm.SIZES)


def test_a_resampled_set_stays_beyond_the_small_tail(world):
    spec = sm.SEQUENCES["spread_set_resampled_whole"]
    m = sm.Model(world, spec["n"], pop=spec.get("pop"))
    sizes = []
    for op in spec["ops"]:
        m.step(op)
        if op[0] == "R":
            sizes.append(m.n)
    assert sizes[0] > 8192


def test_coverage_matrix_is_full():
    found = sm.coverage()
    missing = [cell for cell, hits in found.items() if not hits]
    assert not missing, missing
    cells = {(p, c) for p in sm.PRODUCTS for c in sm.COLUMNS}
    assert cells == set(found) | set(sm.EXEMPT)                 # every cell is either covered or explained
    assert not set(found) & set(sm.EXEMPT)
    assert all(isinstance(r, str) and len(r) > 20 for r in sm.EXEMPT.values())
    # the matrix can be empty-handed: a sequence set without the invalidator has no instance
    assert not sm.coverage({"x": dict(n=257, ops=sm.parse("S2(lf,a) Q(device) R(0)"))})[("cdf", "A")]
    assert not sm.coverage({"x": dict(n=257, ops=sm.parse("S2(lf,a) A W R(0)"))})[("cdf", "A")]
    assert not sm.coverage({"x": dict(n=257, ops=sm.parse("I(samples) G S3 G"))})[("pending_tree", "S3")]
    assert sm.coverage({"x": dict(n=257, ops=sm.parse("S2(lf,a) P A Q(host) R(0)"))})[("cdf", "A")]
    # tile sums are left only with the fused resample off, the CDF only with it on
    seq = sm.parse("S2(lf,a) A R(0)")
    assert not sm.coverage({"x": dict(n=257, ops=seq)})[("tile_sums", "A")]
    assert sm.coverage({"x": dict(n=257, ops=seq, fused=0)})[("tile_sums", "A")]
    assert not sm.coverage({"x": dict(n=257, ops=seq, fused=0)})[("cdf", "A")]
    assert all(found[("tile_sums", c)] for c in sm.COLUMNS)


def test_the_soak_rows_own_walks_are_legal(world):
    """The walks tests/test_gpu_soaks.py runs (its seed, its case count, every size): no operation is refused by the
    model and no resample meets a zero weight total, so the soak neither skips nor aborts."""
    import re
    src = open(os.path.join(HERE, "test_gpu_soaks.py")).read()
    cases = int(re.search(r'"soak_sequences", (\d+)', src).group(1))
    seed = int(re.search(r"seed=(\d+)", src).group(1))
    walks = sm.soak_walks(seed, cases)
    assert {n for n, _ in walks} == set(sm.WALK_SIZES)
    for n, ops in walks:
        assert 8 <= len(ops) <= 14
        m = sm.Model(world, n)
        for i, op in enumerate(ops):
            assert m.legal(op), (n, i, sm.seq_str(ops))
            m.step(op)


def test_random_walks_are_legal_and_replayable(world):
    rng = np.random.default_rng(5)
    kinds = set()
    for _ in range(40):
        ops = sm.random_walk(rng, 257)
        assert 8 <= len(ops) <= 14 and sm.parse(sm.seq_str(ops)) == ops
        m = sm.Model(world, 257)
        for op in ops:
            assert m.legal(op)
            m.step(op)
        kinds |= {op[0] for op in ops}
    assert kinds >= {"S2", "S3", "F2", "F3", "R", "A", "K", "W", "SN", "RS", "I", "C", "M", "Q", "P", "G"}
