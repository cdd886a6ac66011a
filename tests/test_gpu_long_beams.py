"""The beam model (k_score_beam, whose ray walk takes the start cell's offset as a scalar addend) through both forms
of the walk against the oracle: the scene of long_rays.BeamScene on 1400 x 1050 and 1050 x 1400 open maps with
range_max of 999, 1001 and 1600 cells -- one launch in the integer form and two in the fp64 form, chosen by the
engine.  More than 40 % of the beams read beyond 30 m, and test_long_rays_cpu.py shows that every weight moves when
the far walls do.

Weights: 1e-9 relative with the knife-edge budget of test_gpu_parity.py; totals 1e-9 relative; poses bit-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_rays as lr  # noqa: E402
from scenario import rel_err  # noqa: E402
from test_gpu_parity import W_TOL, _knife_edge_budget  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_CAPACITY = 8
N_EVALS = lr.BEAM_N * lr.BEAM_BEAMS


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _check_weights(got, want, what):
    bad = rel_err(got, want) > W_TOL
    assert bad.sum() <= _knife_edge_budget(N_EVALS), (what, int(bad.sum()), np.flatnonzero(bad)[:10],
                                                      rel_err(got, want).max())


@pytest.mark.parametrize("cells", lr.BEAM_RANGE_CELLS)
@pytest.mark.parametrize("shape", sorted(lr.BEAM_SHAPES))
def test_beam_model_with_long_beams_matches_oracle(engine, orc, shape, cells):
    s = lr.beam_scene(orc, shape, cells)
    want, want_total = s.oracle_weights()
    assert np.isfinite(want_total) and want_total > 0.0
    m, sc, pf, data = s.gpu_objects(engine)
    # applyModelToSampleSet on a host buffer
    got = s.samples.copy()
    total = sc.applyModelToSampleSet(data, got, 0)
    assert np.array_equal(got[:, :3], want[:, :3])
    _check_weights(got[:, 3], want[:, 3], (shape, cells, "host buffer"))
    assert abs(total - want_total) <= 1e-9 * abs(want_total), (total, want_total)
    # the resident set
    assert sc.updateSensor(pf, data) is True
    cur = pf.getCurrentSet().samples
    st = pf.getState()
    assert np.array_equal(cur[:, :3], s.samples[:, :3])
    _check_weights(cur[:, 3], want[:, 3] / want_total, (shape, cells, "resident"))
    assert abs(st.total - want_total) <= 1e-9 * abs(want_total), (st.total, want_total)


def test_beam_model_at_32760_cells_is_refused_and_leaves_the_weights(engine, orc):
    """range_max = 32 760 cells: BPF_ERR_CAPACITY from both calls, the host buffer and the resident set as they
    were, and the next scan with a valid range_max scored as ever."""
    import badger_amcl_amd as bpf
    s = lr.beam_scene(orc, "wide", 999)
    m, sc, pf, data = s.gpu_objects(engine)
    too_far = lr.MAX_RAY_CELLS * s.res
    assert too_far / s.res >= lr.MAX_RAY_CELLS
    big = bpf.PlanarData(np.minimum(s.ranges, 40.0), s.angles, too_far)
    got = s.samples.copy()
    with pytest.raises(bpf.BpfError) as ei:
        sc.applyModelToSampleSet(big, got, 0)
    assert ei.value.code == ERR_CAPACITY
    assert np.array_equal(got, s.samples)
    before = pf.getCurrentSet().samples.copy()
    with pytest.raises(bpf.BpfError) as ei:
        sc.updateSensor(pf, big)
    assert ei.value.code == ERR_CAPACITY
    assert np.array_equal(pf.getCurrentSet().samples, before)
    want, want_total = s.oracle_weights()
    total = sc.applyModelToSampleSet(data, got, 0)
    _check_weights(got[:, 3], want[:, 3], "after the refusal")
    assert abs(total - want_total) <= 1e-9 * abs(want_total)
