"""Pose refinement without a GPU: the numpy model (pose_refine_ref.py) against hand-made cases, bpf_pose_refine_lattice
and the row layout of the binding against the model, and the condition on the inputs of
tests/test_gpu_pose_refine.py::test_trajectory_against_the_oracle, checked with the oracle alone."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_refine_ref as prr  # noqa: E402


# ------------------------------------------------------------------------------------ the model itself
@pytest.mark.parametrize("R,A", [(0, 1), (1, 0), (1, 1), (2, 2), (2, 0), (0, 3), (4, 6)])
def test_enumeration_and_centre(R, A):
    M, mc = prr.lattice(R, A)
    da, db, dt = prr.offsets(R, A)
    assert M == (2 * R + 1) ** 2 * (2 * A + 1) == da.shape[0]
    # m = (a (2R+1) + b) (2A+1) + t, a outermost and t innermost
    want = [(a - R, b - R, t - A) for a in range(2 * R + 1) for b in range(2 * R + 1) for t in range(2 * A + 1)]
    assert list(zip(da.tolist(), db.tolist(), dt.tolist())) == want
    assert want[mc] == (0, 0, 0) and want.count((0, 0, 0)) == 1
    assert mc == (M - 1) // 2


def test_steps_are_exact_halvings():
    xy, th = 0.1, math.pi / 8.0
    for level in range(16):
        d, q = prr.steps(xy, th, 1, 1, level)
        assert d * 2.0 ** level == xy and q * 2.0 ** level == th  # the mantissa is untouched
        assert d == xy / 2.0 ** level
    assert prr.steps(float("nan"), th, 0, 1, 3) == (0.0, math.ldexp(th, -3))  # a step without a radius is not read
    assert prr.steps(xy, float("inf"), 2, 0, 0) == (xy, 0.0)


def test_lattice_poses_follow_the_expressions():
    c = np.array([[0.3, -1.7, 0.1], [12.3456, 7.0, -3.0]])
    R, A, xy, th, level = 2, 1, 0.05, 0.2, 3
    p = prr.lattice_poses(c, R, A, xy, th, level)
    M, mc = prr.lattice(R, A)
    assert p.shape == (2, M, 3)
    assert p[:, mc].tobytes() == c.tobytes()
    d, q = math.ldexp(xy, -level), math.ldexp(th, -level)
    m = (3 * 5 + 0) * 3 + 2  # a = 3, b = 0, t = 2
    assert p[1, m].tolist() == [12.3456 + 1.0 * d, 7.0 + (-2.0) * d, -3.0 + 1.0 * q]


# ------------------------------------------------------------------------------------ the order rule
def test_tie_rule_on_hand_made_tables():
    M, mc = prr.lattice(1, 1)  # 27 points, centre 13
    assert (M, mc) == (27, 13)
    assert prr.choose(np.full(M, 0.25), mc) == mc  # all equal: the centre
    assert prr.choose(np.full(M, np.nan), mc) == mc  # all NaN: the centre
    s = np.full(M, 0.5)
    s[[4, mc]] = 0.75
    assert prr.choose(s, mc) == mc  # a tie between the centre and a smaller m: the centre
    s[mc] = 0.5
    s[20] = 0.75
    assert prr.choose(s, mc) == 4  # a tie without the centre: the smaller m
    s[:] = np.nan
    s[25] = -1.0
    assert prr.choose(s, mc) == 25  # NaN below every number, the centre's NaN included
    s[:] = 0.0
    s[3] = -0.0
    s[mc] = np.nan
    assert prr.choose(s, mc) == 0  # -0.0 equals +0.0


def test_replay_leaves_a_chosen_centre_bit_for_bit():
    R, A, L = 1, 1, 4
    M, mc = prr.lattice(R, A)
    poses = np.array([[-0.0, 1.0, -0.0], [0.1, 0.2, 0.3]])
    final, moved, centres = prr.replay(poses, np.full((2, L), mc), R, A, 0.1, 0.2)
    assert final.tobytes() == poses.tobytes() and moved.tolist() == [0, 0]
    trace = np.array([[mc, 0, mc, M - 1], [mc + 1, mc, mc, mc]])
    final, moved, centres = prr.replay(poses, trace, R, A, 0.1, 0.2)
    assert moved.tolist() == [2, 1]
    assert centres[:, 0].tobytes() == poses.tobytes()
    x = (-0.0 + (-1.0) * 0.05) + 1.0 * 0.0125
    assert final[0].tolist() == [x, (1.0 + (-1.0) * 0.05) + 1.0 * 0.0125, (-0.0 + (-1.0) * 0.1) + 1.0 * 0.025]
    assert final[1].tolist() == [0.1, 0.2, 0.3 + 1.0 * 0.2]


def test_decided():
    M, mc = prr.lattice(0, 1)
    assert prr.decided([1.0, 1.0 + 5e-9, 1.0], mc) == (1, True)
    assert prr.decided([1.0, 1.0 + 3e-9, 1.0], mc) == (1, False)
    assert prr.decided([2.0, 1.0, 2.0], mc) == (0, False)
    assert prr.decided([np.nan] * 3, mc) == (1, False)


# ------------------------------------------------------------------------------------ the library's host side
LATTICES = [(0, 1), (1, 0), (1, 1), (2, 2), (2, 0), (0, 3), (4, 6), (0, 1023), (22, 0), (9, 2)]


def test_lattice_call_follows_the_model():
    import badger_amcl_amd.pf as hpf
    for R, A in LATTICES:
        assert hpf.pose_refine_lattice(R, A) == prr.lattice(R, A), (R, A)
    assert prr.lattice(0, 1023)[0] == 2047 and prr.lattice(9, 2)[0] == 1805


@pytest.mark.parametrize("R,A", [(0, 0), (-1, 1), (1, -1), (0, 1024), (23, 0), (9, 3), (4, 13), (1 << 30, 1 << 30)])
def test_lattice_call_refuses(R, A):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    if R >= 0 and A >= 0 and R < 1 << 20:
        M = prr.lattice(R, A)[0]
        assert M < 2 or M > prr.MAX_POINTS
    with pytest.raises(bpf.BpfError) as ei:
        hpf.pose_refine_lattice(R, A)
    assert ei.value.code == 1


def test_lattice_call_takes_null_outputs():
    from badger_amcl_amd import _lib
    m = C.c_int(-1)
    assert _lib.load().bpf_pose_refine_lattice(1, 1, C.byref(m), None) == 0 and m.value == 27
    assert _lib.load().bpf_pose_refine_lattice(1, 1, None, None) == 0


def test_row_is_48_bytes_in_the_binding():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    assert C.sizeof(_lib.PoseRefined) == 48
    assert hpf.POSE_REFINED_DTYPE.itemsize == 48
    for name, _ in _lib.PoseRefined._fields_:
        assert hpf.POSE_REFINED_DTYPE.fields[name][1] == getattr(_lib.PoseRefined, name).offset, name


# ------------------------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("config", prr.CONFIGS)
@pytest.mark.parametrize("model", prr.MODELS)
def test_oracle_decides_at_least_half_of_the_gpu_tests_pairs(orc, model, config):
    """The condition tests/test_gpu_pose_refine.py::test_trajectory_against_the_oracle puts on its inputs, with the
    oracle alone: on the oracle's own descent from the same start poses, at least half of the (pose, level) pairs have
    a best point more than 4e-9 relative above every other."""
    trace, dec = prr.oracle_descent(orc, model, config)
    geo, poses, xy_step, theta_step = prr.planar_case(orc, model, config)
    assert 36 <= poses.shape[0] <= 44 and trace.shape == (poses.shape[0], config[2])
    M, mc = prr.lattice(*config[:2])
    assert dec.mean() >= 0.5, (model, config, dec.mean())
    assert (trace != mc).any()  # and the descent has something to do
