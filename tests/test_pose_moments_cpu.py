"""Pose moments without a GPU: the row layout of the binding, bpf_pose_mixture_apply_moments against the numpy model
(pose_moments_ref.py) byte for byte, every refusal, the model's fixed-order sums against math.fsum, and the corridor /
corner scenarios of tests/test_gpu_pose_moments.py with the oracle's scores alone."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_moments_ref as pmr  # noqa: E402
import pose_refine_ref as prr  # noqa: E402

INVALID = 1  # BPF_ERR_INVALID_ARGUMENT
FLOOR, CAP = (0.0, 0.0, 0.0), (1e6, 1e6, 1e6)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


# ------------------------------------------------------------------------------------ the struct
def test_row_is_96_bytes_in_the_binding():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    assert C.sizeof(_lib.PoseMoments) == 96 and hpf.POSE_MOMENTS_DTYPE.itemsize == 96
    assert hpf.POSE_MOMENTS_DTYPE == pmr.MOMENTS_DTYPE
    assert [n for n, _ in _lib.PoseMoments._fields_] == list(hpf.POSE_MOMENTS_DTYPE.names)
    for name, _ in _lib.PoseMoments._fields_:
        assert hpf.POSE_MOMENTS_DTYPE.fields[name][1] == getattr(_lib.PoseMoments, name).offset, name
    assert (hpf.MOMENTS_VALID, hpf.MOMENTS_FACE_X, hpf.MOMENTS_FACE_Y, hpf.MOMENTS_FACE_THETA) == \
        (pmr.VALID, pmr.FACE_X, pmr.FACE_Y, pmr.FACE_T)


# ------------------------------------------------------------------------------------ the host function
def some_components(k, seed=1):
    rng = np.random.default_rng(seed)
    comps = np.zeros(k, dtype=pmr.COMPONENT_DTYPE)
    comps["mean"] = rng.uniform(-3.0, 3.0, (k, 3))
    comps["rotation"] = np.eye(3)
    comps["sigma"] = (0.05, 0.06, 0.02)
    comps["count"] = rng.integers(0, 100, k)
    return comps


def rows_of(covs, valid=None, seed=2):
    rng = np.random.default_rng(seed)
    covs = np.asarray(covs, dtype=np.float64).reshape(-1, 6)
    rows = np.zeros(covs.shape[0], dtype=pmr.MOMENTS_DTYPE)
    rows["cov"] = covs
    rows["mean"] = rng.uniform(-10.0, 10.0, (covs.shape[0], 3))
    rows["weight_sum"], rows["score_max"], rows["support"] = 1.0, 1.0, 5
    rows["flags"] = pmr.VALID if valid is None else np.where(valid, pmr.VALID | pmr.FACE_X, 0)
    return rows


def lib_apply(comps, src, rows, lo=FLOOR, hi=CAP, take_mean=0, n_components=None, n_rows=None, nulls=()):
    """(rc, components after the call)"""
    from badger_amcl_amd import _lib
    out = np.array(comps, dtype=_lib.MIXTURE_COMPONENT_DTYPE)
    src = np.ascontiguousarray(src, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=_lib.POSE_MOMENTS_DTYPE)
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    args = dict(comps=out.ctypes.data_as(C.POINTER(_lib.MixtureComponent)), src=src.ctypes.data_as(_ip),
                rows=rows.ctypes.data_as(C.POINTER(_lib.PoseMoments)), lo=lo.ctypes.data_as(_dp),
                hi=hi.ctypes.data_as(_dp))
    for name in nulls:
        args[name] = None
    rc = _lib.load().bpf_pose_mixture_apply_moments(
        args["comps"], out.shape[0] if n_components is None else n_components, args["src"], args["rows"],
        rows.shape[0] if n_rows is None else n_rows, args["lo"], args["hi"], int(take_mean))
    return rc, out


def sym(cov6):
    a = np.zeros((3, 3))
    for k, (u, v) in enumerate(pmr.PAIRS):
        a[u, v] = a[v, u] = cov6[k]
    return a


def cov6_of(a):
    return [a[u, v] for u, v in pmr.PAIRS]


def assert_decomposes(cov6):
    """the model's eigenpairs reproduce cov within 1e-12 of its largest entry; the rotation is orthonormal within 1e-14"""
    lam, V = pmr.jacobi(cov6)
    a = sym(cov6)
    scale = np.abs(a).max()
    assert np.abs(V @ np.diag(lam) @ V.T - a).max() <= 1e-12 * scale
    assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-14
    return lam, V


def special_covs():
    rank1 = np.outer([0.3, -0.2, 0.05], [0.3, -0.2, 0.05])
    return {"diagonal": [0.04, 0.0, 0.0, 0.01, 0.0, 0.0025],
            "zero off-diagonal": [0.04, 0.01, 0.0, 0.02, 0.003, 0.0025],
            "rank 1": cov6_of(rank1),
            "slightly indefinite": [0.01, 0.0, 0.0, -1e-18, 0.0, 0.0002]}


def random_psd(n, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        b = rng.normal(size=(3, 3)) * rng.uniform(0.01, 1.0, 3)[None, :]
        out.append(cov6_of(b @ b.T))
    return out


def test_apply_moments_equals_the_model_byte_for_byte():
    covs = random_psd(200) + list(special_covs().values())
    for c in covs:
        assert_decomposes(c)
    rows = rows_of(covs)
    k = len(covs)
    comps = some_components(k)
    src = np.random.default_rng(3).permutation(k)
    for take_mean in (0, 1):
        want = pmr.apply_moments(comps, src, rows, FLOOR, CAP, take_mean)
        rc, got = lib_apply(comps, src, rows, take_mean=take_mean)
        assert rc == 0 and want is not None
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(got["count"], comps["count"])
        if take_mean:
            assert got["mean"][:, :2].tobytes() == np.ascontiguousarray(rows["mean"][src][:, :2]).tobytes()
            assert np.all(np.abs(got["mean"][:, 2]) <= math.pi)
        else:
            assert got["mean"].tobytes() == comps["mean"].tobytes()


def test_special_matrices():
    sp = special_covs()
    lam, V = assert_decomposes(sp["diagonal"])
    assert V.tobytes() == np.eye(3).tobytes() and lam.tolist() == [0.04, 0.01, 0.0025]  # no rotation at all
    lam, V = assert_decomposes(sp["rank 1"])
    assert np.sum(np.abs(lam) > 1e-12) == 1
    rc, got = lib_apply(some_components(1), [0], rows_of([sp["slightly indefinite"]]))
    assert rc == 0 and got["sigma"][0].tolist() == [0.1, 0.0, math.sqrt(0.0002)]  # the floor 0 takes -1e-18
    # theta normalised in the fmod form
    rows = rows_of([sp["diagonal"]])
    rows["mean"][0] = (1.0, 2.0, 3.0 * math.pi + 0.25)
    rc, got = lib_apply(some_components(1), [0], rows, take_mean=1)
    assert rc == 0 and got["mean"][0].tolist() == [1.0, 2.0, pmr.normalize_angle(3.0 * math.pi + 0.25)]
    assert abs(got["mean"][0][2] - (0.25 - math.pi)) < 1e-12


def test_floor_and_cap_are_hit_exactly_by_axis():
    # eigenvectors off the axes: the x / theta plane turned by 0.6 rad.  The large eigenvalue leans on x, the tiny one
    # on theta
    c, s = math.cos(0.6), math.sin(0.6)
    Rm = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    a = Rm @ np.diag([4.0, 0.5, 1e-8]) @ Rm.T
    rows = rows_of([cov6_of(a)])
    lo, hi = (0.01, 0.02, 0.03), (1.0, 0.25, 0.5)
    want = pmr.apply_moments(some_components(1), [0], rows, lo, hi, 0)
    rc, got = lib_apply(some_components(1), [0], rows, lo, hi)
    assert rc == 0 and got.tobytes() == want.tobytes()
    lam, V = pmr.jacobi(rows["cov"][0])
    axes = [int(np.argmax(np.abs(V[:, i]))) for i in range(3)]
    assert sorted(axes) == [0, 1, 2] and abs(V[2, 0]) > 0.5
    for i in range(3):
        v = min(max(lam[i], lo[axes[i]] ** 2), hi[axes[i]] ** 2)
        assert got["sigma"][0][i] == np.sqrt(np.float64(v))
    # the large eigenvalue sits on x (cap 1.0), the tiny one on theta (floor 0.03), y's 0.5 is capped at 0.25
    assert sorted(got["sigma"][0].tolist()) == [0.03, 0.25, 1.0]
    # a tie between axes goes to the lowest
    tie = rows_of([[2.0, 1.0, 0.0, 2.0, 0.0, 0.5]])  # eigenvectors (1, 1, 0) / sqrt 2 and (1, -1, 0) / sqrt 2
    lam, V = pmr.jacobi(tie["cov"][0])
    assert abs(V[0, 0]) == abs(V[1, 0]) and abs(V[0, 1]) == abs(V[1, 1])
    rc, got = lib_apply(some_components(1), [0], tie, (0.0, 0.0, 0.0), (1.0, 100.0, 100.0))
    assert rc == 0 and got["sigma"][0].tolist() == [1.0, 1.0, math.sqrt(0.5)]  # both on x: capped at 1.0


def test_invalid_rows_leave_components_untouched():
    covs = random_psd(6, seed=9)
    valid = np.array([True, False, True, False, False, True])
    rows = rows_of(covs, valid)
    rows["cov"][1] = np.nan  # an invalid row's moments are not read
    comps = some_components(6)
    src = [0, 1, 2, 3, 4, 5]
    for take_mean in (0, 1):
        rc, got = lib_apply(comps, src, rows, take_mean=take_mean)
        assert rc == 0 and got.tobytes() == pmr.apply_moments(comps, src, rows, FLOOR, CAP, take_mean).tobytes()
        assert got[~valid].tobytes() == comps[~valid].tobytes()
        assert np.all(got["sigma"][valid] != comps["sigma"][valid])


def test_refusals():
    rows = rows_of(random_psd(4, seed=11))
    comps = some_components(3)
    src = [3, 0, 2]
    assert lib_apply(comps, src, rows)[0] == 0
    nan, inf = float("nan"), float("inf")
    bad = [dict(nulls=("comps",)), dict(nulls=("src",)), dict(nulls=("rows",)), dict(nulls=("lo",)),
           dict(nulls=("hi",)), dict(n_components=0), dict(n_components=-1), dict(n_components=1025),
           dict(n_rows=0), dict(n_rows=-3), dict(n_rows=1025), dict(n_rows=3),  # source_row 3 is outside [0, 3)
           dict(src=[0, -1, 2]), dict(src=[0, 4, 2]), dict(lo=(-0.1, 0.0, 0.0)), dict(lo=(0.0, nan, 0.0)),
           dict(lo=(0.0, 0.0, inf)), dict(hi=(1.0, -1.0, 1.0)), dict(hi=(1.0, 1.0, nan)), dict(hi=(inf, 1.0, 1.0)),
           dict(lo=(0.5, 0.0, 0.0), hi=(0.4, 1.0, 1.0))]
    for kw in bad:
        a = dict(comps=comps, src=src, rows=rows)
        a.update(kw)
        rc, got = lib_apply(a.pop("comps"), a.pop("src"), a.pop("rows"), **a)
        assert rc == INVALID, kw
        assert got.tobytes() == comps.tobytes(), kw  # nothing was written
        if not ({"nulls", "n_components", "n_rows"} & set(kw)):
            assert pmr.apply_moments(comps, kw.get("src", src), rows, kw.get("lo", FLOOR), kw.get("hi", CAP), 0) is None
    for value in (nan, inf, -inf):
        r = rows.copy()
        r["cov"][1][4] = value  # a valid row no component uses
        rc, got = lib_apply(comps, src, r)
        assert rc == INVALID and got.tobytes() == comps.tobytes()
        assert pmr.apply_moments(comps, src, r, FLOOR, CAP, 0) is None
    # the limits themselves pass, and cap == floor
    big = rows_of(random_psd(1024, seed=12))
    rc, got = lib_apply(some_components(1024), np.arange(1024)[::-1], big, (0.1, 0.1, 0.1), (0.1, 0.1, 0.1))
    assert rc == 0 and np.all(got["sigma"] == 0.1)


def test_python_method_follows_the_library():
    import badger_amcl_amd as bpf
    rows = rows_of(random_psd(5, seed=13), np.array([True, True, False, True, True]))
    comps = some_components(3)
    src = np.array([4, 2, 0], dtype=np.int32)
    before = comps.copy()
    got = bpf.mixtureApplyMoments((comps, src, np.zeros(3, dtype=np.int32)), rows, (0.01, 0.01, 0.001),
                                  (0.5, 0.5, 0.2), take_mean=True)
    assert comps.tobytes() == before.tobytes()  # a new array
    assert got.tobytes() == pmr.apply_moments(comps, src, rows, (0.01, 0.01, 0.001), (0.5, 0.5, 0.2), 1).tobytes()
    with pytest.raises(bpf.BpfError) as ei:
        bpf.mixtureApplyMoments((comps, src), rows, (0.5, 0.0, 0.0), (0.4, 1.0, 1.0))
    assert ei.value.code == INVALID


# ------------------------------------------------------------------------------------ the model's sums
@pytest.mark.parametrize("M", [3, 9, 125, 256, 257, 2025, 2048])
def test_fixed_order_sums_against_fsum(M):
    rng = np.random.default_rng(M)
    t = rng.uniform(0.0, 1.0, (10, M)) * rng.choice([-3.0, 0.0, 1.0, 1e3], (10, M))
    got = pmr.fixed_order_sum(t)
    for q in range(10):
        exact = math.fsum(t[q].tolist())
        assert abs(got[q] - exact) <= M * 2.0 ** -52 * math.fsum(np.abs(t[q]).tolist())
    # one term alone, wherever it stands, comes through bit for bit
    for at in (0, M - 1, M // 2):
        one = np.zeros(M)
        one[at] = 0.1
        assert pmr.fixed_order_sum(one) == 0.1


def test_weights_and_rows_on_hand_made_tables():
    R, A = 1, 0
    s = np.array([1.0, 2.0, np.nan, 4.0, 3.0, 2.0, 0.5, 4.0, 1.0])
    w, s_max = pmr.weights(s, 0.5)
    assert s_max == 4.0 and w.tolist() == [0.0, 0.0, 0.0, 2.0, 1.0, 0.0, 0.0, 2.0, 0.0]
    row = pmr.moments_row((1.0, 2.0, 3.0), s, R, A, 0.1, float("nan"), 0.5)
    assert row["flags"] == pmr.VALID | pmr.FACE_Y  # m = 3: a = 1, b = 0; the tie with m = 7 goes to the smaller m
    assert row["support"] == 3 and row["weight_sum"] == 5.0 and row["score_max"] == 4.0
    # offsets (a, b): m 3 = (0, -1), m 4 = (0, 0), m 7 = (1, 0)
    assert row["mean"].tolist() == [1.0 + (2.0 / 5.0) * 0.1, 2.0 + (-2.0 / 5.0) * 0.1, 3.0 + 0.0 * 0.0]
    assert row["cov"][0] == ((2.0 / 5.0 - (2.0 / 5.0) * (2.0 / 5.0)) * 0.1) * 0.1
    assert row["cov"][2] == 0.0 and row["cov"][4] == 0.0 and row["cov"][5] == 0.0  # no heading axis
    # invalid: all NaN, and a largest score of 0
    for scores, top in ((np.full(9, np.nan), np.nan), (np.zeros(9), 0.0), (np.full(9, -1.0), -1.0)):
        row = pmr.moments_row((1.0, -0.0, 3.0), scores, R, A, 0.1, 0.0, 0.0)
        assert row["flags"] == 0 and row["support"] == 0 and row["weight_sum"] == 0.0 and np.all(row["cov"] == 0.0)
        assert row["mean"].tobytes() == np.array([1.0, -0.0, 3.0]).tobytes()
        assert np.array([row["score_max"]]).tobytes() == np.array([top]).tobytes()
    # a flat surface: the lattice's uniform moments, R (R + 1) / 3 per axis in offset units
    for R, A in ((1, 0), (2, 2), (4, 12)):
        M, mc = prr.lattice(R, A)
        row = pmr.moments_row((0.0, 0.0, 0.0), np.full(M, 0.75), R, A, 1.0, 1.0, 0.5)
        assert row["flags"] == pmr.VALID and row["support"] == M and row["mean"].tolist() == [0.0, 0.0, 0.0]
        assert np.allclose(row["cov"], [R * (R + 1) / 3, 0, 0, R * (R + 1) / 3, 0, A * (A + 1) / 3], rtol=1e-14)


# ------------------------------------------------------------------------------------ the scenarios, oracle alone
def xy_principal_axis(cov):
    """(unit vector of the xy block's larger eigenvalue, larger eigenvalue, smaller eigenvalue)"""
    lam, vec = np.linalg.eigh(np.array([[cov[0], cov[1]], [cov[1], cov[3]]]))
    return vec[:, 1], lam[1], lam[0]


def test_corridor_and_corner_with_the_oracle_alone(orc):
    """What tests/test_gpu_pose_moments.py::test_corridor_and_corner compares the device with: in the corridor the xy
    block's principal axis is x, the variance along exceeds the variance across and the best point lies on the x face
    (the surface is flat along x); at the corner no face bit is set and the variance along is smaller."""
    corridor = pmr.Scene(orc, "corridor").oracle_moments()
    corner = pmr.Scene(orc, "corner").oracle_moments()
    print("corridor", corridor, "\ncorner", corner)
    axis, along, across = xy_principal_axis(corridor["cov"])
    assert corridor["flags"] & pmr.VALID and corner["flags"] & pmr.VALID
    assert abs(axis[0]) > 0.999 and abs(axis[1]) < 0.04
    assert corridor["cov"][0] > corridor["cov"][3] and along > 2.0 * across
    assert corridor["flags"] & pmr.FACE_X and not corridor["flags"] & pmr.FACE_Y
    # flat along x exactly: the uniform variance of 7 points, 4 steps^2
    assert abs(corridor["cov"][0] - 4.0 * pmr.SCENE_LATTICE[1] ** 2) <= 1e-15
    assert corner["flags"] == pmr.VALID
    assert corner["cov"][0] < corridor["cov"][0]
