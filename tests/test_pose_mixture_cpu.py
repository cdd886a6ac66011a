"""From hit rows to mixture components without a GPU: bpf_pose_mixture_from_hits against the numpy model
(pose_mixture_ref.py) byte for byte on hand-made tables, the counts' sum on random tables, every refusal, the
struct's size in the binding, and the condition on the inputs of
tests/test_gpu_mixture_init.py::test_search_refine_seed_track_planar, checked with the oracle alone."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pose_mixture_ref as pmr  # noqa: E402

INVALID = 1  # BPF_ERR_INVALID_ARGUMENT
SIGMA = (0.05, 0.05, 0.02)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def lib_call(poses, scores, total, xy, th, cap, sigma=SIGMA, n_rows=None, nulls=()):
    """(rc, components, source_row, merged) of the library on plain arrays; nulls: argument names passed as NULL."""
    from badger_amcl_amd import _lib
    L = _lib.load()
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    g = np.ascontiguousarray(sigma, dtype=np.float64)
    room = max(1, min(int(cap), 1024))
    out = np.zeros(room, dtype=_lib.MIXTURE_COMPONENT_DTYPE)
    src = np.full(room, -7, dtype=np.int32)
    mrg = np.full(room, -7, dtype=np.int32)
    n = C.c_int(-7)
    args = dict(poses=p.ctypes.data_as(_dp), scores=s.ctypes.data_as(_dp), sigma=g.ctypes.data_as(_dp),
                out=out.ctypes.data_as(C.POINTER(_lib.MixtureComponent)), src=src.ctypes.data_as(_ip),
                mrg=mrg.ctypes.data_as(_ip), n=C.byref(n))
    for name in nulls:
        args[name] = None
    rc = L.bpf_pose_mixture_from_hits(args["poses"], args["scores"], p.shape[0] if n_rows is None else n_rows,
                                      int(total), float(xy), float(th), int(cap), args["sigma"], args["out"],
                                      args["src"], args["mrg"], args["n"])
    k = max(n.value, 0)
    return rc, out[:k], src[:k], mrg[:k]


def assert_equals_model(poses, scores, total, xy, th, cap, sigma=SIGMA):
    want = pmr.mixture_from_hits(poses, scores, total, xy, th, cap, sigma)
    rc, comps, src, mrg = lib_call(poses, scores, total, xy, th, cap, sigma)
    assert want is not None and rc == 0
    assert comps.tobytes() == want[0].tobytes()
    assert src.tobytes() == want[1].tobytes() and mrg.tobytes() == want[2].tobytes()
    assert int(comps["count"].sum()) == total and np.all(comps["count"] >= 0)
    return comps, src, mrg


def test_struct_is_128_bytes_in_the_binding():
    from badger_amcl_amd import _lib
    import badger_amcl_amd.pf as hpf
    assert C.sizeof(_lib.MixtureComponent) == 128 and _lib.MIXTURE_COMPONENT_DTYPE.itemsize == 128
    assert hpf.MIXTURE_COMPONENT_DTYPE == pmr.COMPONENT_DTYPE
    for name, kind in _lib.MixtureComponent._fields_:
        assert getattr(_lib.MixtureComponent, name).offset == _lib.MIXTURE_COMPONENT_DTYPE.fields[name][1]


def test_ties_in_score_go_by_row():
    poses = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]
    comps, src, _ = assert_equals_model(poses, [0.5, 0.75, 0.5, 0.75], 10, 0.1, 0.1, 8)
    assert src.tolist() == [1, 3, 0, 2]
    assert comps["count"].tolist() == [3, 3, 2, 2]


def test_on_the_merge_distance_and_one_ulp_outside():
    d = 0.25
    # the angle test goes through normalize_angle, whose (a + pi) - pi rounds at pi's scale: the distance that a
    # difference of exactly 0.125 lies ON is normalize_angle(0.125), and its next neighbour is 4 ulp of 0.125 away
    t = pmr.normalize_angle(0.125)
    thetas = [0.625 + q * 2.0 ** -53 for q in range(1, 64)]
    outside = next(v for v in thetas if pmr.normalize_angle(v - 0.5) > t)
    poses = [[1.0, 2.0, 0.5],
             [1.0 + d, 2.0, 0.5],                      # exactly on the distance in x: merged
             [1.0, 2.0 - d, 0.5],                      # exactly on it in y: merged
             [1.0, 2.0, 0.625],                        # exactly on it in theta: merged
             [np.nextafter(1.0 + d, 2.0), 2.0, 0.5],   # one ulp outside in x: kept
             [1.0, np.nextafter(2.0 - d, 0.0), 0.5],   # one ulp outside in y: kept
             [1.0, 2.0, outside]]                      # the first theta whose normalised difference is larger: kept
    assert (1.0 + d) - 1.0 == d and 2.0 - (2.0 - d) == d and pmr.normalize_angle(0.625 - 0.5) == t
    comps, src, mrg = assert_equals_model(poses, [7, 6, 5, 4, 3, 2, 1], 100, d, t, 8)
    assert src.tolist() == [0, 4, 5, 6] and mrg.tolist() == [3, 0, 0, 0]


def test_theta_differing_by_whole_turns_is_merged_and_the_mean_is_normalised():
    two_pi = 2.0 * math.pi
    poses = [[0.0, 0.0, 0.3 + 3 * two_pi], [0.0, 0.0, 0.3], [0.0, 0.0, 0.3 - 2 * two_pi], [0.0, 0.0, 0.3 + math.pi]]
    comps, src, mrg = assert_equals_model(poses, [4, 3, 2, 1], 17, 0.0, 1e-9, 8)
    assert src.tolist() == [0, 3] and mrg.tolist() == [2, 0]
    assert comps["mean"][0, 2] == pmr.normalize_angle(0.3 + 3 * two_pi) and abs(comps["mean"][0, 2] - 0.3) < 1e-12
    assert np.all(np.abs(comps["mean"][:, 2]) <= math.pi)


def test_unusable_rows_are_dropped():
    nan, inf = float("nan"), float("inf")
    poses = [[0, 0, 0], [1, 1, 0], [2, 2, 0], [3, 3, 0], [4, 4, 0], [nan, 5, 0], [6, inf, 0], [7, 7, -inf], [8, 8, 0]]
    scores = [nan, inf, -inf, 0.0, -1.0, 1.0, 1.0, 1.0, 0.5]
    comps, src, mrg = assert_equals_model(poses, scores, 9, 0.1, 0.1, 8)
    assert src.tolist() == [8] and mrg.tolist() == [0] and comps["count"].tolist() == [9]


def test_max_components_reached():
    poses = [[float(i), 0.0, 0.0] for i in range(10)]
    poses.append([0.01, 0.0, 0.0])  # near the best row: still merged into it after the cap is reached
    scores = [10 - i for i in range(10)] + [0.05]
    comps, src, mrg = assert_equals_model(poses, scores, 1000, 0.1, 0.1, 3)
    assert src.tolist() == [0, 1, 2] and mrg.tolist() == [1, 0, 0]


def test_one_row_only():
    comps, src, mrg = assert_equals_model([[1.5, -2.5, 4.0]], [1e-300], 4096, 0.1, 0.1, 1024)
    assert comps["count"].tolist() == [4096] and comps["mean"][0, :2].tolist() == [1.5, -2.5]
    assert np.array_equal(comps["rotation"][0], np.eye(3)) and comps["sigma"][0].tolist() == list(SIGMA)
    assert comps["reserved"].tolist() == [0]


def test_fewer_samples_than_components():
    poses = [[float(i), 0.0, 0.0] for i in range(7)]
    comps, _, _ = assert_equals_model(poses, [7, 6, 5, 4, 3, 2, 1], 3, 0.1, 0.1, 7)
    assert comps.shape[0] == 7 and (comps["count"] == 0).sum() >= 4


@pytest.mark.parametrize("k,total", [(3, 10), (7, 100), (64, 1000), (1024, 5000), (6, 5)])
def test_equal_weights_that_do_not_divide(k, total):
    poses = [[float(i), 0.0, 0.0] for i in range(k)]
    comps, _, _ = assert_equals_model(poses, [0.1] * k, total, 0.1, 0.1, k)
    c = comps["count"]
    assert c.max() - c.min() == 1 and np.all(np.diff(c) <= 0)  # the remainder goes to the first components


def test_random_tables_sum_and_equal_the_model():
    rng = np.random.default_rng(20240611)
    for case in range(1000):
        n = int(rng.integers(1, 41)) if case % 250 else 1024
        poses = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-20, 20, n)], axis=1)
        scores = rng.uniform(0.0, 1.0, n) ** int(rng.integers(1, 9))
        if case % 3 == 0:
            scores = np.round(scores, 1)  # ties and zeros
        if case % 7 == 0:
            scores[rng.integers(0, n)] = np.nan
        if not np.any(np.isfinite(scores) & (scores > 0)):
            scores[0] = 1.0
        total = int(rng.integers(1, 100000))
        cap = int(rng.integers(1, 1025))
        assert_equals_model(poses, scores, total, float(rng.uniform(0, 2)), float(rng.uniform(0, 1)), cap)


def test_refusals():
    poses, scores = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [1.0, 2.0]
    good = dict(total=10, xy=0.1, th=0.1, cap=4)
    assert lib_call(poses, scores, **good)[0] == 0
    nan, inf = float("nan"), float("inf")
    bad = [dict(total=0), dict(total=-5), dict(cap=0), dict(cap=1025), dict(cap=-1), dict(n_rows=0), dict(n_rows=-1),
           dict(n_rows=1025), dict(xy=-1e-9), dict(xy=nan), dict(xy=inf), dict(th=-0.1), dict(th=nan), dict(th=inf),
           dict(sigma=(-0.1, 0, 0)), dict(sigma=(0, nan, 0)), dict(sigma=(0, 0, inf)),
           dict(nulls=("poses",)), dict(nulls=("scores",)), dict(nulls=("sigma",)), dict(nulls=("out",)),
           dict(nulls=("n",))]
    for kw in bad:
        rc, comps, _, _ = lib_call(poses, scores, **dict(good, **kw))
        assert rc == INVALID and comps.shape[0] == 0, kw
        if "nulls" not in kw and "n_rows" not in kw:
            assert pmr.mixture_from_hits(poses, scores, *[dict(good, **kw)[a] for a in ("total", "xy", "th", "cap")],
                                         kw.get("sigma", SIGMA)) is None, kw
    # no usable row
    assert lib_call(poses, [0.0, nan], **good)[0] == INVALID
    assert pmr.mixture_from_hits(poses, [0.0, nan], 10, 0.1, 0.1, 4, SIGMA) is None
    # the two optional outputs may be NULL
    rc, comps, src, mrg = lib_call(poses, scores, nulls=("src", "mrg"), **good)
    assert rc == 0 and comps.shape[0] == 2 and src.tolist() == [-7, -7] and mrg.tolist() == [-7, -7]
    # sigma 0 is allowed
    assert lib_call(poses, scores, sigma=(0, 0, 0), **good)[0] == 0


def test_python_wrapper_takes_hits_and_refined_rows():
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    hits = np.zeros(3, dtype=hpf.POSE_HIT_DTYPE)
    hits["pose"] = [[1, 2, 7.0], [1.01, 2, 7.0], [4, 4, 0]]
    hits["score"] = [0.5, 0.9, 0.3]
    rows = np.zeros(3, dtype=hpf.POSE_REFINED_DTYPE)
    rows["pose"], rows["score"] = hits["pose"], hits["score"]
    want = pmr.mixture_from_hits(hits["pose"], hits["score"], 1000, 0.05, 0.1, 16, SIGMA)
    for table in (hits, rows):
        comps, src, mrg = bpf.mixtureFromHits(table, 1000, 0.05, 0.1, 16, SIGMA)
        assert comps.dtype == hpf.MIXTURE_COMPONENT_DTYPE
        assert comps.tobytes() == want[0].tobytes() and src.tolist() == [1, 2] and mrg.tolist() == [1, 0]
    with pytest.raises(bpf.BpfError):
        bpf.mixtureFromHits(hits, 0, 0.05, 0.1, 16, SIGMA)


# ------------------------------------------------------------------------------------ the end-to-end test's inputs
def test_oracle_alone_localises_from_the_mixture(orc):
    """The condition on the inputs of test_search_refine_seed_track_planar, so that a GPU failure cannot hide behind a
    bad scenario.  The test's own chain with the oracle's scores in place of the device's: every candidate of the
    search scored, the best refined by the lattice descent (the poses around the true pose, and the decoys the map's
    symmetries put among them), the components of pose_mixture_ref, seeded through K successive
    orc_pf_init_with_gaussian calls sharing the rng, then the test's number of sensor-update + resample cycles; the
    oracle's max-weight pose must lie within one cell in x and y and one search heading step of the true pose."""
    import mixture_oracle as mo
    sc_ = mo.e2e_scenario(orc)
    truth = np.asarray(sc_.pose, dtype=np.float64)
    poses, scores = mo.oracle_search_refine(sc_)
    xy, th = mo.e2e_merge(sc_.res)
    comps, src, merged = pmr.mixture_from_hits(poses, scores, mo.E2E_N, xy, th, mo.E2E_CAP, mo.E2E_SIGMA)
    far = np.hypot(comps["mean"][:, 0] - truth[0], comps["mean"][:, 1] - truth[1]) > 1.0
    print("components", comps["mean"].round(3).tolist(), comps["count"].tolist())
    assert comps.shape[0] == mo.E2E_CAP and np.any(far) and not np.all(far)  # decoys are among the components
    opf = orc.ParticleFilter(100, mo.E2E_N, 0.0, 0.0, 85.0, seed=mo.E2E_SEED)
    mo.oracle_init_with_mixture(orc, opf, comps)
    mo.oracle_cycles(sc_, opf, mo.E2E_CYCLES)
    w, pose = mo.oracle_max_weight_pose(orc, opf.samples[:opf.sample_count])
    print("oracle max-weight pose", pose, "truth", truth, "weight", w, "samples", opf.sample_count)
    assert mo.within_e2e_bound(pose, truth, sc_.res)


def test_oracle_alone_localises_from_the_mixture_cloud(orc):
    """The same condition on the inputs of test_search_refine_seed_track_cloud: the room, cloud and model of
    tests/test_gpu_pose_search_cloud.py at its smallest shape, the chain with the oracle's cloud scores alone."""
    import mixture_oracle as mo
    scene = mo.CloudScene(orc)
    H = mo.E2E_CLOUD_HEADINGS
    poses, scores = mo.oracle_search_refine_cloud(scene)
    xy, th = mo.e2e_merge(scene.res, H)
    comps, src, merged = pmr.mixture_from_hits(poses, scores, mo.E2E_N, xy, th, mo.E2E_CAP, mo.E2E_SIGMA)
    turned = np.abs([pmr.normalize_angle(t - scene.truth[2]) for t in comps["mean"][:, 2]]) > 2.0 * math.pi / H
    print("components", comps["mean"].round(3).tolist(), comps["count"].tolist())
    assert comps.shape[0] == mo.E2E_CAP and np.any(turned) and not np.all(turned)  # decoys at other headings
    opf = orc.ParticleFilter(100, mo.E2E_N, 0.0, 0.0, 85.0, seed=mo.E2E_SEED)
    mo.oracle_init_with_mixture(orc, opf, comps)
    mo.oracle_cycles_cloud(scene, opf, mo.E2E_CLOUD_CYCLES)
    w, pose = mo.oracle_max_weight_pose(orc, opf.samples[:opf.sample_count])
    print("oracle max-weight pose", pose, "truth", scene.truth, "weight", w, "samples", opf.sample_count)
    assert mo.within_e2e_bound(pose, scene.truth, scene.res, H)
