"""The 3-D worlds of tests/cloud_geometry.py on the CPU, with the oracle only: each world has the property it was made
for, the clouds and particle sets reach what the GPU tests rely on, and the two voxel forms of the scoring kernel
(kernels_cloud.hpp) are restated and held against the reference's division."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_geometry as cg  # noqa: E402

NAMES = sorted(cg.GEOMETRIES)
INEXACT_WORLDS = ["V2", "V3", "V5"]


# ------------------------------------------------------------------------------------------------ the table
def test_each_world_has_the_property_it_is_for():
    size = {n: np.array(g[1]) - np.array(g[0]) + 1 for n, g in cg.GEOMETRIES.items()}
    mn = {n: g[0] for n, g in cg.GEOMETRIES.items()}
    # V1: whole tiles both ways (the far border ring is the last column / row of the last tile), min_x > 0
    assert (size["V1"][0] + 2) % 8 == 0 and (size["V1"][1] + 2) % 8 == 0 and mn["V1"][0] > 0
    # V2: one cell into a third tile, z needs more than a byte, min_y > 0
    assert (size["V2"][0] + 2) % 8 == 1 and (size["V2"][0] + 2) // 8 == 2 and size["V2"][2] > 255 and mn["V2"][1] > 0
    # V3: bounds 10^4 cells from the origin with either sign, no span holds cell 0
    g = cg.GEOMETRIES["V3"]
    assert g[0][0] >= 10000 and g[1][1] <= -10000 and all(lo > 0 or hi < 0 for lo, hi in zip(g[0], g[1]))
    assert all(abs(np.spacing(np.float32(g[0][a] * g[2]))) > 1.2e-4 for a in (0, 1))   # float ulps out there
    # V4: narrower than a tile, one z plane
    assert size["V4"][0] < 8 and size["V4"][2] == 1
    # V5: the room every other cloud test uses
    from badger_amcl_amd import synth
    occ = synth.box_room_voxels()
    assert tuple(occ.min(axis=0) - 3) == cg.GEOMETRIES["V5"][0] and tuple(occ.max(axis=0) + 3) == cg.GEOMETRIES["V5"][1]
    # no plane is too large for the dense volume, so BPF_OPT_CLOUD_DENSE decides the layout on all five
    for n in NAMES:
        ntx, nty = (size[n][0] + 2 + 7) // 8, (size[n][1] + 2 + 7) // 8
        assert ntx * nty * 64 < 1 << 24


def test_exact_reciprocal_rule_classifies_the_resolutions():
    """score_cloud's host rule restated (cloud_geometry.exact_rinv): the table's resolutions and the two lists of the
    rounding check fall on the side they are listed under."""
    for n, (_, _, res, exact) in cg.GEOMETRIES.items():
        assert cg.exact_rinv(res) is exact, n
    assert all(cg.exact_rinv(r) for r in cg.EXACT_RESOLUTIONS)
    assert not any(cg.exact_rinv(r) for r in cg.INEXACT_RESOLUTIONS)


# ------------------------------------------------------------------------------------------------ voxel rounding
def _rounding_inputs(res, seed):
    """Float coordinates: (k + 0.5) res stepped by -2 .. +2 float ulps for |k| <= 4000, and as many anywhere in that
    range."""
    faces = cg.face_floats(res, -4000, 4000).reshape(-1)
    rng = np.random.default_rng(seed)
    anywhere = rng.uniform(-4000.5 * res, 4000.5 * res, faces.size).astype(np.float32)
    return np.concatenate([faces, anywhere])


def test_voxel_forms_against_true_division():
    """The kernel's two quotient forms restated with libm's fma against floor(v / res + 0.5) in double, 80 010 floats
    per resolution, half of them within two float ulps of a voxel face:

      corrected reciprocal (voxel_of) on 0.03, 0.06, 0.07, 0.15, 0.3, 0.075:     0 voxels differ
      exact form (voxel_of_exact) on the eleven resolutions it is chosen for:    0 voxels differ
      exact form applied to 0.03 / 0.06 / 0.07 (a wrong dispatch):               67 / 67 / 65 differ, all of them among
                                                                                 the 40 005 face floats (0.17 %)

    so a launch that takes the exact form at an inexact resolution shows in a face cloud, and a right launch needs no
    allowance there."""
    for k, res in enumerate(cg.INEXACT_RESOLUTIONS):
        v = _rounding_inputs(res, 100 + k)
        want = cg.voxel_reference(v, res)
        assert np.array_equal(np.array(cg.voxel_corrected_form(v, res)), want), res
    for k, res in enumerate(cg.EXACT_RESOLUTIONS):
        v = _rounding_inputs(res, 200 + k)
        assert np.array_equal(np.array(cg.voxel_exact_form(v, res)), cg.voxel_reference(v, res)), res
    wrong = {}
    for k, res in enumerate((0.03, 0.06, 0.07)):
        v = _rounding_inputs(res, 300 + k)
        d = np.array(cg.voxel_exact_form(v, res)) != cg.voxel_reference(v, res)
        wrong[res] = (int(d[: d.size // 2].sum()), int(d[d.size // 2:].sum()))
    print("exact form applied to inexact resolutions (on faces, elsewhere):", wrong)
    assert all(on_face > 0 for on_face, _ in wrong.values()), wrong


def test_voxel_reference_is_the_oracles_world_to_map(orc):
    s = cg.scenario(orc, "V3")
    v = cg.face_floats(s.res, 19990, 20070).reshape(-1)
    want = cg.voxel_reference(v, s.res)
    for x, c in zip(v[::7], want[::7]):
        assert s.lut.world_to_map([float(x), 0.0, float(x)])[0] == c == s.lut.world_to_map([0.0, 0.0, float(x)])[2]


# ------------------------------------------------------------------------------------------------ clouds, particles
@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_inputs_reach_what_the_gpu_tests_rely_on(orc, name, pitched):
    s = cg.scenario(orc, name)
    assert s.pts[pitched].shape == (5000, 3) and s.pts[pitched].dtype == np.float32
    assert 5000 > 2 * 2048 and 5000 % 256 != 0          # more than two LDS chunks, a ragged last one
    assert s.samples.shape == (300, 4) and (~np.isfinite(s.samples[:, :3])).any(axis=1).sum() == 3
    finite = np.isfinite(s.samples[:, 2])
    assert s.samples[finite, 2].min() < -3.0 and s.samples[finite, 2].max() > 3.0 and np.abs(s.samples[finite, 2]).max() <= np.pi
    st = s.statistics(pitched=pitched)
    assert min(st["off"]) > 0, st                       # points leave the map on each of its six sides
    assert st["seeing"] > 0.9, st                       # ... and most particles see the map
    assert 0.30 <= st["on"] <= 0.95, st
    assert st["sensitive"] >= 0.2, st                   # an x / y exchange or a z slip reads another ratio
    # particles stand on either side of all four edges
    on = s.robot_on_map(s.samples[np.isfinite(s.samples[:, :3]).all(axis=1)])
    assert 0.3 < on.mean() < 0.95
    # BORDER is eligible: the LUT leaves two of the 256 ratios free; the appended form leaves none
    assert len(np.unique(s.lut.distance_ratios)) <= 254
    assert len(np.unique(s.full_ratios())) == 256
    # obstacles: no mirror or transposition symmetry
    vol = s.volume()
    k = min(vol.shape[0], vol.shape[1])
    assert not np.array_equal(vol[:k, :k], vol[:k, :k].transpose(1, 0, 2))
    assert not np.array_equal(vol, vol[::-1]) and not np.array_equal(vol, vol[:, ::-1])


@pytest.mark.parametrize("name", NAMES)
def test_helper_cells_are_the_oracles(orc, name):
    """The numpy restatement behind the statistics against the oracle's own conversion, at yaw 0 where libm and numpy
    cannot differ, through both mountings; and the oracle's weights for the whole set are finite and discriminate."""
    s = cg.scenario(orc, name)
    one = np.array([[s.pose[0], s.pose[1], 0.0, 1.0]])
    for pitched in (False, True):
        w = s.world_points(one, pitched=pitched)[0].astype(np.float64)
        c = s.cells(one, pitched=pitched)[0] + s.mn
        for q in range(0, 5000, 211):
            assert tuple(s.lut.world_to_map(w[q])) == tuple(c[q])
        want = s.samples.copy()
        total = orc.cloud_apply(s.oracle_cloud("plain", pitched), s.lut, want, s.pts[pitched])
        assert np.isfinite(want[:, 3]).all() and np.isfinite(total) and total > 0
        assert len(np.unique(np.round(want[:, 3] / s.samples[:, 3], 9))) > 30


# ------------------------------------------------------------------------------------------------ faces
@pytest.mark.parametrize("name", NAMES)
def test_face_clouds_stand_on_faces_with_different_neighbours(orc, name):
    s = cg.scenario(orc, name)
    differ, total = 0, 0
    vol = s.volume()
    for axis in range(3):
        pts, d = s.face_cloud(axis)
        n_faces = int(s.size[axis]) + 10
        assert pts.shape == (5 * n_faces, 3) and pts.dtype == np.float32
        c = cg.voxel_reference(pts, s.res)
        # the five points of a face fall on its two sides; the on / off-map faces at both ends are among them
        for f in range(n_faces):
            k = int(s.mn[axis]) - 5 + f
            assert set(c[5 * f:5 * f + 5, axis]) <= {k, k + 1}
        assert c[:, axis].min() < s.mn[axis] - 3 and c[:, axis].max() > s.mx[axis] + 3
        both = [len(set(c[5 * f:5 * f + 5, axis])) == 2 for f in range(n_faces)]
        assert np.mean(both) > 0.9
        # the other two coordinates: cell centres inside the map
        others = [a for a in range(3) if a != axis]
        for a in others:
            assert (c[:, a] >= s.mn[a]).all() and (c[:, a] <= s.mx[a]).all()
            assert np.allclose(pts[:, a], c[:, a] * s.res, rtol=1e-6, atol=0)
        # `differs` is what it says, read back from the volume
        for f in range(n_faces):
            k = int(s.mn[axis]) - 5 + f
            cell = c[5 * f].copy()
            r = []
            for kk in (k, k + 1):
                cell[axis] = kk
                rel = cell - s.mn
                inside = (rel >= 0).all() and (rel < s.size).all()
                r.append(int(vol[rel[1], rel[0], rel[2]]) if inside else 255)
            assert (r[0] != r[1]) == bool(d[5 * f]), (axis, k)
        differ += int(d.sum())
        total += d.size
        assert d.sum() >= 10       # every axis has at least its two on / off-map faces
    assert differ >= 0.5 * total, (differ, total)


@pytest.mark.parametrize("name", INEXACT_WORLDS)
def test_face_clouds_tell_a_wrong_dispatch(orc, name):
    """The exact form as the kernel's loop states it (voxel1_exact: the lower bound folded into the addend) applied to
    these worlds' resolutions moves face points into the neighbouring voxel where that voxel holds another ratio:
    three points of V2's z faces and one of V5's x faces; none on V3, whose floats near 1.4 km are too coarse to come
    that close to a face.  So with EXACT_RINV forced the face-cloud weights change on V2 and V5, and on V3 only the
    reported form tells.  The corrected form moves none."""
    s = cg.scenario(orc, name)
    seen = {}
    for axis in range(3):
        pts, d = s.face_cloud(axis)
        v, mn, size = pts[:, axis], int(s.mn[axis]), int(s.size[axis])
        want = cg.voxel_reference(v, s.res) - mn + 1
        assert np.array_equal(np.array(cg.voxel_corrected_form(v, s.res)) - mn + 1, want)
        got = cg.voxel1_exact_form(v, s.res, mn)
        on_map = [np.where((c >= 1) & (c <= size), c, 0) for c in (want, got)]   # off the map is one class
        seen["xyz"[axis]] = int(((on_map[0] != on_map[1]) & d).sum())
    print(name, "face points the forced exact form scores under another ratio:", seen)
    assert seen == {"V2": dict(x=0, y=0, z=3), "V3": dict(x=0, y=0, z=0), "V5": dict(x=1, y=0, z=0)}[name]


def test_identity_mountings_leave_the_points_alone():
    """Quaternion (0, 0, 0, 1) gives the float identity exactly; (1e-30, 0, 0, 1), which selects the general kernel,
    differs from it by +-2e-30 in two entries, which vanish in the float sums of any coordinate that is not 0."""
    m = cg.quat_matrix_f32((0.0, 0.0, 0.0, 1.0))
    assert np.array_equal(m, np.eye(3, dtype=np.float32).reshape(-1))
    g = cg.quat_matrix_f32((1e-30, 0.0, 0.0, 1.0))
    off = g - m
    assert np.count_nonzero(off) == 2 and np.abs(off).max() < 3e-30 and g[0] == g[4] == g[8] == 1.0


@pytest.mark.parametrize("name", NAMES)
def test_general_kernel_identity_keeps_the_face_voxels(orc, name):
    s = cg.scenario(orc, name)
    one = np.array([[0.0, 0.0, 0.0, 1.0]])
    for axis in range(3):
        pts, _ = s.face_cloud(axis)
        for quat in ((0.0, 0.0, 0.0, 1.0), (1e-30, 0.0, 0.0, 1.0)):
            w = s.world_points(one, pts, tf_xyz=(0.0, 0.0, 0.0), tf_quat=quat)[0]
            assert np.array_equal(cg.voxel_reference(w, s.res), cg.voxel_reference(pts, s.res))
            if quat[0] == 0.0:
                assert np.array_equal(w, pts)


@pytest.mark.parametrize("name", NAMES)
def test_robot_face_samples_stand_on_both_sides(orc, name):
    s = cg.scenario(orc, name)
    r = s.robot_face_samples()
    assert r.shape == (40, 4)
    on = s.robot_on_map(r)
    assert 10 <= on.sum() <= 30
    # each on / off-map face (k = min - 1 and k = max, either axis) has particles on both of its sides
    for block in (0, 2, 4, 6):
        assert len(set(on[5 * block:5 * block + 5])) == 2, block
    # the oracle's own conversion says the same
    for p, o in zip(r, on):
        c = s.lut.world_to_map([p[0], p[1], 0.0])
        assert o == bool(s.mn[0] <= c[0] <= s.mx[0] and s.mn[1] <= c[1] <= s.mx[1])
