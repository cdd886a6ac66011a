"""tests/far_frames.py holds its claims, from the oracle alone (no GPU): the frames sit where they say relative to the
range of the fixed-point sums, the key-edge clouds sit where they say relative to kld_pack's range, and the exact
reference is one the oracle's own serial evaluation meets within the bound the GPU tests use against it."""
from fractions import Fraction

import numpy as np
import pytest

import far_frames as ff

CLOUDS = list(ff.CLOUDS)


def _set_sums(name, frame, form):
    s = ff.cloud(name, frame, form)
    t = ff.terms(s)
    return s, t, [ff.exact_sum(t[k]) for k in range(9)]


@pytest.mark.parametrize("form", ff.WEIGHTS)
@pytest.mark.parametrize("name", CLOUDS)
def test_under_and_over_lie_on_their_sides_of_two_to_the_31(name, form):
    """The exact sum of w x^2: under in (0.99 * 2^31, 2^31), over_xx in (2^31, 1.01 * 2^31); every other sum of both
    frames is in range, so that the xx sum alone decides."""
    lo, hi = Fraction(99, 100) * ff.TWO31, Fraction(101, 100) * ff.TWO31
    for frame, (a, b) in (("under", (lo, ff.TWO31)), ("over_xx", (ff.TWO31, hi))):
        s, t, sums = _set_sums(name, frame, form)
        assert a < sums[5] < b, (frame, float(sums[5]))
        for k in (0, 1, 2, 3, 4, 6, 7, 8):
            assert abs(sums[k]) < Fraction(1, 2) * ff.TWO31, (frame, k, float(sums[k]))
        assert np.all(np.abs(t) < ff.TERM_GUARD)  # no single term trips the per-term guard


@pytest.mark.parametrize("name", CLOUDS)
def test_over_xy_passes_two_to_the_31_in_the_cross_term_only_and_downwards(name):
    s, t, sums = _set_sums(name, "over_xy", "normalised")
    assert sums[6] < -ff.TWO31 and sums[7] < -ff.TWO31
    assert -Fraction(2) * ff.TWO31 < sums[6]
    # (the squares do pass 2^31 at (-70 000, 52 000): 4.9e9 and 2.7e9 -- "only the cross term" cannot hold for this
    # offset, whose |x y| = 3.64e9 lies between them; what the frame adds is a NEGATIVE sum beyond the range)
    assert sums[5] > ff.TWO31 and sums[8] > ff.TWO31
    assert np.all(np.abs(t) < ff.TERM_GUARD)


@pytest.mark.parametrize("name", CLOUDS)
def test_per_term_guard_fires_in_the_last_frame_only(name):
    """Normalised weights: every term of every frame but `guard` is below 2e9; in `guard` w y^2 is not.  The 2 000
    sample cloud is the exception the arithmetic forces: w y^2 = 4e12 / 2000 = 2e9 at y = -2e6, so there `far` trips
    the per-term guard as well (a second case of it, on the one-block path)."""
    for frame in ff.OFFSETS:
        s, t, sums = _set_sums(name, frame, "normalised")
        if frame == "guard" or (frame == "far" and name == "blob2000"):
            assert np.any(np.abs(t[8]) >= ff.TERM_GUARD)
            assert np.all(np.abs(t[:5]) < ff.TERM_GUARD)
        else:
            assert np.all(np.abs(t) < ff.TERM_GUARD), frame


def test_the_path_thresholds_are_on_both_sides():
    """2 000 samples take the one-block kernel (<= 4096), 5 000 and 6 000 the multi-launch / distributed forms."""
    assert ff.CLOUDS["blob2000"] <= 4096 < ff.CLOUDS["blobs5000"] and ff.CLOUDS["shards6000"] > 4096


@pytest.mark.parametrize("form", ff.WEIGHTS)
@pytest.mark.parametrize("frame", ff.OFFSETS)
@pytest.mark.parametrize("name", ["blobs5000", "blob2000"])
def test_oracle_meets_the_exact_reference_within_the_gpu_tests_bound(orc, name, frame, form):
    """The oracle's serial double chain against the exactly summed reference: counts, labels and the heaviest cluster
    agree; weights and means within n 2^-53 relative, covariances within n 2^-53 max(x^2, y^2) -- the bound
    tests/test_gpu_far_stats.py uses between the device evaluation and the oracle, which the reference therefore can
    meet."""
    s, want, exact = ff.reference(orc, name, frame, form)
    n = s.shape[0]
    eps = n * 2.0 ** -53
    scale = ff.cov_scale(s)
    assert want["n"] == exact["n"] >= (3 if name == "blobs5000" else 1)
    assert np.array_equal(want["count"], exact["count"])
    assert int(want["count"].sum()) == n
    assert int(np.argmax(want["weight"])) == int(np.argmax(exact["weight"]))
    # the labels fed to exact_stats are the oracle's: its counts per label are those of its statistics
    labels = ff.oracle_labels(orc, s)
    assert np.array_equal(np.bincount(labels, minlength=want["n"]), want["count"])
    assert np.all(np.abs(want["weight"] - exact["weight"]) <= eps * exact["weight"])
    assert np.all(np.abs(want["mean"][:, :2] - exact["mean"][:, :2]) <= eps * np.abs(exact["mean"][:, :2]))
    assert np.all(np.abs(want["cov"][:, :4] - exact["cov"][:, :4]) <= eps * scale)
    assert np.all(np.abs(want["set_mean"][:2] - exact["set_mean"][:2]) <= eps * np.abs(exact["set_mean"][:2]))
    assert np.all(np.abs(want["set_cov"][:4] - exact["set_cov"][:4]) <= eps * scale)
    # headings: a few ulp of the circular sums (libm against numpy, serial against exact)
    assert np.allclose(want["mean"][:, 2], exact["mean"][:, 2], rtol=0, atol=1e-12)
    assert np.allclose(want["cov"][:, 4], exact["cov"][:, 4], rtol=0, atol=1e-12, equal_nan=True)


def test_bin_size_is_read_from_the_tree(orc):
    b = ff.bin_size(orc)
    assert b == 0.5
    # ... and a key is floor(x / bin): poses on either side of a far bin boundary fall into two bins, on one side into one
    x = (1 << 22) * b
    for xs, bins in (((x - 0.01, x + 0.01), 2), ((x + 0.01, x + 0.49), 1)):
        t = orc.KDTree()
        for v in xs:
            t.insert_pose((v, 0.0, 0.0))
        assert t.node_count() == bins


@pytest.mark.parametrize("name", [c for c in ff.EDGE_CLOUDS if c.startswith("inside")])
def test_inside_clouds_pack_and_reach_the_last_admitted_key(orc, name):
    b = ff.bin_size(orc)
    s = ff.edge_cloud(name, 3000, b)
    assert np.all(ff.packs(s, b))
    sign, axis = name[-2], name[-1]
    k = ff.keys_of(s, b)["xy".index(axis)]
    if sign == "+":
        assert k.max() == ff.KEY_MAX[axis] and k[0] == ff.KEY_MAX[axis]
    else:
        assert k.min() == ff.KEY_MIN[axis] and k[0] == ff.KEY_MIN[axis]
    assert k.max() - k.min() >= 30  # the cloud spreads over +-10 m
    assert ff.KEY_MAX["x"] == 2 ** 23 - 2 and ff.KEY_MAX["y"] == 2 ** 23 - 1 and ff.KEY_MIN["x"] == -2 ** 23


@pytest.mark.parametrize("name", [c for c in ff.EDGE_CLOUDS if c.startswith("straddle")])
def test_straddle_clouds_decline_in_part(orc, name):
    b = ff.bin_size(orc)
    s = ff.edge_cloud(name, 3000, b)
    share = 1.0 - ff.packs(s, b).mean()
    assert 0.1 <= share <= 0.9, share


def test_mid_cloud_has_high_key_bits_set_on_both_signs(orc):
    b = ff.bin_size(orc)
    s = ff.edge_cloud("mid", 3000, b)
    kx, ky = ff.keys_of(s, b)
    assert np.all(ff.packs(s, b))
    assert kx.min() > 2 ** 22 - 64 and kx.max() < 2 ** 22 + 64 and (kx < 2 ** 22).any() and (kx >= 2 ** 22).any()
    assert ky.min() > -2 ** 22 - 64 and ky.max() < -2 ** 22 + 64
