"""Cluster statistics of one engine in map frames far from the origin (tests/far_frames.py): the 32.96 fixed-point sums
of kernels_stats.hpp end at |sum| < 2^31, which sum w x^2 reaches 46 km out with normalised weights and a few hundred
metres out with weights of 1.  Every frame x weight form x {one-block kernel (2 000 samples), multi-launch path
(5 000)} x BPF_OPT_STATS_HOST.

Host mode: the oracle's bits at every frame.

Device mode: the cluster count, every count (the labels) and the heaviest cluster exact.  Against the EXACTLY summed
reference (far_frames.exact_stats): weights and x / y means within 8 * 2^-53 relative, covariances within
16 * 2^-53 * max(x^2, y^2) absolute -- the integer sum is exact to n 2^-96, fx_to_double rounds twice, the division and
the subtraction add a few ulp of m / W ~ x^2, and the compiler may fuse mean * mean into the subtraction; headings keep
1e-12 (sincos of the device against numpy's, <= 2 ulp per term).  Against the oracle's serial chain, the looser of the
two: n * 2^-53 * max(x^2, y^2) on the covariances.

A case that does not fit the format (a term >= 2e9, or a sum >= 2^31 in a cluster or in the set: over_xx, over_xy,
guard, and most frames with weights of 1) must come back as the host evaluation, bit-equal to the oracle: neither a
wrapped sum nor the per-term guard may show as anything but a correct result.  The engine does not report which
evaluation answered, so the route is read off the result: a case that fits may be answered by either (flagging is
allowed to be conservative), one that does not fit only by the host."""
import numpy as np
import pytest

import far_frames as ff

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _read(pf):
    from test_gpu_shard_stats import read_stats
    return read_stats(pf)


def _equals_oracle(got, want):
    k = int(np.argmax(want["weight"])) if want["n"] else -1
    return (int(got["n"][0]) == want["n"] and np.array_equal(got["set_mean"], want["set_mean"])
            and np.array_equal(got["set_cov"], want["set_cov"], equal_nan=True)
            and np.array_equal(got["weight"], want["weight"]) and np.array_equal(got["mean"], want["mean"])
            and np.array_equal(got["cov"], want["cov"], equal_nan=True)
            and np.array_equal(got["count"], want["count"])
            and (k < 0 or (got["best_w"][0] == want["weight"][k] and np.array_equal(got["best_pose"], want["mean"][k]))))


def _device_errors(got, exact, want, scale):
    """The worst error of each kind in units of its bound (<= 1 passes), and the exact parts as a bool."""
    n = exact["n"]
    same = int(got["n"][0]) == n and np.array_equal(got["count"], exact["count"])
    if not same:
        return False, {}
    k = int(np.argmax(exact["weight"]))
    same = same and got["best_w"][0] == got["weight"][k] and np.array_equal(got["best_pose"], got["mean"][k])
    nn = int(exact["count"].sum())
    err = dict(
        weight=np.max(np.abs(got["weight"] - exact["weight"]) / exact["weight"]) / (8 * EPS),
        mean_xy=np.max(np.abs(got["mean"][:, :2] - exact["mean"][:, :2]) / np.abs(exact["mean"][:, :2])) / (8 * EPS),
        cov=np.max(np.abs(got["cov"][:, :4] - exact["cov"][:, :4])) / (16 * EPS * scale),
        set_mean_xy=np.max(np.abs(got["set_mean"][:2] - exact["set_mean"][:2]) / np.abs(exact["set_mean"][:2])) / (8 * EPS),
        set_cov=np.max(np.abs(got["set_cov"][:4] - exact["set_cov"][:4])) / (16 * EPS * scale),
        heading=np.max(np.abs(got["mean"][:, 2] - exact["mean"][:, 2])) / 1e-12,
        heading_var=np.nanmax(np.abs(got["cov"][:, 4] - exact["cov"][:, 4])) / 1e-12,
        oracle_cov=max(np.max(np.abs(got["cov"][:, :4] - want["cov"][:, :4])),
                       np.max(np.abs(got["set_cov"][:4] - want["set_cov"][:4]))) / (nn * EPS * scale),
        oracle_weight=np.max(np.abs(got["weight"] - want["weight"]) / want["weight"]) / 1e-12,
        oracle_mean_xy=np.max(np.abs(got["mean"][:, :2] - want["mean"][:, :2]) / np.abs(want["mean"][:, :2])) / 1e-12)
    return same, err


@pytest.mark.parametrize("host", [0, 1], ids=["device", "host"])
@pytest.mark.parametrize("name", ["blob2000", "blobs5000"])
@pytest.mark.parametrize("form", ff.WEIGHTS)
@pytest.mark.parametrize("frame", ff.OFFSETS)
def test_cluster_stats_in_far_frames(engine, orc, frame, form, name, host):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    from test_gpu_next_rows import _assert_stats_equal
    s, want, exact = ff.reference(orc, name, frame, form)
    n = s.shape[0]
    pf = bpf.ParticleFilter(engine, 100, n, 0.0, 0.0, 85.0)
    engine.set_option(hpf.OPT_STATS_HOST, host)
    try:
        pf.initWithSamples(s)
        if host:
            _assert_stats_equal(pf, want, exact=True)
            return
        got = _read(pf)
        fits = ff.fits_fixed_point(s, exact)
        by_host = _equals_oracle(got, want)
        same, err = _device_errors(got, exact, want, ff.cov_scale(s))
        print("far stats %s %s %s: fits %d answered by %s, clusters %d, errors / bound %s" %
              (frame, form, name, fits, "host" if by_host else "device", exact["n"],
               {k: float("%.3g" % v) for k, v in err.items()}))
        assert same  # cluster count, every count, the heaviest cluster
        if not fits:
            assert by_host
        else:
            assert by_host or all(v <= 1.0 for v in err.values()), err
        # two evaluations from scratch give the same bits
        pf.snapshot()
        pf.restore()
        again = _read(pf)
        for k in got:
            assert np.array_equal(got[k], again[k], equal_nan=True), k
    finally:
        engine.set_option(hpf.OPT_STATS_HOST, 0)


@pytest.mark.parametrize("name", ["blob2000", "blobs5000"])
def test_the_last_frame_that_fits_is_answered_on_the_device_within_the_exact_bounds(engine, orc, name):
    """`under` with normalised weights (sum w x^2 in (0.99, 1) * 2^31) meets the bounds against the exactly summed
    reference, whichever evaluation answered -- the host's serial chain of n terms would have to be as good as the
    exact sum to pass here -- and `control` and `few_km` do too."""
    import badger_amcl_amd as bpf
    for frame in ("control", "few_km", "under"):
        s, want, exact = ff.reference(orc, name, frame, "normalised")
        assert ff.fits_fixed_point(s, exact)
        pf = bpf.ParticleFilter(engine, 100, s.shape[0], 0.0, 0.0, 85.0)
        pf.initWithSamples(s)
        same, err = _device_errors(_read(pf), exact, want, ff.cov_scale(s))
        assert same and all(v <= 1.0 for v in err.values()), (frame, err)
