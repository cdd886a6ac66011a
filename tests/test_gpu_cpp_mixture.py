"""The mixture initialiser from plain C++ (tests/cpp/mixture_smoke.cpp): badger_amcl_amd::mixtureFromHits on refined
rows, ParticleFilter::initWithMixture on one engine and LocalShardedParticleFilter::initWithMixture at W = 2 -- the
components, the source rows, the merged counts and the sets byte for byte what the Python binding gives."""
import numpy as np
import pytest

import cpp_driver

N, W, SEED = 5000, 2, 33
SIGMA = (0.08, 0.06, 0.03)
XY_MERGE, THETA_MERGE, CAP = 0.1, 0.2, 16


def _rows():
    import badger_amcl_amd.pf as hpf
    rng = np.random.default_rng(12)
    rows = np.zeros(64, dtype=hpf.POSE_REFINED_DTYPE)
    centres = rng.uniform(1.0, 9.0, (24, 2))
    pick = rng.integers(0, 24, 64)
    rows["pose"][:, :2] = centres[pick] + rng.uniform(-0.08, 0.08, (64, 2))
    rows["pose"][:, 2] = rng.uniform(-12.0, 12.0, 64)  # accumulated, not normalised
    rows["score"] = rng.uniform(0.0, 1.0, 64) ** 3
    rows["score"][5] = np.nan
    rows["score"][9] = 0.0
    return rows


def _compile(tmp_path):
    return cpp_driver.compile_driver(tmp_path, "mixture_smoke", "-Wall", "-Werror")


def test_mixture_driver_compiles():
    """CPU: the driver builds against the adapter's new members."""
    import pathlib
    import tempfile
    from badger_amcl_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as d:
        _compile(pathlib.Path(d))


@pytest.mark.gpu
def test_cpp_gives_the_python_rows_and_sets(tmp_path):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    rows = _rows()
    comps, src, merged = bpf.mixtureFromHits(rows, N, XY_MERGE, THETA_MERGE, CAP, SIGMA)
    assert comps.shape[0] == CAP and merged.sum() > 0 and int(comps["count"].sum()) == N
    e = bpf.Engine(0)
    try:
        pf = bpf.ParticleFilter(e, 10, N, 0.0, 0.0, 85.0)
        pf.srand48(SEED)
        pf.initWithMixture(comps)
        want = pf.getCurrentSet().samples.copy()
    finally:
        e.close()
    exe = _compile(tmp_path)
    paths = cpp_driver.write_case(tmp_path, None, dict(rows=rows))
    res = cpp_driver.run_driver(exe, [paths["rows"], N, XY_MERGE, THETA_MERGE, CAP, *SIGMA, SEED, W, tmp_path],
                                timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.split() == [str(CAP), str(W)]
    assert (tmp_path / "components.bin").read_bytes() == comps.tobytes()
    assert (tmp_path / "source_row.bin").read_bytes() == src.tobytes()
    assert (tmp_path / "merged.bin").read_bytes() == merged.tobytes()
    assert (tmp_path / "single.bin").read_bytes() == want.tobytes()
    parts = [np.fromfile(str(tmp_path / ("rank%d.bin" % r)), dtype=np.float64).reshape(-1, 4) for r in range(W)]
    assert [p.shape[0] for p in parts] == [(N * (r + 1)) // W - (N * r) // W for r in range(W)]
    assert np.concatenate(parts).tobytes() == want.tobytes()
