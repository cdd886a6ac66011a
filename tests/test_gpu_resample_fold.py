"""The single-launch resample (draw blocks of 128 draws, the block that finishes last runs the stop rule) against the
separate launches with the host's ordered replay (BPF_OPT_FUSED_RESAMPLE = 0): sets, M, leaf and bin counts,
convergence and the drand48 state equal bit for bit -- over bin counts around the draw blocks' size and the kernel's
limit, and over windows built so that a key's first occurrence and its repeats fall into chosen draw blocks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3000            # 23 draw blocks of 128 and one of 56
BLOCK = 128
CELL_TH = 10 * np.pi / 180
GRID = (16, 16, 8)  # histogram cells the sets are laid on: 2048


@pytest.fixture(scope="module")
def engine():
    import badger_amcl_amd as bpf
    e = bpf.Engine(0)
    yield e
    e.close()


def _cells(n_cells, seed):
    flat = np.random.default_rng(seed).choice(GRID[0] * GRID[1] * GRID[2], size=n_cells, replace=False)
    return np.stack([flat % GRID[0], (flat // GRID[0]) % GRID[1], flat // (GRID[0] * GRID[1])], 1)


def _set_on(cells, cell_of_pose):
    """Poses at the centres of cells[cell_of_pose[i]], equal weights."""
    n = len(cell_of_pose)
    c = cells[np.asarray(cell_of_pose)]
    s = np.empty((n, 4))
    s[:, 0] = (c[:, 0] + 0.5) * 0.5 + 1.0
    s[:, 1] = (c[:, 1] + 0.5) * 0.5 + 1.0
    s[:, 2] = (c[:, 2] + 0.5) * CELL_TH
    s[:, 3] = 1.0 / n
    return s


def _resample(engine, samples, resampler, min_s, fused, cycles=2):
    import badger_amcl_amd as bpf
    import badger_amcl_amd.pf as hpf
    n = samples.shape[0]
    engine.set_option(hpf.OPT_FUSED_RESAMPLE, fused)
    try:
        pf = bpf.ParticleFilter(engine, min_s, n, 0.0, 0.0, 85.0)
        pf.setResampleModel(resampler)
        pf.srand48(11)
        pf.initWithSamples(samples)
        log = []
        for _ in range(cycles):
            pf.updateResample()
            st = pf.getState()
            log.append((pf.getCurrentSet().samples.copy(), st.sample_count, st.leaf_count, st.bin_count,
                        st.converged, pf.getRngState(), st.kld_on_device))
            cur = pf.getCurrentSet().samples
            cur[:, 3] = 1.0 / cur.shape[0]
            pf.initWithSamples(cur)  # (the next cycle draws from the new set again)
        return log
    finally:
        engine.set_option(hpf.OPT_FUSED_RESAMPLE, 1)


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1:6] == b[1:6]


def _both(engine, samples, resampler, min_s, cycles=2):
    one = _resample(engine, samples, resampler, min_s, 1, cycles)
    gen = _resample(engine, samples, resampler, min_s, 0, cycles)
    for c in range(cycles):
        _same(one[c], gen[c])
    return one, gen


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("min_s", [10, N])   # an early stop, and the whole window
@pytest.mark.parametrize("n_bins", [1, 2, 64, 65, 127, 128, 129, 1024])
def test_single_launch_equals_separate_launches(engine, resampler, min_s, n_bins):
    s = _set_on(_cells(n_bins, n_bins), np.arange(N) % n_bins)
    one, gen = _both(engine, s, resampler, min_s)
    for c in range(2):
        assert one[c][6] == 2  # the single-launch resample ran
        assert gen[c][6] != 2
    if min_s == N and resampler == 1:
        assert one[0][1] == N and one[0][3] == n_bins  # systematic, equal weights: every pose once, every bin


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("min_s", [10, N])
def test_one_bin_too_many_falls_back(engine, resampler, min_s):
    """1 025 distinct bins in the window are one more than the kernel's tree holds: the general path takes over."""
    n_bins = 1025
    s = _set_on(_cells(n_bins, 7), np.arange(N) % n_bins)
    one, gen = _both(engine, s, resampler, min_s, cycles=1)
    bins_in_window = len(np.unique(np.floor(gen[0][0][:, :3] / [0.5, 0.5, CELL_TH]).astype(np.int64), axis=0))
    assert gen[0][1] == N  # (that many bins bring no early stop: the window's bins are the new set's)
    if resampler == 1:
        assert bins_in_window == n_bins
    if bins_in_window > 1024:
        assert one[0][6] != 2  # kld_on_device reports the fallback
    else:
        assert one[0][6] == 2


def _draw_order(engine, n, resampler):
    """Which pose each candidate draw takes for n equally weighted poses (the drand48 stream and the CDF decide, not
    the poses): read off a run of the separate launches over poses that differ in x inside one histogram cell."""
    s = _set_on(_cells(1, 1), np.zeros(n, int))
    x0 = s[0, 0]
    s[:, 0] = x0 + (np.arange(n) - n // 2) * 1e-5
    out = _resample(engine, s, resampler, n, 0, cycles=1)[0]
    assert out[1] == n
    d = np.rint((out[0][:, 0] - x0) / 1e-5).astype(int) + n // 2
    assert np.array_equal(s[d, 0], out[0][:, 0])
    return d


def _fresh_after(d, start, taken_before):
    """The first draw index >= start whose pose no draw before `taken_before` takes."""
    early = set(d[:taken_before].tolist())
    for m in range(start, len(d)):
        if d[m] not in early:
            return m
    raise AssertionError("no such draw")


# The windows below are built from the draw order of N equally weighted poses.  The multinomial resampler's order is
# the drand48 stream's whatever the stop; the systematic one's targets depend on the set size, so it runs with min_s = N.
BUILT = [(0, 10), (0, N), (1, N)]


@pytest.mark.parametrize("resampler,min_s", BUILT)
def test_first_occurrence_ends_block_0_repeats_start_block_1(engine, resampler, min_s):
    d = _draw_order(engine, N, resampler)
    cells = _cells(41, 3)
    cell_of = np.arange(N) % 40                      # 40 common bins ...
    first = BLOCK - 1
    assert d[first] not in set(d[:first].tolist())   # (true of the stream pinned by srand48(11); else pick another seed)
    poses = [d[first]] + [d[m] for m in range(BLOCK, BLOCK + 8) if d[m] not in set(d[:first].tolist())]
    assert len(poses) >= 4
    cell_of[poses] = 40                              # ... and one that draw 127 meets first and draws 128 .. repeat
    s = _set_on(cells, cell_of)
    one, gen = _both(engine, s, resampler, min_s, cycles=1)
    assert one[0][6] == 2
    if min_s == N:
        key = np.floor(gen[0][0][:, :3] / [0.5, 0.5, CELL_TH]).astype(np.int64)
        rare = np.flatnonzero((key == cells[40] + [2, 2, 0]).all(1))
        assert rare[0] == first and BLOCK <= rare[1] < BLOCK + 8


@pytest.mark.parametrize("resampler", [0, 1])
@pytest.mark.parametrize("n", [1024, N])             # eight full draw blocks; 23 and one of 56 draws
def test_rarest_key_first_met_in_the_last_block(engine, resampler, n):
    d = _draw_order(engine, n, resampler)
    last_block = ((n - 1) // BLOCK) * BLOCK
    m_rare = _fresh_after(d, last_block + 3, last_block + 3)
    cells = _cells(41, 5)
    cell_of = np.arange(n) % 40
    cell_of[d[m_rare]] = 40
    s = _set_on(cells, cell_of)
    one, gen = _both(engine, s, resampler, n, cycles=1)
    assert one[0][6] == 2
    assert one[0][1] == n and one[0][3] == 41        # the whole window, the rare bin counted
    key = np.floor(gen[0][0][:, :3] / [0.5, 0.5, CELL_TH]).astype(np.int64)
    assert np.flatnonzero((key == cells[40] + [2, 2, 0]).all(1))[0] == m_rare


@pytest.mark.parametrize("resampler,min_s", BUILT)
def test_unpackable_key_drawn_by_a_later_block_falls_back(engine, resampler, min_s):
    """One pose 5 000 km out: its key does not fit the 24 + 24 + 16 bit packing.  No draw of block 0 takes it."""
    d = _draw_order(engine, N, resampler)
    once = np.bincount(d, minlength=N)[d] == 1       # draws whose pose no other draw takes
    m_far = 5 * BLOCK + 17 + int(np.flatnonzero(once[5 * BLOCK + 17:])[0])
    assert m_far < 8 * BLOCK                         # block 5 .. 7 alone meets it
    s = _set_on(_cells(40, 9), np.arange(N) % 40)
    s[d[m_far], 0] = 5.0e6
    one, gen = _both(engine, s, resampler, min_s, cycles=1)
    # the first window of a new filter is the whole stream (3 000 draws): the kernel has drawn the pose whether or
    # not the stop comes before it, and hands the window to the general path
    assert one[0][6] != 2
    if gen[0][1] > m_far:
        assert gen[0][0][m_far, 0] == 5.0e6
