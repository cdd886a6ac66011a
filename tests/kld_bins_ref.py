"""Plain-Python restatement of both resamplers (particle_filter.cpp:269-354 and :356-421) with a switch for what the
KLD stop rule counts (bpf_pf_set_kld_count):
  LEAVES (0): k = PFKDTree::getLeafCount, the reference's rule (the oracle KDTree's leaf_count());
  BINS   (1): k = the number of distinct histogram keys (the oracle KDTree's node_count(): one node per key).
Built like pose_check_ref.py from the drand48 recurrence, a bisection of the serial CDF and the oracle's KDTree and
resampleLimit.  test_kld_bins_cpu.py pins the LEAVES form against the oracle; BINS has no reference run, this is its
reference.  test_gpu_kld_bins.py holds the device to it."""
import bisect

from pose_check_ref import Rng, skip  # noqa: F401  (re-exported for the tests)

LEAVES, BINS = 0, 1


def tree_count(t, mode):
    return t.leaf_count() if mode == LEAVES else t.node_count()


def set_count(samples, mode, kdtree_cls):
    """The count of a whole set in `mode` (the tree of every sample, pf_kdtree.cpp:49-56)."""
    t = kdtree_cls()
    for p in samples[:, :3]:
        t.insert_pose([float(v) for v in p], 1.0)
    return tree_count(t, mode)


def resample(samples, count_k, w_diff, rng, gen, resampler, orc_pf, kdtree_cls, mode):
    """One resample of `samples` (N x 4, the weights the resampler sees).  count_k = the current set's count in `mode`
    (the systematic resampler's size); gen(rng) = random_pose_fn_ for the recovery draws (w_diff > 0); orc_pf: an
    oracle ParticleFilter for resampleLimit (min / max samples, pop_err, pop_z).
    Returns (poses, count of the new set in `mode`, leaf_count, node_count, random flags); rng is advanced."""
    n = samples.shape[0]
    maxs = orc_pf.pf.max_samples
    c = [0.0]
    for w in samples[:, 3]:
        c.append(c[-1] + float(w))

    def find(u):
        i = bisect.bisect_right(c, u) - 1
        assert 0 <= i < n and c[i] <= u < c[i + 1], "CDF miss"
        return i

    t = kdtree_cls()
    want, rnd = [], []
    if resampler == 0:
        while len(want) < maxs:
            if rng.drand48() < w_diff:  # :383 (drawn also when w_diff = 0)
                pose, r = gen(rng), True
            else:
                pose, r = [float(v) for v in samples[find(rng.drand48()), :3]], False
            want.append(pose)
            rnd.append(r)
            t.insert_pose(pose, 1.0)
            if len(want) > orc_pf.resample_limit(tree_count(t, mode)):  # :416
                break
    else:
        count = orc_pf.resample_limit(count_k)
        n_random = 0
        if w_diff > 0.0:
            count = int(count * (1.0 + w_diff))
            count = min(count, maxs)
            n_random = int(w_diff * count)
        n_sys = count - n_random
        start = rng.drand48()
        delta = 1.0 / n_sys
        for _ in range(n_random):
            want.append(gen(rng))
            rnd.append(True)
        target = start
        for _ in range(n_sys):
            want.append([float(v) for v in samples[find(target), :3]])
            rnd.append(False)
            target += delta
            if target > 1.0:
                target -= 1.0
        for pose in want:
            t.insert_pose(pose, 1.0)
    return want, tree_count(t, mode), t.leaf_count(), t.node_count(), rnd


def stop_of_stream(keys, orc_pf, mode, kdtree_cls):
    """The multinomial stop rule over a given key stream: the set size M (len(keys) when it does not stop)."""
    t = kdtree_cls()
    for m, k in enumerate(keys):
        t.insert_key(k, 1.0)
        if m + 1 > orc_pf.resample_limit(tree_count(t, mode)):
            return m + 1
    return len(keys)
