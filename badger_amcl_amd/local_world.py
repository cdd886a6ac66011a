"""A sharded filter with ALL its ranks in this process (include/badger_pf.h, bpf_shard_connect_local).

LocalShardedFilter owns W engines' filters and W worker threads, one per engine, and carries ShardedFilter's public
method names: every collective member fans out to the workers -- each enters the engine's one-call form
(bpf_shard_update_sensor_planar, bpf_shard_update_resample, ...) for its rank, ctypes releases the GIL for the length
of the call, and the ranks meet inside the library at the exchanges -- and joins them.  The ranks' status codes must
agree (a RuntimeError otherwise); the figures returned are rank 0's.  There is no torch.distributed process group, no
socket and no child process behind it."""
import ctypes as C
import queue
import threading

import numpy as np

from . import _lib
from .pf import POSE_HIT_DTYPE, BpfError, mixture_components
from .sharded import (RESAMPLE_FORMS, TREE_ROUTES, ShardedState, check_kld_modes, check_settings, even_counts,
                      mixture_of_hits)

EXCHANGE_NONE, EXCHANGE_MAILBOX, EXCHANGE_RCCL, EXCHANGE_LOCAL = 0, 1, 2, 3
STATS_ROUTES = {1: "gathered", 2: "distributed", 3: "host"}
_dp = C.POINTER(C.c_double)


class _Worker(threading.Thread):
    """The host thread of one rank: runs what it is handed, in order."""

    def __init__(self, rank):
        super().__init__(name="bpf-local-rank-%d" % rank, daemon=True)
        self.jobs = queue.Queue()
        self.start()

    def run(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            fn, box, done = job
            try:
                box.append((True, fn()))
            except BaseException as err:  # handed to the caller of run()
                box.append((False, err))
            done.set()

    def submit(self, fn):
        box, done = [], threading.Event()
        self.jobs.put((fn, box, done))
        return box, done


class LocalShardedFilter:
    """pfs[r]: the pf.ParticleFilter of rank r, each on an engine of its own, created with the GLOBAL min / max sample
    counts and holding rank r's contiguous slice (or nothing yet, when an init follows)."""

    def __init__(self, pfs, first_window=4096, timeout_ms=None, kld_count=None, connect=True, resample_form="window",
                 max_share=2.0, rebalance="off", trigger_share=1.5, multinomial_form="window"):
        """multinomial_form: as for ShardedFilter ("in_place": the multinomial resampler resamples every slice into
        itself, the stop index from the ranks' bin lists; max_share and rebalance apply to it too).
        resample_form, max_share: as for ShardedFilter ("in_place": the systematic resampler resamples every slice
        into itself, self.counts is uneven afterwards, self.form_used tells which form a resample took).
        rebalance, trigger_share: as for ShardedFilter ("auto": an in-place resample never falls back to the window
        form, and slices more uneven than trigger_share * ceil(M / W) go back to the even split behind it;
        self.rebalanced tells how many samples moved)."""
        self.pfs = list(pfs)
        self.world = len(self.pfs)
        self.engines = [p.e for p in self.pfs]
        self.lib = self.engines[0].lib
        self.max_global = self.pfs[0].max_samples
        self._workers = [_Worker(r) for r in range(self.world)]
        self._first_window = first_window
        self.window_hint = [first_window] * self.world
        self.sample_count = 0
        self.leaf_count = self.bin_count = 0
        self.windows_used = 0
        self.cdf_miss = False
        self.stats_route = self.tree_route = None
        self.counts = [0] * self.world
        form, mn_form, rebalance_code = check_settings(resample_form, multinomial_form, rebalance)
        self.resample_form, self.max_share, self.form_used = resample_form, float(max_share), "window"
        self.multinomial_form = multinomial_form
        self.rebalance_mode, self.trigger_share, self.rebalanced = rebalance, float(trigger_share), 0
        for e in self.engines:
            e.check(self.lib.bpf_shard_set_resample_form(e.h, form, self.max_share))
            e.check(self.lib.bpf_shard_set_multinomial_form(e.h, mn_form))
            e.check(self.lib.bpf_shard_set_rebalance(e.h, rebalance_code, self.trigger_share))
        if kld_count is not None:
            for p in self.pfs:
                p.setKldCount(int(kld_count))
        modes = [p.getKldCount() for p in self.pfs]
        self.kld_count = check_kld_modes("LocalShardedFilter", modes)
        if timeout_ms is not None:
            self.set_timeout_ms(timeout_ms)
        if connect:
            self.connect()

    # ---- the world
    def connect(self):
        """bpf_shard_connect_local over the engines (again after a broken world: the old one is released)."""
        arr = (C.c_void_p * self.world)(*[e.h for e in self.engines])
        rc = self.lib.bpf_shard_connect_local(arr, self.world, 0)
        if rc != 0:
            raise BpfError(rc, "bpf_shard_connect_local: " + self.lib.bpf_error_string(rc).decode())

    def set_timeout_ms(self, ms):
        for e in self.engines:
            e.check(self.lib.bpf_shard_mailbox_set_timeout_ms(e.h, int(ms)))

    def exchange_mode(self):
        out = []
        for e in self.engines:
            m = C.c_int(-1)
            e.check(self.lib.bpf_shard_exchange_mode(e.h, C.byref(m)))
            out.append(m.value)
        return out

    def exchange_counts(self):
        out = []
        for e in self.engines:
            n = C.c_longlong(-1)
            e.check(self.lib.bpf_shard_exchange_count(e.h, C.byref(n)))
            out.append(n.value)
        return out

    def shutdown(self):
        for e in self.engines:
            if e.h:
                self.lib.bpf_shard_shutdown(e.h)

    def close(self):
        """Ends the worker threads (the engines stay with their owner)."""
        for w in self._workers:
            w.jobs.put(None)
        for w in self._workers:
            w.join()
        self._workers = []

    # ---- fan out and join
    def run(self, fn, ranks=None):
        """fn(rank) on the worker thread of every rank in `ranks` (default: all) at once; the results in that order.
        An exception raised on a worker is raised here (the first one by rank) after all have finished."""
        ranks = list(range(self.world)) if ranks is None else list(ranks)
        pending = [self._workers[r].submit(lambda r=r: fn(r)) for r in ranks]
        out = []
        for box, done in pending:
            done.wait()
            out.append(box[0])
        for ok, val in out:
            if not ok:
                raise val
        return [val for _, val in out]

    def for_each_rank(self, fn):
        """fn(rank, pf) on every rank's thread: map / scanner / model set-up of the engines, in parallel."""
        return self.run(lambda r: fn(r, self.pfs[r]))

    def codes(self, call, ranks=None):
        """call(rank, engine handle, lib) -> status code, on the ranks' threads; the codes as they came back."""
        return self.run(lambda r: int(call(r, self.engines[r].h, self.lib)), ranks)

    def _collective(self, call):
        rcs = self.codes(call)
        if len(set(rcs)) != 1:
            raise RuntimeError("LocalShardedFilter: the ranks' statuses differ: %s" % rcs)
        if rcs[0] != 0:
            self.engines[0].check(rcs[0])

    # ---- starting the set
    def _even_share(self, n):
        self.counts = even_counts(n, self.world)
        self.sample_count = n

    def _first(self, r):
        return sum(self.counts[:r])

    def _after_init(self):
        self._even_share(self.max_global)
        self.leaf_count, self.bin_count = self._global_leaf_count()
        self.window_hint = [self._first_window] * self.world
        self.windows_used = 0
        r = C.c_int()
        self.engines[0].check(self.lib.bpf_shard_tree_last_route(self.engines[0].h, C.byref(r)))
        self.tree_route = TREE_ROUTES.get(r.value)

    def init_with_gaussian(self, mean, rotation, sigma):
        m, rot, d = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (mean, rotation, sigma))
        assert m.size == 3 and rot.size == 9 and d.size == 3
        self._collective(lambda r, h, lib: lib.bpf_shard_init_with_gaussian_all(
            h, m.ctypes.data_as(_dp), rot.ctypes.data_as(_dp), d.ctypes.data_as(_dp)))
        self._after_init()

    def init_with_mixture(self, components):
        """ParticleFilter.initWithMixture over the local world: the counts sum to max_samples of the global set."""
        comps, ptr = mixture_components(components)
        self._collective(lambda r, h, lib: lib.bpf_shard_init_with_mixture_all(h, ptr, comps.shape[0]))
        self._after_init()

    def init_with_random_poses(self):
        self._collective(lambda r, h, lib: lib.bpf_shard_init_with_random_poses_all(h))
        self._after_init()

    def load(self, slices, tree=True):
        """Slices loaded by hand: slices[r] = [n_r, 4] samples of rank r (n_r = 0 allowed), in global order.  tree: the
        leaf and bin counts of the global set's tree come over the exchange (the systematic resampler reads them
        before the first resample); without it they read 0 until a resample installs them."""
        assert len(slices) == self.world
        self.counts = [int(np.asarray(s).shape[0]) for s in slices]
        self.sample_count = sum(self.counts)
        total = self.sample_count

        def put(r, pf):
            if self.counts[r] > 0:
                return pf.initWithSamples(np.asarray(slices[r], dtype=np.float64).reshape(-1, 4))
            # a shard without samples (bpf_pf_set_samples takes none): adopt an empty slice of the global set
            pf.e.check(self.lib.bpf_shard_adopt_dev(pf.e.h, None, None, None, 0, total, 0, 0))
        self.for_each_rank(put)
        self.leaf_count, self.bin_count = self._global_leaf_count() if tree else (0, 0)
        self.window_hint = [self._first_window] * self.world

    def restore(self, counts, leaf_count=0):
        """The shards were put back by pf.restore(): reset the bookkeeping (ShardedFilter.restore)."""
        self.counts = list(counts)
        self.sample_count = sum(counts)
        self.leaf_count = leaf_count

    def _global_leaf_count(self):
        got = [None] * self.world

        def call(r, h, lib):
            a, b = C.c_int(), C.c_int()
            rc = lib.bpf_shard_global_leaf_count(h, C.byref(a), C.byref(b))
            got[r] = (a.value, b.value)
            return rc
        self._collective(call)
        if len(set(got)) != 1:
            raise RuntimeError("LocalShardedFilter: the ranks disagree on the global tree: %s" % got)
        return got[0]

    # ---- the steps
    def update_action(self, odom, data):
        """odom: the pf.Odom of every rank (a list), or one pf.Odom whose model every engine already carries."""
        def call(r, h, lib):
            return lib.bpf_shard_update_action(h, data.pose.ctypes.data_as(_dp), data.delta.ctypes.data_as(_dp),
                                               data.absolute_motion.ctypes.data_as(_dp), self._first(r),
                                               self.sample_count)
        self._collective(call)

    def update_sensor(self, data):
        """pf.PlanarData (beam skipping of the prob model included) or pf.PointCloudData."""
        n = self.sample_count
        if hasattr(data, "points_"):
            pts = data.points_
            ptr = pts.ctypes.data_as(C.POINTER(C.c_float))
            return self._collective(lambda r, h, lib: lib.bpf_shard_update_sensor_cloud(h, ptr, pts.shape[0], n))
        ranges, angles = data.pointers()
        self._collective(lambda r, h, lib: lib.bpf_shard_update_sensor_planar(h, ranges, angles, data.range_count_,
                                                                               data.range_max_, n))

    def update_resample(self):
        got = [None] * self.world

        def call(r, h, lib):
            m, leaf, bins = C.c_int(self.sample_count), C.c_int(self.leaf_count), C.c_int(0)
            wins, hint, miss = C.c_int(0), C.c_int(self.window_hint[r]), C.c_int(0)
            rc = lib.bpf_shard_update_resample(h, C.byref(m), C.byref(leaf), C.byref(bins), C.byref(wins), C.byref(hint),
                                               C.byref(miss))
            got[r] = (m.value, leaf.value, bins.value, wins.value, hint.value, miss.value)
            return rc
        try:
            self._collective(call)
        except (BpfError, RuntimeError):
            # rebalance="auto": the call can fail AFTER its resample became current, in the rebalance behind it.  The
            # books then follow the new, uneven set before the error goes up: the resample must not be run again;
            # rebalance() may be
            if all(self._resample_committed(r) for r in range(self.world)) and None not in got:
                self._after_resample(got)
            raise
        self._after_resample(got)

    def _resample_committed(self, r):
        c = C.c_int()
        self.engines[r].check(self.lib.bpf_shard_resample_committed(self.engines[r].h, C.byref(c)))
        return bool(c.value)

    def _after_resample(self, got):
        if len(set(g[:3] for g in got)) != 1:
            raise RuntimeError("LocalShardedFilter: the ranks resampled to different sets: %s" % got)
        m, self.leaf_count, self.bin_count, self.windows_used = got[0][:4]
        self.window_hint = [g[4] for g in got]
        self.cdf_miss = any(g[5] for g in got)
        self._even_share(m)
        self.form_used = "window"
        if self.resample_form == "in_place" or self.multinomial_form == "in_place":
            # the split is the engines' record: uneven after a resample that stayed in place
            slices = [self.slice(r) for r in range(self.world)]
            if len(set(sl[2] for sl in slices)) != 1:
                raise RuntimeError("LocalShardedFilter: the ranks took different resample forms: %s" % slices)
            if slices[0][2] == RESAMPLE_FORMS["in_place"]:
                self.counts = [sl[1] for sl in slices]
                self.form_used = "in_place"
                if [sl[0] for sl in slices] != [self._first(r) for r in range(self.world)] or sum(self.counts) != m:
                    raise RuntimeError("LocalShardedFilter: the ranks' slices do not tile the set: %s" % slices)
                self.rebalanced = self._rebalance_last() if self.rebalance_mode == "auto" else 0

    def _rebalance_last(self):
        got = []
        for e in self.engines:
            t = C.c_longlong(-1)
            e.check(self.lib.bpf_shard_rebalance_last(e.h, C.byref(t)))
            got.append(t.value)
        if len(set(got)) != 1:
            raise RuntimeError("LocalShardedFilter: the ranks moved different numbers of samples: %s" % got)
        return got[0]

    def rebalance(self):
        """The slices back to the even split in global order (bpf_shard_rebalance on every rank): only the samples on
        the wrong rank move.  Returns the number moved over all ranks; 0: the split was even already."""
        got = [None] * self.world

        def call(r, h, lib):
            t = C.c_longlong(-1)
            rc = lib.bpf_shard_rebalance(h, C.byref(t))
            got[r] = t.value
            return rc
        self._collective(call)
        if len(set(got)) != 1:
            raise RuntimeError("LocalShardedFilter: the ranks moved different numbers of samples: %s" % got)
        self._even_share(sum(self.counts))
        self.rebalanced = got[0]
        return got[0]

    def slice(self, r):
        """(global_first, local_count, form_used) of rank r's engine (bpf_shard_slice)."""
        first, n, form = C.c_longlong(), C.c_int(), C.c_int()
        self.engines[r].check(self.lib.bpf_shard_slice(self.engines[r].h, C.byref(first), C.byref(n), C.byref(form)))
        return first.value, n.value, form.value

    # ---- the global pose and the particle cloud
    def compute_cluster_stats(self):
        """(cluster_count, set_mean[3], set_cov[5]) of the global set, the same bits on every rank."""
        got = [None] * self.world

        def call(r, h, lib):
            n, route = C.c_int(), C.c_int()
            mean, cov = np.zeros(3), np.zeros(5)
            rc = lib.bpf_shard_compute_cluster_stats(h, C.byref(n), mean.ctypes.data_as(_dp), cov.ctypes.data_as(_dp),
                                                     C.byref(route))
            got[r] = (n.value, mean, cov, route.value)
            return rc
        self._collective(call)
        for g in got[1:]:
            if g[0] != got[0][0] or g[1].tobytes() != got[0][1].tobytes() or g[2].tobytes() != got[0][2].tobytes():
                raise RuntimeError("LocalShardedFilter: the ranks' statistics differ")
        self.stats_route = STATS_ROUTES.get(got[0][3])
        return got[0][:3]

    def get_cluster(self, k):
        """(weight, mean[3], count, cov[5]) of cluster k of the global set, None past the last cluster."""
        self.compute_cluster_stats()
        return self.pfs[0].getClusterStats(k)

    def get_max_weight_pose(self):
        got = [None] * self.world

        def call(r, h, lib):
            w, pose = C.c_double(), np.zeros(3)
            rc = lib.bpf_shard_get_max_weight_pose(h, C.byref(w), pose.ctypes.data_as(_dp))
            got[r] = (w.value, pose)
            return rc
        self._collective(call)
        for g in got[1:]:
            if g[0] != got[0][0] or g[1].tobytes() != got[0][1].tobytes():
                raise RuntimeError("LocalShardedFilter: the ranks' max-weight poses differ")
        return got[0]

    def get_pose_array(self, root=0, first=0, stride=1):
        """[count, 7] float64 rows of the global samples first, first + stride, ... as rank `root` receives them
        (root = -1: every rank receives; rank 0's copy is returned after they were compared)."""
        if not -1 <= root < self.world:
            raise ValueError("get_pose_array: root in [-1, world)")
        n = self.sample_count
        room = (n - first + stride - 1) // stride if stride >= 1 and 0 <= first < n else 0
        got = [None] * self.world

        def call(r, h, lib):
            receives = root < 0 or root == r
            out = np.empty((max(room, 1), 7), dtype=np.float64) if receives else None
            cnt = C.c_int()
            rc = lib.bpf_shard_get_pose_array(h, int(root), int(first), int(stride),
                                              out.ctypes.data_as(_dp) if receives else None, int(room), C.byref(cnt))
            got[r] = out[:cnt.value] if receives and rc == 0 else None
            return rc
        self._collective(call)
        if root >= 0:
            return got[root]
        for g in got[1:]:
            if g.tobytes() != got[0].tobytes():
                raise RuntimeError("LocalShardedFilter: the ranks' pose arrays differ")
        return got[0]

    # ---- global localisation: pose search over the ranks
    def _search(self, k, call, want_stats):
        """call(rank, handle, lib, hits*, n*, stats*) -> status on every rank's thread; the rows (rank 0's, after all
        ranks' rows were compared as bytes) and, for the pruned forms, every rank's stats."""
        W = self.world
        hits = [np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE) for _ in range(W)]
        ns = [C.c_int(0) for _ in range(W)]
        sts = [_lib.PoseSearchStats() for _ in range(W)]
        self._collective(lambda r, h, lib: call(r, h, lib, hits[r].ctypes.data_as(C.POINTER(_lib.PoseHit)),
                                                C.byref(ns[r]), C.byref(sts[r])))
        rows = [hits[r][:ns[r].value] for r in range(W)]
        for r in range(1, W):
            if rows[r].tobytes() != rows[0].tobytes():
                raise RuntimeError("LocalShardedFilter: the ranks' search rows differ (rank %d)" % r)
        if want_stats:
            return rows[0], [{name: getattr(st, name) for name, _ in _lib.PoseSearchStats._fields_} for st in sts]
        return rows[0]

    def search_poses(self, data, headings, cell_stride, k, first=0, count=-1):
        """PlanarScanner.searchPoses over the ranks (bpf_shard_search_poses): rank r scores candidates
        [first + T r / W, first + T (r + 1) / W) of the T given, the lists are merged on the device, and the rows are
        the single engine's, byte for byte.  Every engine carries the map and the scanner's model already, as for
        update_sensor."""
        rp, ap = data.pointers()
        return self._search(k, lambda r, h, lib, hits, n, st: lib.bpf_shard_search_poses(
            h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(first), int(count),
            int(k), hits, n), False)

    def search_poses_pruned(self, data, headings, cell_stride, k, block=8, first_block=0, block_count=-1):
        """PlanarScanner.searchPosesPruned over the ranks (bpf_shard_search_poses_pruned): the block range is split,
        and behind their seeds the ranks prune against the largest k-th score any of them holds.  Returns
        (rows, per-rank stats); a rank's stats count its own share."""
        rp, ap = data.pointers()
        return self._search(k, lambda r, h, lib, hits, n, st: lib.bpf_shard_search_poses_pruned(
            h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(block),
            int(first_block), int(block_count), int(k), hits, n, st), True)

    def cloud_search_poses(self, data, headings, cell_stride, k, first=0, count=-1):
        """PointCloudScanner.searchPoses over the ranks (bpf_shard_cloud_search_poses)."""
        pts = data.points_
        ptr = pts.ctypes.data_as(C.POINTER(C.c_float))
        return self._search(k, lambda r, h, lib, hits, n, st: lib.bpf_shard_cloud_search_poses(
            h, ptr, pts.shape[0], int(headings), int(cell_stride), int(first), int(count), int(k), hits, n), False)

    def cloud_search_poses_pruned(self, data, headings, cell_stride, k, block=8, first_block=0, block_count=-1):
        """PointCloudScanner.searchPosesPruned over the ranks (bpf_shard_cloud_search_poses_pruned): (rows, per-rank
        stats)."""
        pts = data.points_
        ptr = pts.ctypes.data_as(C.POINTER(C.c_float))
        return self._search(k, lambda r, h, lib, hits, n, st: lib.bpf_shard_cloud_search_poses_pruned(
            h, ptr, pts.shape[0], int(headings), int(cell_stride), int(block), int(first_block), int(block_count),
            int(k), hits, n, st), True)

    def localize(self, scanners, data, headings, cell_stride, k, refine, moments, mixture, pruned=True, block=8):
        """Global localisation in one call, host composition only: the sharded search; refinePoses and poseMoments on
        every rank (replicated: at most 1024 lattices, identical inputs on identical devices); mixtureFromHits and
        mixtureApplyMoments; init_with_mixture.  scanners[r]: rank r's PlanarScanner or PointCloudScanner.
        refine = (xy_radius, xy_step, theta_radius, theta_step, levels); moments = (xy_radius, xy_step, theta_radius,
        theta_step, baseline, sigma_floor, sigma_cap); mixture = (xy_merge, theta_merge, max_components, sigma).
        Returns the components."""
        cloud = hasattr(data, "points_")
        if pruned:
            hits, _ = (self.cloud_search_poses_pruned if cloud else self.search_poses_pruned)(
                data, headings, cell_stride, k, block)
        else:
            hits = (self.cloud_search_poses if cloud else self.search_poses)(data, headings, cell_stride, k)
        comps = self.for_each_rank(lambda r, pf: mixture_of_hits(scanners[r], data, hits, self.max_global, refine,
                                                                 moments, mixture))
        for c in comps[1:]:
            if c.tobytes() != comps[0].tobytes():
                raise RuntimeError("LocalShardedFilter: the ranks' mixtures differ")
        self.init_with_mixture(comps[0])
        return comps[0]

    def selftest(self, rounds=1):
        """bpf_shard_local_selftest on every rank."""
        self._collective(lambda r, h, lib: lib.bpf_shard_local_selftest(h, int(rounds)))

    def set_random_pose_generator(self, mode):
        for p in self.pfs:
            p.setRandomPoseGenerator(mode)

    def set_uniform_pose_check(self, threshold, multiplier, scoring=0):
        for p in self.pfs:
            p.setUniformPoseCheck(threshold, multiplier, scoring)

    def rank_states(self):
        return [p.getState() for p in self.pfs]

    def rng_states(self):
        return [p.getRngState() for p in self.pfs]

    def local_sets(self):
        """The ranks' slices on the host, [n_r, 4] each, in rank order."""
        return self.for_each_rank(lambda r, pf: pf.getCurrentSet().samples)

    def state(self):
        st = self.pfs[0].getState()
        return ShardedState(sample_count=self.sample_count, local_count=st.sample_count, leaf_count=self.leaf_count,
                            bin_count=self.bin_count, converged=st.converged,
                            percent_converged=st.percent_converged, w_slow=st.w_slow, w_fast=st.w_fast,
                            total=st.total, cdf_miss=self.cdf_miss, windows=self.windows_used)
