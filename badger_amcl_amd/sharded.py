"""One particle filter sharded over the GPUs of a node: one process per GPU, each engine holds a
contiguous slice of the particle index space, `torch.distributed` (backend "nccl" = RCCL over
xGMI) carries the three small exchanges the path really has:

  update_action    none: every rank walks the same drand48 stream (attempt compaction over the GLOBAL
                   Gaussian ranks), materialises the draws of its own index range and ends on the same state
  update_sensor    all-gather of W per-shard weight totals (8 B each)
  update_resample  per candidate-draw window one integer all-reduce(sum) of [6, window] int64 (pose
                   bits + histogram key of every draw; exactly one shard writes each column, the
                   others contribute 0).  The shards' slices of the global CDF come from the totals
                   gathered by the sensor update (slice_q = total_q / sum(totals), the same quotient on
                   every rank), so no further exchange is needed; only when the weights were set by
                   something else than update_sensor are the W local CDF sums all-gathered instead.
                   Recovery draws (w_diff > 0): every rank resolves the same draw chain and shard 0 writes
                   the random free-space poses -- no further exchange.

                   resample_form="in_place" (systematic only, opt-in): no window.  Every rank resamples its own slice
                   into its own slice (the teeth of the comb that fall into its slice of the global CDF); what crosses
                   is the bin lists of the new tree (16 B per occupied bin), nine int64 words (limb sums of x and y,
                   all-reduced) and one int64 count (all-reduced) for updateConverged.  The slices come out uneven
                   and concatenate to the single engine's set with the wrapped teeth moved to the front.

                   rebalance() / rebalance="auto": the slices back to the even split in global order; only the
                   samples on the wrong rank move, one ragged all-gather of their x / y / theta / w bits (32 B per moved
                   sample into every rank: the gather is a broadcast, no point-to-point form is built).

  init             (init_with_gaussian / init_with_random_poses: every rank writes its even share of the set ONE
                   engine would produce and ends on the same drand48 state -- no exchange for the poses) then the
                   histogram tree of the GLOBAL set, whose leaf count the systematic resampler reads first: all-gather
                   of the per-rank bin lists (16 B per occupied bin), merged redundantly on every rank into the distinct
                   keys in first-appearance order, and the tree of those.  A key outside the packing range on any
                   rank sends every rank down the keys route (12 B per particle, host tree).

  statistics       (compute_cluster_stats / get_cluster / get_max_weight_pose: the clusters of the GLOBAL set and
                   the pose of the heaviest one, the same bits on every rank as one engine holding the whole set)
                   up to 4096 particles: one all-gather of the slices' x / y / theta / weight (<= 128 KB), every rank
                   evaluates the whole set in one single-block launch.  Larger sets stay where they are: all-gather
                   of the per-rank bin lists (packed key + global index of the key's first sample, 16 B per occupied
                   bin), bins merged and labelled redundantly on every rank, then one integer all-reduce(sum) of the
                   per-cluster fixed-point sums (ten 128-bit sums per cluster as four 32-bit limbs in int64 words, so
                   the lane-wise sum is exact).  A key outside the packing range or a non-finite term on any rank
                   sends every rank to the host evaluation of the gathered set (32 B per particle).

Scoring itself shards with no communication.  The KLD stop rule (an ordered kd-tree replay) runs
redundantly on every rank from the assembled key window, so all ranks agree on the sample count
without another exchange; the resampled set is re-split evenly in index order.

`ShardedFilter` is backend-agnostic: `HipShardBackend` drives the C-ABI stage functions
(bpf_shard_*); the CPU tests plug in a backend of their own over gloo.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .pf import POSE_HIT_DTYPE, merge_pose_hits, mixture_components, mixtureApplyMoments, mixtureFromHits


class _DevArray:
    """Zero-copy view of engine-owned device memory for torch (cuda array interface v2)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


_VIEW_DTYPES = {"<i8": torch.int64, "<f8": torch.float64, "<i4": torch.int32}


class HipShardBackend:
    """Stage functions of include/badger_pf.h on one GPU.  Runs on torch's current stream so that
    torch copies / RCCL collectives and engine kernels are ordered without host syncs."""

    def __init__(self, engine, scanner, pf, device):
        self.e, self.sc, self.pf = engine, scanner, pf
        self.device = device
        stream = torch.cuda.current_stream(device)
        engine.set_stream(stream.cuda_stream)
        p = C.c_void_p()
        engine.check(engine.lib.bpf_shard_scalars_dev(engine.h, C.byref(p)))
        self.scalars = torch.as_tensor(_DevArray(p.value, (16,), "<f8"), device=device)
        self._total_view, self._sum_view = self.scalars[0:1], self.scalars[7:8]
        self._engine_device_min = None

    def n_local(self):
        return self.pf.getState().sample_count

    # ---- mailbox exchange (include/badger_pf.h, bpf_shard_mailbox_*): peer stores over xGMI instead of collectives
    def mailbox_create(self, rank, world, max_window):
        """64-byte IPC handle of this engine's mailbox, or None when it cannot be allocated / exported."""
        buf = (C.c_ubyte * 64)()
        rc = self.e.lib.bpf_shard_mailbox_create(self.e.h, rank, world, int(max_window), buf)
        self._mb_world, self._mb_stride, self._mb_views = world, int(max_window), {}
        self._mb_rank = rank
        return bytes(buf) if rc == 0 else None

    def mailbox_connect(self, handles):
        """Maps the peers (handles: world x 64 bytes in rank order) and runs one round with all of them."""
        return self.e.lib.bpf_shard_mailbox_connect(self.e.h, C.c_char_p(handles)) == 0

    def mailbox_update_sensor(self, data, global_n):
        """Scoring, exchange of the totals and normalisation in one call; None when beam skipping needs the
        caller's all-reduce in between (the stage functions finish the update then)."""
        rp, ap = data.pointers()
        rc = self.e.lib.bpf_shard_mailbox_update_sensor_planar(self.e.h, rp, ap, data.range_count_, data.range_max_,
                                                               int(global_n))
        if rc == 100:  # BPF_SHARD_NEED_BEAM_COUNTS
            return None
        self.e.check(rc)
        return True

    def mailbox_update_resample(self, flags, global_n, leaf_count, window_hint):
        """updateResample of the shard in one call: (M, leaf_count, bin_count, windows, window_hint)."""
        if self._engine_device_min != self.kld_device_min:
            self.e.set_option(3, int(self.kld_device_min) if self.kld_device_min < (1 << 31) else 0)  # KLD_DEVICE_MIN
            self._engine_device_min = self.kld_device_min
        g, lf, bn, wn, hint = (C.c_int(int(global_n)), C.c_int(int(leaf_count)), C.c_int(0), C.c_int(0),
                               C.c_int(int(window_hint)))
        rc = self.e.lib.bpf_shard_mailbox_update_resample(self.e.h, C.c_void_p(flags.data_ptr()), C.byref(g),
                                                          C.byref(lf), C.byref(bn), C.byref(wn), C.byref(hint))
        # (kept for resample_committed(): the engine wrote them before an AUTO rebalance that failed behind the resample)
        self.last_resample = (g.value, lf.value, bn.value, wn.value, hint.value)
        self.e.check(rc)
        return self.last_resample

    def resample_committed(self):
        """True when the last one-call resample made its new set current, whatever it returned (an error then came
        from the AUTO rebalance behind it: the resample must not be run again)."""
        c = C.c_int()
        self.e.check(self.e.lib.bpf_shard_resample_committed(self.e.h, C.byref(c)))
        return bool(c.value)

    def mailbox_selftest(self, rounds=4):
        """Full window exchanges with a payload every rank verifies (both parities, twice)."""
        return self.e.lib.bpf_shard_mailbox_selftest(self.e.h, rounds) == 0

    def mailbox_destroy(self):
        self.e.lib.bpf_shard_mailbox_destroy(self.e.h)

    def mailbox_set_timeout_ms(self, ms):
        self.e.check(self.e.lib.bpf_shard_mailbox_set_timeout_ms(self.e.h, int(ms)))

    def mailbox_error_stage(self):
        """(totals wait failed, window wait failed) of the mailbox in use; drains the stream first."""
        a, b = C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_mailbox_error_stage(self.e.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def _view(self, ptr, shape, typestr="<i8"):
        """Device tensor over engine memory the library handed out; an empty tensor of that shape when it holds
        nothing (the pointer need not be valid then)."""
        if 0 in shape:
            return torch.empty(shape, dtype=_VIEW_DTYPES[typestr], device=self.device)
        return torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.device)

    def _bins(self, fn, *args):
        """(int64 [2, n_bins] device tensor, flag) of one of the bpf_shard_*_bins_dev entry points."""
        p, n, flag = C.c_void_p(), C.c_int(), C.c_int()
        self.e.check(fn(self.e.h, *args, C.byref(p), C.byref(n), C.byref(flag)))
        return self._view(p.value, (2, n.value)), bool(flag.value)

    def _mb_view(self, ptr, shape, typestr):
        v = self._mb_views.get(ptr)
        if v is None:
            v = self._mb_views[ptr] = torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.device)
        return v

    def mailbox_totals(self):
        """The W totals of the scoring stage just issued (complete once normalize has run: it waits in-kernel)."""
        p = C.c_void_p()
        self.e.check(self.e.lib.bpf_shard_mailbox_totals(self.e.h, C.byref(p)))
        return self._mb_view(p.value, (self._mb_world,), "<f8")

    def mailbox_window(self):
        """A fresh [6, max_window] int64 window; valid until the next-but-one call."""
        p, stride = C.c_void_p(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_mailbox_window(self.e.h, C.byref(p), C.byref(stride)))
        return self._mb_view(p.value, (6, stride.value), "<i8")

    def score(self, data):
        lib, e = self.e.lib, self.e
        if hasattr(data, "points_"):  # PointCloudData: the 3-D path
            e.check(lib.bpf_shard_score_cloud(e.h, data.points_.ctypes.data_as(C.POINTER(C.c_float)),
                                              data.points_.shape[0]))
            return
        rp, ap = data.pointers()
        rc = lib.bpf_shard_score_planar(e.h, rp, ap, data.range_count_, data.range_max_)
        if rc != 100:  # BPF_SHARD_NEED_BEAM_COUNTS
            e.check(rc)
            return None
        # beam skipping: the per-beam agreement counts have to be summed over the shards first
        return self.beam_counts()

    def beam_counts(self):
        p, n = C.c_void_p(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_beam_counts_dev(self.e.h, C.byref(p), C.byref(n)))
        return self._view(p.value, (n.value,), "<i4")

    def score_finish(self, data, global_n):
        e = self.e
        e.check(e.lib.bpf_shard_score_planar_finish(e.h, data.ranges_.ctypes.data_as(C.POINTER(C.c_double)),
                                                    data.angles_.ctypes.data_as(C.POINTER(C.c_double)),
                                                    data.range_count_, data.range_max_, int(global_n)))

    def local_total(self):
        return self._total_view

    def normalize(self, totals, global_n):
        e = self.e
        e.check(e.lib.bpf_shard_normalize_dev(e.h, C.c_void_p(totals.data_ptr()), totals.numel(), int(global_n)))

    def build_cdf(self, flags):
        self.e.check(self.e.lib.bpf_shard_build_cdf(self.e.h, C.c_void_p(flags.data_ptr())))

    def local_sum(self):
        return self._sum_view

    def draw_window(self, rng, m0, m1, sums, sums_are_totals, rank, world, window, flags):
        e = self.e
        e.check(e.lib.bpf_shard_draw_window_dev(e.h, C.c_uint64(rng), m0, m1, C.c_void_p(sums.data_ptr()),
                                                int(sums_are_totals), rank, world, C.c_void_p(window.data_ptr()),
                                                window.shape[1], C.c_void_p(flags.data_ptr())))

    def tail_small(self, x_all, y_all, th_all, m, lo, hi, leaf, bins):
        e = self.e
        e.check(e.lib.bpf_shard_tail_small_dev(e.h, C.c_void_p(x_all.data_ptr()), C.c_void_p(y_all.data_ptr()),
                                               C.c_void_p(th_all.data_ptr()), m, lo, hi, leaf, bins))

    def kld_reset(self):
        self.e.check(self.e.lib.bpf_kld_reset(self.e.h))

    def kld_insert(self, keys_cpu, n):
        k = keys_cpu.numpy()
        assert k.dtype == np.int64 and k.flags.c_contiguous
        self.e.check(self.e.lib.bpf_kld_insert(self.e.h, k.ctypes.data_as(C.c_void_p), 1, k.shape[1], n))

    def kld_feed(self, keys_cpu, n, first):
        stop = C.c_int(-1)
        k = keys_cpu.numpy()
        assert k.dtype == np.int64 and k.flags.c_contiguous
        self.e.check(self.e.lib.bpf_kld_feed(self.e.h, k.ctypes.data_as(C.c_void_p), 1, k.shape[1], n, first,
                                             C.byref(stop)))
        return stop.value

    def kld_feed_window(self, window, n, first):
        """Keys = rows 3..5 of the assembled device window; no torch copy, no stream synchronisation."""
        stop = C.c_int(-1)
        self.e.check(self.e.lib.bpf_kld_feed_dev(self.e.h, C.c_void_p(window.data_ptr()), window.shape[1], n, first,
                                                 C.byref(stop)))
        return stop.value

    def resample_model(self):
        return self.pf.resample_model

    def begin_resample(self, rng, leaf_count):
        """(w_diff, systematic count); resolves the draw chain when w_diff > 0 (multinomial)."""
        w, c = C.c_double(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_begin_resample(self.e.h, C.c_uint64(rng), int(leaf_count), C.byref(w),
                                                         C.byref(c)))
        return w.value, c.value

    def end_resample(self, m):
        """drand48 state after m samples; resets the averages when w_diff > 0."""
        out = C.c_uint64()
        self.e.check(self.e.lib.bpf_shard_end_resample(self.e.h, int(m), C.byref(out)))
        return out.value

    def resample_limit(self, leaf_count):
        out = C.c_int()
        self.e.check(self.e.lib.bpf_pf_resample_limit(self.e.h, int(leaf_count), C.byref(out)))
        return out.value

    def systematic_window(self, rng, count, sums, sums_are_totals, rank, world, window, flags):
        e = self.e
        e.check(e.lib.bpf_shard_systematic_window_dev(e.h, C.c_uint64(rng), count, C.c_void_p(sums.data_ptr()),
                                                      int(sums_are_totals), rank, world,
                                                      C.c_void_p(window.data_ptr()), window.shape[1],
                                                      C.c_void_p(flags.data_ptr())))

    # ---- the systematic resample in place (include/badger_pf.h, bpf_shard_inplace_*)
    def set_resample_form(self, form, max_share):
        self.e.check(self.e.lib.bpf_shard_set_resample_form(self.e.h, int(form), float(max_share)))

    def resample_form(self):
        f, s = C.c_int(), C.c_double()
        self.e.check(self.e.lib.bpf_shard_get_resample_form(self.e.h, C.byref(f), C.byref(s)))
        return f.value, s.value

    def slice(self):
        """(global_first, local_count, form_used) as the last sharded init or resample left this engine's slice."""
        first, n, form = C.c_longlong(), C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_slice(self.e.h, C.byref(first), C.byref(n), C.byref(form)))
        return first.value, n.value, form.value

    def inplace_select(self, rng, count, sums, sums_are_totals, rank, world, flags):
        """(counts of every rank, this rank's global_first, form used); RESAMPLE_WINDOW: the cap applies, nothing
        was changed."""
        counts, first, form = (C.c_int * world)(), C.c_longlong(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_inplace_select_dev(
            self.e.h, C.c_uint64(rng), int(count), C.c_void_p(sums.data_ptr()), int(sums_are_totals), rank, world,
            C.c_void_p(flags.data_ptr()), counts, C.byref(first), C.byref(form)))
        return [int(v) for v in counts], first.value, form.value

    def inplace_xy_sums(self):
        """int64 limb words of the new slice's x / y sums and the flag (engine memory; reduced in place by the
        caller)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.e.check(self.e.lib.bpf_shard_inplace_xy_sums_dev(self.e.h, C.byref(p), C.byref(n)))
        return self._view(p.value, (n.value,))

    def inplace_converged(self, reduced, global_count):
        """one int64 word: this slice's particles near the mean of the reduced sums (reduced in place by the caller)"""
        p = C.c_void_p()
        self.e.check(self.e.lib.bpf_shard_inplace_converged_dev(self.e.h, C.c_void_p(reduced.data_ptr()),
                                                                int(global_count), C.byref(p)))
        return self._view(p.value, (1,))

    def inplace_converged_finish(self, reduced_count, global_count):
        self.e.check(self.e.lib.bpf_shard_inplace_converged_finish(self.e.h, C.c_void_p(reduced_count.data_ptr()),
                                                                   int(global_count)))

    # ---- the multinomial resample in place (include/badger_pf.h, bpf_shard_inplace_mn_*)
    def set_multinomial_form(self, form):
        self.e.check(self.e.lib.bpf_shard_set_multinomial_form(self.e.h, int(form)))

    def multinomial_form(self):
        f = C.c_int()
        self.e.check(self.e.lib.bpf_shard_get_multinomial_form(self.e.h, C.byref(f)))
        return f.value

    def inplace_mn_select(self, rng, sums, sums_are_totals, rank, world, flags):
        """The candidate draws this rank owns, into the set that is not current; returns how many it keeps."""
        n = C.c_int()
        self.e.check(self.e.lib.bpf_shard_inplace_mn_select_dev(
            self.e.h, C.c_uint64(rng), C.c_void_p(sums.data_ptr()), int(sums_are_totals), rank, world,
            C.c_void_p(flags.data_ptr()), C.byref(n)))
        return n.value

    def inplace_mn_bins(self):
        """(int64 [2, n_bins] device tensor: packed keys, first draw indices; key-out-of-range flag)."""
        return self._bins(self.e.lib.bpf_shard_inplace_mn_bins_dev)

    def inplace_mn_stop(self, all_bins, counts, pad):
        """all_bins: int64 [world, 2, pad] gathered lists.  (M, leaf_count, bin_count, counts of every rank, this rank's
        global_first, form used); RESAMPLE_WINDOW: the cap applies, nothing was changed."""
        W = len(counts)
        c = (C.c_int * W)(*[int(v) for v in counts])
        m, leaf, bins, first, form = C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_int()
        out = (C.c_int * W)()
        self.e.check(self.e.lib.bpf_shard_inplace_mn_stop_dev(
            self.e.h, C.c_void_p(all_bins.data_ptr()), c, W, int(pad), C.byref(m), C.byref(leaf), C.byref(bins), out,
            C.byref(first), C.byref(form)))
        return m.value, leaf.value, bins.value, [int(v) for v in out], first.value, form.value

    # ---- rebalancing the slices (include/badger_pf.h, bpf_shard_rebalance_*)
    def set_rebalance(self, mode, trigger_share):
        self.e.check(self.e.lib.bpf_shard_set_rebalance(self.e.h, int(mode), float(trigger_share)))

    def rebalance_setting(self):
        m, t = C.c_int(), C.c_double()
        self.e.check(self.e.lib.bpf_shard_get_rebalance(self.e.h, C.byref(m), C.byref(t)))
        return m.value, t.value

    def rebalance_last(self):
        """Samples the last rebalance of this engine moved over all ranks (0: the last AUTO resample found none)."""
        t = C.c_longlong()
        self.e.check(self.e.lib.bpf_shard_rebalance_last(self.e.h, C.byref(t)))
        return t.value

    def rebalance_plan(self, counts, rank, world):
        """(out[] of every rank, this rank's new global_first, its new count); the plan is recorded in the engine."""
        c = (C.c_longlong * len(counts))(*[int(v) for v in counts])
        out, first, n = (C.c_longlong * max(int(world), 1))(), C.c_longlong(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_rebalance_plan(self.e.h, c, int(rank), int(world), out, C.byref(first),
                                                         C.byref(n)))
        return [int(v) for v in out][:int(world)], first.value, n.value

    def rebalance_export(self):
        """int64 [4, out[rank]] device view: the bits of x / y / theta / w of this rank's outgoing samples."""
        p, n = C.c_void_p(), C.c_longlong()
        self.e.check(self.e.lib.bpf_shard_rebalance_export_dev(self.e.h, C.byref(p), C.byref(n)))
        return self._view(p.value, (4, n.value))

    def rebalance_import(self, rows, rank_off, row_stride):
        """rows: the gathered int64 rows (None when nothing moves anywhere); rank q's row k at
        rank_off[q] + k * row_stride."""
        if rows is None:
            return self.e.check(self.e.lib.bpf_shard_rebalance_import_dev(self.e.h, None, None, 0))
        assert rows.dtype == torch.int64 and rows.is_contiguous()
        off = (C.c_longlong * len(rank_off))(*[int(v) for v in rank_off])
        self.e.check(self.e.lib.bpf_shard_rebalance_import_dev(self.e.h, C.c_void_p(rows.data_ptr()), off,
                                                               int(row_stride)))

    def kld_insert_window(self, window, n):
        self.e.check(self.e.lib.bpf_kld_insert_dev(self.e.h, C.c_void_p(window.data_ptr()), window.shape[1], n))

    def local_pose_keys(self):
        """int64 [3, n_local] histogram keys of the local poses (floor(pose / cell), pf_kdtree.cpp:52-54)."""
        s = self.pf.getCurrentSet().samples
        k = np.stack([np.floor(s[:, 0] / 0.5), np.floor(s[:, 1] / 0.5), np.floor(s[:, 2] / (10 * np.pi / 180))])
        return torch.from_numpy(k.astype(np.int64)).to(self.device)

    kld_device_min = 8192  # draws left after the first window from which the device tree takes the whole stream

    def kld_stop_window(self, window, n):
        """Stop rule for the whole stream on the device: (handled, stop or -1, leaf_count, bin_count)."""
        h, stop, leaf, bins = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_kld_stop_dev(self.e.h, C.c_void_p(window.data_ptr()), window.shape[1], n,
                                                 C.byref(h), C.byref(stop), C.byref(leaf), C.byref(bins)))
        return bool(h.value), stop.value, leaf.value, bins.value

    def kld_counts(self):
        a, b = C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_kld_leaf_count(self.e.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def adopt(self, x, y, th, count, global_m, leaf, bins):
        e = self.e
        e.check(e.lib.bpf_shard_adopt_dev(e.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                          C.c_void_p(th.data_ptr()), count, global_m, leaf, bins))

    def converged(self, x_all, y_all, m):
        e = self.e
        e.check(e.lib.bpf_shard_converged_dev(e.h, C.c_void_p(x_all.data_ptr()), C.c_void_p(y_all.data_ptr()), m))

    def skip(self, state, n):
        return int(self.e.lib.bpf_drand48_skip(C.c_uint64(state), C.c_uint64(n)))

    # ---- cluster statistics of the global set (include/badger_pf.h, bpf_shard_stats_*)
    def stats_local_soa(self):
        """float64 [4, n_local] device tensor: x, y, theta, weight of the slice (a copy; the gather pads it)."""
        p = [C.c_void_p() for _ in range(4)]
        n = C.c_int()
        self.e.check(self.e.lib.bpf_shard_samples_dev(self.e.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]),
                                                      C.byref(p[3]), C.byref(n)))
        return torch.stack([self._view(q.value, (n.value,), "<f8") for q in p])

    def stats_gathered(self, soa, global_n):
        """Gathered form on the whole set [4, global_n]: 1 installed, 0 declined (too many bins / clusters),
        -1 host route."""
        h = C.c_int()
        self.e.check(self.e.lib.bpf_shard_stats_gathered_dev(
            self.e.h, C.c_void_p(soa[0].data_ptr()), C.c_void_p(soa[1].data_ptr()), C.c_void_p(soa[2].data_ptr()),
            C.c_void_p(soa[3].data_ptr()), int(global_n), C.byref(h)))
        return h.value

    def stats_local_bins(self, global_first):
        """(int64 [2, n_bins] device tensor: packed keys, global first indices; host-route flag)."""
        return self._bins(self.e.lib.bpf_shard_stats_local_bins_dev, int(global_first))

    def stats_label(self, all_bins, counts, pad):
        """all_bins: int64 [world, 2, pad] gathered lists; returns the global cluster count."""
        c = (C.c_int * len(counts))(*[int(v) for v in counts])
        out = C.c_int()
        self.e.check(self.e.lib.bpf_shard_stats_label_dev(self.e.h, C.c_void_p(all_bins.data_ptr()), c, len(counts),
                                                          int(pad), C.byref(out)))
        return out.value

    def stats_local_sums(self):
        """int64 limb words of the slice's per-cluster sums (engine memory; reduced in place by the caller)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.e.check(self.e.lib.bpf_shard_stats_local_sums_dev(self.e.h, C.byref(p), C.byref(n)))
        return self._view(p.value, (n.value,))

    def stats_finish(self, reduced):
        """False: the reduced sums do not fit the fixed-point format (a frame far from the origin) and nothing was
        installed -- on every rank alike; the host route takes over."""
        self.e.check(self.e.lib.bpf_shard_stats_finish_dev(self.e.h, C.c_void_p(reduced.data_ptr())))
        ok = C.c_int()
        self.e.check(self.e.lib.bpf_shard_stats_finish_installed(self.e.h, C.byref(ok)))
        return bool(ok.value)

    def stats_local_samples_host(self):
        """numpy [n_local, 4] copy of the slice (the host route only)."""
        return self.pf.getCurrentSet().samples

    def stats_host(self, all_samples):
        a = np.ascontiguousarray(all_samples, dtype=np.float64)
        self.e.check(self.e.lib.bpf_shard_stats_host(self.e.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0]))

    def stats_result(self):
        return self.pf.computeClusterStats()

    def stats_cluster(self, k):
        return self.pf.getClusterStats(k)

    def stats_max_weight_pose(self):
        return self.pf.getMaxWeightPose()

    # ---- the particle cloud of the global set (include/badger_pf.h, bpf_shard_pose_rows_dev and the calls around it)
    def pose_rows(self, global_first, first, stride):
        """int64 [3, n_sel] device view: x / y / theta bits of the slice's samples that the selection first,
        first + stride, ... of the GLOBAL index space picks (engine memory, valid until the next pose-array call)."""
        p, n = C.c_void_p(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_pose_rows_dev(self.e.h, int(global_first), int(first), int(stride),
                                                        C.byref(p), C.byref(n)))
        return self._view(p.value, (3, n.value))

    def pose_array_from_rows(self, rows, n):
        """rows: int64 [3, >= n] device tensor of gathered rows in global order; the [n, 7] float64 pose array."""
        out = np.empty((max(int(n), 1), 7), dtype=np.float64)
        assert rows.dtype == torch.int64 and rows.shape[0] == 3 and rows.stride(1) == 1 and rows.shape[1] >= n
        self.e.check(self.e.lib.bpf_pose_array_from_rows_dev(
            self.e.h, C.c_void_p(rows.data_ptr()), int(rows.stride(0)) if n else 0, int(n),
            out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[0]))
        return out[:int(n)]

    def get_pose_array_all(self, root, first, stride, room):
        """The whole query over the engine's own exchange (mailbox): the [count, 7] array where this rank receives,
        else None."""
        receives = root < 0 or root == self._mb_rank
        out = np.empty((max(int(room), 1), 7), dtype=np.float64) if receives else None
        n = C.c_int()
        self.e.check(self.e.lib.bpf_shard_get_pose_array(
            self.e.h, int(root), int(first), int(stride),
            out.ctypes.data_as(C.POINTER(C.c_double)) if receives else None, int(room), C.byref(n)))
        return out[:n.value] if receives else None

    # ---- a sharded set initialised on its ranks, and the global set's tree (include/badger_pf.h, bpf_shard_init_*,
    # bpf_shard_tree_*)
    @staticmethod
    def _gauss_args(mean, rotation, sigma):
        m, r, d = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (mean, rotation, sigma))
        assert m.size == 3 and r.size == 9 and d.size == 3
        dp = C.POINTER(C.c_double)
        return (m, r, d), (m.ctypes.data_as(dp), r.ctypes.data_as(dp), d.ctypes.data_as(dp))

    def init_gaussian(self, mean, rotation, sigma, global_first, local_count, global_count):
        keep, ptr = self._gauss_args(mean, rotation, sigma)
        self.e.check(self.e.lib.bpf_shard_init_with_gaussian(self.e.h, ptr[0], ptr[1], ptr[2], int(global_first),
                                                             int(local_count), int(global_count)))

    def init_random_poses(self, global_first, local_count, global_count):
        self.e.check(self.e.lib.bpf_shard_init_with_random_poses(self.e.h, int(global_first), int(local_count),
                                                                 int(global_count)))

    def init_mixture(self, components, global_first, local_count, global_count):
        """bpf_shard_init_with_mixture: the components' counts are those of the GLOBAL set."""
        comps, ptr = mixture_components(components)
        self.e.check(self.e.lib.bpf_shard_init_with_mixture(self.e.h, ptr, comps.shape[0], int(global_first),
                                                            int(local_count), int(global_count)))

    def init_mixture_all(self, components):
        comps, ptr = mixture_components(components)
        self.e.check(self.e.lib.bpf_shard_init_with_mixture_all(self.e.h, ptr, comps.shape[0]))
        return self.global_leaf_count()

    def init_gaussian_all(self, mean, rotation, sigma):
        """The init and the global tree over the engine's own exchange (mailbox): (leaf_count, bin_count)."""
        keep, ptr = self._gauss_args(mean, rotation, sigma)
        self.e.check(self.e.lib.bpf_shard_init_with_gaussian_all(self.e.h, ptr[0], ptr[1], ptr[2]))
        return self.global_leaf_count()

    def init_random_poses_all(self):
        self.e.check(self.e.lib.bpf_shard_init_with_random_poses_all(self.e.h))
        return self.global_leaf_count()

    # ---- pose search over the ranks (include/badger_pf.h, bpf_shard_search_poses and its three siblings)
    def exchange_mode(self):
        """bpf_shard_exchange_mode: 0 while the engine has no exchange of its own (mailbox, RCCL or a local world)"""
        m = C.c_int(-1)
        self.e.check(self.e.lib.bpf_shard_exchange_mode(self.e.h, C.byref(m)))
        return m.value

    def _search_all(self, k, call):
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n, st = C.c_int(), _lib.PoseSearchStats()
        self.e.check(call(hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n), C.byref(st)))
        return hits[:n.value], {name: getattr(st, name) for name, _ in _lib.PoseSearchStats._fields_}

    def search_poses_all(self, data, headings, cell_stride, k, first, count):
        """The whole sharded search over the engine's own exchange: the rows (planar scan or cloud by the data)."""
        if hasattr(data, "points_"):
            pts = data.points_
            return self._search_all(k, lambda hits, n, st: self.e.lib.bpf_shard_cloud_search_poses(
                self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], int(headings), int(cell_stride),
                int(first), int(count), int(k), hits, n))[0]
        rp, ap = data.pointers()
        return self._search_all(k, lambda hits, n, st: self.e.lib.bpf_shard_search_poses(
            self.e.h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(first),
            int(count), int(k), hits, n))[0]

    def search_poses_pruned_all(self, data, headings, cell_stride, k, block, first_block, block_count):
        """The pruned sharded search over the engine's own exchange: (rows, this rank's stats)."""
        if hasattr(data, "points_"):
            pts = data.points_
            return self._search_all(k, lambda hits, n, st: self.e.lib.bpf_shard_cloud_search_poses_pruned(
                self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], int(headings), int(cell_stride),
                int(block), int(first_block), int(block_count), int(k), hits, n, st))
        rp, ap = data.pointers()
        return self._search_all(k, lambda hits, n, st: self.e.lib.bpf_shard_search_poses_pruned(
            self.e.h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(block),
            int(first_block), int(block_count), int(k), hits, n, st))

    def global_leaf_count(self):
        a, b = C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_global_leaf_count(self.e.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tree_local_bins(self, global_first):
        """(int64 [2, n_bins] device tensor: packed keys, global first indices; key-out-of-range flag)."""
        return self._bins(self.e.lib.bpf_shard_tree_local_bins_dev, int(global_first))

    def tree_merge(self, all_bins, counts, pad):
        """all_bins: int64 [world, 2, pad] gathered lists; installs and returns (leaf_count, bin_count)."""
        c = (C.c_int * len(counts))(*[int(v) for v in counts])
        a, b = C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_tree_merge_dev(self.e.h, C.c_void_p(all_bins.data_ptr()), c, len(counts),
                                                         int(pad), C.byref(a), C.byref(b)))
        return a.value, b.value

    def tree_local_keys(self):
        """int64 [3, n_local] device tensor: the raw histogram keys of the slice (the keys route only)."""
        p, n = C.c_void_p(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_tree_local_keys_dev(self.e.h, C.byref(p), C.byref(n)))
        return self._view(p.value, (n.value, 3), "<i4").to(torch.int64).t().contiguous()

    def tree_from_keys(self, all_keys):
        """all_keys: int [global_n, 3] on the host, in index order; installs and returns (leaf_count, bin_count)."""
        k = np.ascontiguousarray(all_keys, dtype=np.int32)
        a, b = C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_shard_tree_from_keys(self.e.h, k.ctypes.data_as(C.POINTER(C.c_int)), k.shape[0],
                                                         C.byref(a), C.byref(b)))
        return a.value, b.value

    def tree_last_route(self):
        r = C.c_int()
        self.e.check(self.e.lib.bpf_shard_tree_last_route(self.e.h, C.byref(r)))
        return r.value

    def rng_state(self):
        return self.pf.getRngState()

    def set_rng_state(self, s):
        self.pf.setRngState(s)

    def update_action(self, odom, data, global_first, global_count):
        odom.updateActionShard(data, global_first, global_count)

    def max_samples(self):
        return self.pf.max_samples

    def max_beams(self):
        return getattr(self.sc, "max_beams", 2)

    def set_random_pose_generator(self, mode):
        self.pf.setRandomPoseGenerator(mode)

    def set_uniform_pose_check(self, threshold, multiplier, scoring):
        self.pf.setUniformPoseCheck(threshold, multiplier, scoring)

    def set_kld_count(self, mode):
        self.pf.setKldCount(mode)

    def kld_count(self):
        return self.pf.getKldCount()

    def state(self):
        return self.pf.getState()


def pose_selection(counts, first, stride):
    """Which samples of every slice the selection first, first + stride, ... of the global index space picks: per rank
    (local index of the first selected sample, number selected), from the ranks' sample counts alone."""
    if stride < 1 or first < 0:
        raise ValueError("pose_selection: first >= 0 and stride >= 1")
    out, at = [], 0
    for n in counts:
        i0 = (stride - (at - first) % stride) % stride if at >= first else first - at
        out.append((i0, (n - i0 + stride - 1) // stride if i0 < n else 0))
        at += n
    return out


RESAMPLE_WINDOW, RESAMPLE_IN_PLACE = 0, 1  # BPF_SHARD_RESAMPLE_*
RESAMPLE_FORMS = {"window": RESAMPLE_WINDOW, "in_place": RESAMPLE_IN_PLACE}
REBALANCE_MODES = {"off": 0, "auto": 1}  # BPF_SHARD_REBALANCE_*
TREE_ROUTES = {1: "device", 2: "host", 3: "bins", 4: "keys"}  # BPF_SHARD_TREE_ROUTE_*


def check_settings(resample_form, multinomial_form, rebalance):
    """The settings ShardedFilter and LocalShardedFilter share; the library's codes of the three."""
    if resample_form not in RESAMPLE_FORMS:
        raise ValueError("resample_form: window or in_place")
    if multinomial_form not in RESAMPLE_FORMS:
        raise ValueError("multinomial_form: window or in_place")
    if rebalance not in REBALANCE_MODES:
        raise ValueError("rebalance: off or auto")
    return RESAMPLE_FORMS[resample_form], RESAMPLE_FORMS[multinomial_form], REBALANCE_MODES[rebalance]


def check_kld_modes(who, modes):
    """Every rank computes the same stop rule, so every rank must count the same way; the mode."""
    if len(set(int(m) for m in modes)) != 1:
        raise ValueError("%s: the ranks use different KLD count modes %s" % (who, modes))
    return int(modes[0])


def mixture_of_hits(scanner, data, hits, total_count, refine, moments, mixture):
    """What localize() runs on a rank between the search and the init: refinePoses, poseMoments, mixtureFromHits and
    mixtureApplyMoments, as one engine would run them; the components."""
    refined = scanner.refinePoses(data, hits, *refine)
    xy_radius, xy_step, theta_radius, theta_step, baseline, sigma_floor, sigma_cap = moments
    rows = scanner.poseMoments(data, refined, xy_radius, xy_step, theta_radius, theta_step, baseline)
    return mixtureApplyMoments(mixtureFromHits(refined, total_count, *mixture), rows, sigma_floor, sigma_cap)


def even_counts(n, W):
    """The even split of n samples over W ranks in global order: rank r holds [n r / W, n (r + 1) / W)."""
    return [(n * (r + 1)) // W - (n * r) // W for r in range(W)]


def resample_window_for(x):
    """A resample window for a stop expected x draws ahead: a quarter more, in whole 1024s (csrc/resample_plan.hpp)."""
    return max(1024, (x + x // 4 + 1023) // 1024 * 1024)


class ShardedState:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class ShardedFilter:
    """ParticleFilter::updateSensor / updateResample over W shards (see module docstring)."""

    def __init__(self, backend, dist, rank=None, world=None, first_window=4096, exchange="auto",
                 mailbox_timeout_ms=None, kld_count=None, init_follows=False, resample_form="window", max_share=2.0,
                 rebalance="off", trigger_share=1.5, multinomial_form="window"):
        """multinomial_form: "window" (the default) or "in_place": the MULTINOMIAL resampler resamples every slice into
        itself (include/badger_pf.h, bpf_shard_set_multinomial_form): every rank keeps the candidate draws of its own
        slice, the stop index comes from the ranks' bin lists, and the concatenation of the slices is the reference's
        set sorted stably by the owner of each draw.  max_share and rebalance apply to it as to the systematic form;
        a key outside the packing sends that resample to the window form too.  Every rank passes the same.
        resample_form: "window" (every rank receives the draw window and keeps an even cut) or "in_place": the
        systematic resampler resamples every slice into itself (include/badger_pf.h, bpf_shard_set_resample_form) --
        self.counts is uneven afterwards, the concatenation of the slices is the reference's set with the wrapped
        teeth moved to the front.  When the largest slice would exceed max_share * ceil(M / W) that resample takes the
        window form; self.form_used tells.  The multinomial resampler ignores the setting.  Every rank passes the same.
        rebalance: "off", or "auto": an in-place resample is never sent to the window form, and when its largest slice
        exceeds trigger_share * ceil(M / W) (a policy condition, default 1.5, >= 1) the slices go back to the even
        split in global order (rebalance(); self.rebalanced tells how many samples moved).  form_used stays "in_place".
        init_follows: the caller starts the set with init_with_gaussian / init_with_random_poses next, so the tree
        of whatever the engines hold now is not built (it matters to the systematic resampler only).
        kld_count: what the KLD stop rule counts, pf.KLD_COUNT_LEAVES or pf.KLD_COUNT_BINS (None: the backend's
        current mode).  Every rank must use the same mode; the constructor checks it over the process group."""
        self.b = backend
        self.mailbox_timeout_ms = mailbox_timeout_ms
        self.recoveries = 0  # exchanges that ran out of time and were finished over the collectives
        self._step = 0       # resamples completed (the ranks compare it when they recover)
        self.dist = dist
        self.rank = dist.get_rank() if rank is None else rank
        self.world = dist.get_world_size() if world is None else world
        self.device = backend.device
        self.cpu_collectives = dist.get_backend() == "gloo" and torch.device(self.device).type != "cpu"
        self._nccl = not self.cpu_collectives and dist.get_backend() == "nccl"
        self._gather_out = {}
        self._pose_views = {}
        self.max_global = backend.max_samples()  # engines are created with the GLOBAL min / max sample counts
        n = torch.tensor([backend.n_local()], dtype=torch.int64, device=self.device)
        self.counts = [int(v) for v in self._all_gather(n).cpu().tolist()]
        # every rank computes the same stop rule from the same window, so every rank must count the same way
        if kld_count is not None:
            backend.set_kld_count(int(kld_count))
        self.kld_count = int(backend.kld_count()) if hasattr(backend, "kld_count") else 0
        modes = self._all_gather(torch.tensor([self.kld_count], dtype=torch.int64, device=self.device)).cpu().tolist()
        check_kld_modes("ShardedFilter", modes)
        form, mn_form, rebalance_code = check_settings(resample_form, multinomial_form, rebalance)
        self.resample_form, self.max_share = resample_form, float(max_share)
        self.form_used = "window"  # of the last resample
        if resample_form != "window" or hasattr(backend, "set_resample_form"):
            backend.set_resample_form(form, self.max_share)
        self.multinomial_form = multinomial_form
        if multinomial_form != "window" or hasattr(backend, "set_multinomial_form"):
            backend.set_multinomial_form(mn_form)
        self.rebalance_mode, self.trigger_share = rebalance, float(trigger_share)
        self.rebalanced = 0  # samples the last rebalance moved (0: the last resample needed none)
        if rebalance != "off" or hasattr(backend, "set_rebalance"):
            backend.set_rebalance(rebalance_code, self.trigger_share)
        # ranks that took different forms would wait in different exchanges: every rank must pass the same
        mine = torch.tensor([float(form), self.max_share, float(rebalance_code), self.trigger_share, float(mn_form)],
                            dtype=torch.float64, device=self.device)
        forms = self._all_gather(mine).reshape(self.world, 5).cpu().tolist()
        if any(f != forms[0] for f in forms):
            raise ValueError("ShardedFilter: the ranks use different resample forms / max_share / rebalance settings %s"
                             % forms)
        self.window_hint = self._first_window = first_window
        self.tree_route = None  # how the last init found the global leaf count: "device", "host", "bins" or "keys"
        self.out = torch.zeros((3, self.max_global), dtype=torch.float64, device=self.device)
        self.flags = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._windows = {}
        self.sample_count = sum(self.counts)
        self.leaf_count = self.bin_count = 0
        self.windows_used = 0
        self.totals = None  # per-shard weight totals of the last update_sensor (None: weights changed since)
        self._stats_valid = False  # the backend holds the statistics of the current GLOBAL set
        self.stats_route = None    # how the last statistics were evaluated: "gathered", "distributed" or "host"
        self._fused_totals = False  # the last update_sensor went through the engine's one-call mailbox form
        # exchange: "mailbox" = peer stores through IPC-mapped device memory (all ranks on one node), "collective" =
        # torch.distributed all-gather / all-reduce, "auto" = mailbox when every rank could set it up
        self.mailbox = False
        # what the bring-up found: "pass" (every rank created, mapped, completed the connect round and verified the
        # four self-test windows cell by cell), "fail: <stage>" (some rank did not; the collectives carry the
        # exchanges), "not run" (collectives requested)
        self.mailbox_verdict = "not run"
        if exchange not in ("auto", "mailbox", "collective"):
            raise ValueError("exchange: auto, mailbox or collective")
        if exchange != "collective" and hasattr(backend, "mailbox_create") and self.world <= 16:
            self.mailbox = self._setup_mailbox()
        if exchange == "mailbox" and not self.mailbox:
            raise RuntimeError("mailbox exchange requested but not every rank could set it up")
        if backend.resample_model() == 1 and not init_follows:
            # the systematic resampler sizes the new set from the leaf count of the CURRENT set's tree, which the
            # reference builds when the set is created (not after motion updates): take it now
            self._global_leaf_count()

    def _all_agree(self, ok):
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        if self.cpu_collectives:
            h = t.cpu()
            self.dist.all_reduce(h, op=self.dist.ReduceOp.MIN)
            return int(h.item()) == 1
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return int(t.item()) == 1

    def _setup_mailbox(self):
        """True when every rank created its mailbox, mapped all the others and completed a round with them."""
        b = self.b
        if self.mailbox_timeout_ms is not None and hasattr(b, "mailbox_set_timeout_ms"):
            b.mailbox_set_timeout_ms(self.mailbox_timeout_ms)
        handle = b.mailbox_create(self.rank, self.world, self.max_global)
        mine = torch.tensor(list(handle if handle is not None else bytes(64)), dtype=torch.uint8, device=self.device)
        handles = self._all_gather(mine).cpu().numpy().tobytes()
        stage = "create / IPC export"
        ok = self._all_agree(handle is not None)
        if ok:
            stage = "IPC map + connect round"
            ok = self._all_agree(b.mailbox_connect(handles))
        if ok:
            # the words arrive; do the window cells?  (a peer's stores must be visible behind this GPU's caches)
            stage = "window self-test"
            ok = self._all_agree(b.mailbox_selftest())
        if not ok:
            b.mailbox_destroy()
        self.mailbox_verdict = "pass" if ok else "fail: " + stage
        return ok

    def use_collectives(self):
        """Drop the mailbox and carry the exchanges over torch.distributed from the next update on (bench.py times
        the same filter once per exchange; every rank calls this between two steps)."""
        if self.mailbox:
            self.b.mailbox_destroy()
        self.mailbox = False
        self._drop_exchange_caches()

    def try_mailbox(self):
        """(Re-)establish the mailbox between two steps; True when every rank could."""
        if not self.mailbox and hasattr(self.b, "mailbox_create") and self.world <= 16:
            self._drop_exchange_caches()
            self.mailbox = self._setup_mailbox()
        return self.mailbox

    def _drop_totals(self):
        """The weights changed (or are about to): the totals of the last update_sensor no longer describe them."""
        self.totals = None
        self._fused_totals = False

    def _drop_exchange_caches(self):
        """What belongs to the exchange in use: the window buffers, the views into them, the totals it delivered."""
        self._windows.clear()
        self._pose_views.clear()
        self._drop_totals()

    # ---- a mailbox wait ran out of time (a rank stalled: page-in, debugger, a long host pause)
    def _is_exchange_error(self, err):
        return getattr(err, "code", None) == 9  # BPF_ERR_EXCHANGE

    def _recover_exchange(self, committed=False):
        """Every rank gets here after its OWN wait has run out (the rank that stalled finds its peers gone one
        exchange later), so the collectives below are reached by all of them.  The engine's rule (badger_pf.h): after a
        failed wait for the totals the weights are scored but NOT normalised and the local total is in the scalars;
        a failed window wait has changed nothing of the current set.  So: drop the mailbox, all-gather the local
        totals, normalise where that was still due, and go on with the collectives -- the interrupted resample is
        simply run again over them.  The mailbox is set up afresh after the step.
        One exception to "a failed window wait has changed nothing", with rebalance="auto": the one-call resample can
        fail AFTER its resample became current, in the rebalance behind it (backend.resample_committed()).  Then
        `committed` is passed: the resample is NOT run again -- it would draw from the new set with stale counts and
        advance the rng a second time.  The weights are 1 / M and there are no totals to rebuild; the caller refreshes
        the counts from the engines and runs only the staged rebalance()."""
        b = self.b
        totals_failed, _ = b.mailbox_error_stage()
        # meeting point of the ranks, and a check that they are recovering the same step (a time-out that fell
        # within microseconds of the awaited word can leave them a step apart: that is reported, not papered over)
        steps = self._all_gather(torch.tensor([self._step], dtype=torch.int64, device=self.device)).cpu().tolist()
        if len(set(int(v) for v in steps)) != 1:
            raise RuntimeError("sharded filter: the ranks fell out of step around a mailbox time-out: %r" % (steps,))
        b.mailbox_destroy()
        self.mailbox = False
        self._drop_exchange_caches()
        if not committed:
            totals = self._all_gather(b.local_total()).clone()
            if totals_failed:
                b.normalize(totals, self.sample_count)
            self.totals = totals
        self.recoveries += 1
        self._remake_mailbox = True

    # ---- collectives (device tensors with nccl; staged through the host only for gloo + GPU)
    def _all_gather(self, t):
        if self._nccl:
            # one output buffer per shape, reused: the callers consume the result before the next gather of that shape
            key = (t.numel(), t.dtype)
            out = self._gather_out.get(key)
            if out is None:
                out = self._gather_out[key] = torch.empty(self.world * t.numel(), dtype=t.dtype, device=t.device)
            self.dist.all_gather_into_tensor(out, t if t.is_contiguous() else t.contiguous())
            return out
        src = t.cpu() if self.cpu_collectives else t
        outs = [torch.empty_like(src) for _ in range(self.world)]
        self.dist.all_gather(outs, src.contiguous())
        res = torch.cat(outs)
        return res.to(self.device) if self.cpu_collectives else res

    def _all_reduce_sum(self, t):
        if self.cpu_collectives:
            h = t.cpu()
            self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM)
            t.copy_(h)
        else:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t

    def _window(self, key, count):
        """The [6, >= count] int64 draw window of the next exchange."""
        if self.mailbox:
            return self.b.mailbox_window()
        window = self._windows.get(key)
        if window is None:
            window = self._windows[key] = torch.zeros((6, count), dtype=torch.int64, device=self.device)
        return window

    def _assemble(self, window):
        """Every shard's columns into every shard's window: nothing to do with a mailbox (the draw kernel stored
        them into all peers, the window's first consumer waits for them), one integer all-reduce otherwise."""
        if not self.mailbox:
            self._all_reduce_sum(window)

    def _pose_rows(self, window):
        """(x, y, theta) float64 row views of a window buffer; the buffers live in self._windows, so are the views."""
        v = self._pose_views.get(id(window))
        if v is None:
            p = window[0:3].view(torch.float64)
            v = self._pose_views[id(window)] = (p[0], p[1], p[2], window)  # keeps the buffer alive with its id
        return v

    # ---- initWithGaussian / initWithPoseFn over the shards (particle_filter.cpp:105-163): no exchange for the poses
    TREE_ROUTES = TREE_ROUTES

    def init_with_gaussian(self, mean, rotation, sigma):
        """ParticleFilter::initWithGaussian given PDFGaussian's decomposition (cr_ row-major 3x3, cd_): every rank
        passes the same arguments and holds the same rng state; rank r ends with samples [G r / W, G (r + 1) / W) of
        the max_samples = G samples one engine would hold."""
        if self.mailbox and hasattr(self.b, "init_gaussian_all"):
            return self._after_init(*self.b.init_gaussian_all(mean, rotation, sigma))
        lo, n = self._even_share()
        self.b.init_gaussian(mean, rotation, sigma, lo, n, self.max_global)
        self._after_init(*self._global_tree())

    def init_with_mixture(self, components):
        """ParticleFilter.initWithMixture over the shards (a MIXTURE_COMPONENT_DTYPE array whose counts sum to
        max_samples = G): every rank passes the same components and holds the same rng state; rank r ends with
        samples [G r / W, G (r + 1) / W) of the set one engine would hold."""
        if self.mailbox and hasattr(self.b, "init_mixture_all"):
            return self._after_init(*self.b.init_mixture_all(components))
        lo, n = self._even_share()
        self.b.init_mixture(components, lo, n, self.max_global)
        self._after_init(*self._global_tree())

    def init_with_random_poses(self):
        """ParticleFilter::initWithPoseFn with the generator of set_random_pose_generator (global localisation)."""
        if self.mailbox and hasattr(self.b, "init_random_poses_all"):
            return self._after_init(*self.b.init_random_poses_all())
        lo, n = self._even_share()
        self.b.init_random_poses(lo, n, self.max_global)
        self._after_init(*self._global_tree())

    def _even_share(self):
        G = self.max_global
        self.counts = self._even_counts(G)
        self.sample_count = G
        return (G * self.rank) // self.world, self.counts[self.rank]

    def _even_counts(self, n):
        return even_counts(n, self.world)

    def _after_init(self, leaf, bins):
        self._even_share()
        self.leaf_count, self.bin_count = leaf, bins
        self._drop_totals()
        self._stats_valid = False
        self.window_hint = self._first_window
        self.windows_used = 0
        if hasattr(self.b, "tree_last_route"):
            self.tree_route = self.TREE_ROUTES.get(self.b.tree_last_route())

    def _exchange_bin_lists(self, bins, flag):
        """The ranks' bin lists of a merge stage (shard_exchange_bin_lists in abi_shard_node.inl): (bin_counts,
        any_flag, all_bins, pad).  Every rank's (n_bins, flag) pair crosses first; any_flag: some rank raised its
        flag -- it travelled with the counts, so every rank turns off to its caller's other route here together, and
        no list crosses (all_bins is None).  Otherwise all_bins = int64 [world, 2, pad], zero-filled."""
        meta = torch.tensor([bins.shape[1], 1 if flag else 0], dtype=torch.int64, device=self.device)
        meta = self._all_gather(meta).reshape(self.world, 2).cpu().tolist()
        bin_counts = [int(m[0]) for m in meta]
        if any(int(m[1]) for m in meta):
            return bin_counts, True, None, max(max(bin_counts), 1)
        all_bins, pad = self._gather_ragged(bins, bin_counts)
        return bin_counts, False, all_bins.contiguous(), pad

    def _concat_ragged(self, allv, counts):
        """[world, rows, pad] of _gather_ragged without its padding: [rows, sum(counts)] in rank order."""
        return torch.cat([allv[r, :, :counts[r]] for r in range(self.world)], dim=1)

    def _global_tree(self):
        """Leaf and bin count of the tree of the whole set from the ranks' bin lists (self.counts describes the
        slices); installed in the backend."""
        b = self.b
        bin_counts, out_of_range, all_bins, pad = self._exchange_bin_lists(
            *b.tree_local_bins(sum(self.counts[:self.rank])))
        if out_of_range:
            # the keys route: every raw key of the global set, in index order, through the host tree
            allk, _ = self._gather_ragged(b.tree_local_keys(), self.counts)
            return b.tree_from_keys(self._concat_ragged(allk.cpu(), self.counts).t().contiguous().numpy())
        return b.tree_merge(all_bins, bin_counts, pad)

    # ---- motion update (Odom::updateAction): no exchange
    def update_action(self, odom, data):
        self._stats_valid = False
        first = sum(self.counts[:self.rank])
        self.b.update_action(odom, data, first, self.sample_count)

    # ---- Seam A
    def update_sensor(self, data):
        self._stats_valid = False
        if self.mailbox and not hasattr(data, "points_") and hasattr(self.b, "mailbox_update_sensor"):
            # mailbox: the exchange is inside the kernels, so the whole update is one call into the engine
            if self.b.mailbox_update_sensor(data, self.sample_count):
                if self.b.max_beams() < 2:
                    # PlanarScanner::updateSensor is a no-op then (planar_scanner.cpp:128-129): nothing was posted
                    return self._drop_totals()
                self.totals = self.b.mailbox_totals()
                self._fused_totals = True
                return
            # beam skipping: the counting pass has run; sum its counts over the shards and finish stage by stage
            counts = self.b.beam_counts()
            self._all_reduce_sum(counts)
            self.b.score_finish(data, self.sample_count)
            self.totals = self.b.mailbox_totals()
            self.b.normalize(self.totals, self.sample_count)
            self._fused_totals = False
            return
        self._fused_totals = False
        counts = self.b.score(data)
        if counts is not None:
            # prob model with beam skipping: one extra all-reduce of max_beams int32 between its two passes
            self._all_reduce_sum(counts)
            self.b.score_finish(data, self.sample_count)
        # mailbox: the scoring stage has already stored this rank's total into every peer, normalize waits in-kernel
        self.totals = self.b.mailbox_totals() if self.mailbox else self._all_gather(self.b.local_total())
        self.b.normalize(self.totals, self.sample_count)

    def _global_leaf_count(self):
        """Leaf count of the kd-tree of the whole current set (what set_a->kdtree->getLeafCount() is for the
        reference's systematic resampler): known after a resample, otherwise built once from all shards' keys."""
        if self.leaf_count > 0:
            return self.leaf_count
        b = self.b
        pad = max(self.counts)
        mine = torch.zeros((3, pad), dtype=torch.int64, device=self.device)
        k = b.local_pose_keys()
        mine[:, :k.shape[1]] = k
        allk = self._all_gather(mine.reshape(-1)).reshape(self.world, 3, pad).cpu()
        b.kld_reset()
        for r in range(self.world):
            if self.counts[r]:
                b.kld_insert(allk[r, :, :self.counts[r]].contiguous(), self.counts[r])
        self.leaf_count, self.bin_count = b.kld_counts()
        return self.leaf_count

    # ---- Seam B, systematic (particle_filter.cpp:269-354, w_diff == 0)
    def _update_resample_systematic(self):
        b, W = self.b, self.world
        rng = b.rng_state()
        w_diff, count = b.begin_resample(rng, self._global_leaf_count())
        b.build_cdf(self.flags)
        if self.totals is not None:
            sums, sums_are_totals = self.totals, True
        else:
            sums, sums_are_totals = self._all_gather(b.local_sum()), False
        self.form_used = "window"
        if self.resample_form == "in_place" and self._resample_in_place(rng, count, sums, sums_are_totals):
            return
        window = self._window((count, "sys"), count)
        b.systematic_window(rng, count, sums, sums_are_totals, self.rank, W, window, self.flags)
        self._assemble(window)
        b.kld_reset()
        b.kld_insert_window(window, count)  # the tree of the new set: every sample, no stop rule
        leaf, bins = b.kld_counts()
        M = count
        lo, hi = (M * self.rank) // W, (M * (self.rank + 1)) // W
        pose = self._pose_rows(window)
        if M <= 8192:
            b.tail_small(pose[0], pose[1], pose[2], M, lo, hi, leaf, bins)
        else:
            b.adopt(pose[0][lo:hi], pose[1][lo:hi], pose[2][lo:hi], hi - lo, M, leaf, bins)
            b.converged(pose[0][:M], pose[1][:M], M)
        b.set_rng_state(b.end_resample(M))
        self.counts = self._even_counts(M)
        self.sample_count = M
        self.leaf_count, self.bin_count = leaf, bins
        self.windows_used = 1
        self.totals = None

    def _resample_in_place(self, rng, count, sums, sums_are_totals):
        """Every rank resamples its slice into its slice (bpf_shard_inplace_*); False: the imbalance cap sends this
        resample to the window form, nothing was changed.  Three small exchanges: the bin lists of the new tree, the
        limb words of the x / y sums, the count of updateConverged."""
        b = self.b
        counts, _, form = b.inplace_select(rng, count, sums, sums_are_totals, self.rank, self.world, self.flags)
        if form != RESAMPLE_IN_PLACE:
            return False
        self.counts, self.sample_count = counts, count
        return self._finish_in_place(count, counts, *self._global_tree())

    def _finish_in_place(self, M, counts, leaf, bins):
        """The tail of both in-place forms: the new slices (`counts` of every rank, M in all) are current in the
        backends.  The limb words of the x / y sums and the count of updateConverged cross, then the books; True."""
        b = self.b
        self.counts, self.sample_count = counts, M
        words = b.inplace_xy_sums()
        self._all_reduce_sum(words)  # limb form: the lane-wise int64 sum is exact
        near = b.inplace_converged(words, M)
        self._all_reduce_sum(near)
        b.inplace_converged_finish(near, M)
        b.set_rng_state(b.end_resample(M))
        self.leaf_count, self.bin_count = leaf, bins
        self.windows_used = 0
        self.totals = None
        self.form_used = "in_place"
        if hasattr(b, "tree_last_route"):
            self.tree_route = self.TREE_ROUTES.get(b.tree_last_route())
        self.rebalanced = 0
        if self.rebalance_mode == "auto" and max(counts) > self.trigger_share * ((M + self.world - 1) // self.world):
            self.rebalance()  # every rank decides alike from the same counts
        return True

    def _resample_in_place_mn(self, rng, sums, sums_are_totals):
        """The multinomial resample in place, stage by stage (bpf_shard_inplace_mn_*); False: this resample goes to the
        window form -- the imbalance cap, or a key outside the packing -- and nothing was changed.  Four small
        exchanges: the (bin count, flag) words, the bin lists, the limb words of the x / y sums, the count of
        updateConverged."""
        b, W = self.b, self.world
        b.inplace_mn_select(rng, sums, sums_are_totals, self.rank, W, self.flags)
        bin_counts, out_of_range, all_bins, pad = self._exchange_bin_lists(*b.inplace_mn_bins())
        if out_of_range:
            return False
        M, leaf, nbins, counts, _, form = b.inplace_mn_stop(all_bins, bin_counts, pad)
        if form != RESAMPLE_IN_PLACE:
            return False
        return self._finish_in_place(M, counts, leaf, nbins)

    # ---- the slices back to the even split, in global order (include/badger_pf.h, bpf_shard_rebalance_*)
    def rebalance(self):
        """Collective: every rank calls it.  Only the samples on the wrong rank move: one ragged all-gather of the
        outgoing x / y / theta / w bits, 32 B per moved sample into every rank.  The concatenation of the slices is
        unchanged bit for bit; tree counts, converged, w_slow / w_fast and the rng stay; the statistics are evaluated
        again and the totals of a sensor update are dropped (the next resample gathers the local CDF sums).  Returns
        the number of samples moved over all ranks (0: the split was even already, nothing crossed)."""
        b, W = self.b, self.world
        out, _, _ = b.rebalance_plan(self.counts, self.rank, W)
        moved = sum(out)
        if moved:
            allr, pad = self._gather_ragged(b.rebalance_export(), out)
            b.rebalance_import(allr.contiguous(), [r * 4 * pad for r in range(W)], pad)
            self._drop_totals()
            self._stats_valid = False
        else:
            b.rebalance_import(None, None, 0)
        self.counts = self._even_counts(sum(self.counts))
        self.rebalanced = moved
        return moved

    # ---- Seam B (multinomial, w_diff == 0)
    def update_resample(self):
        self._stats_valid = False
        self._update_resample()
        self._step += 1

    def _update_resample(self):
        b, W = self.b, self.world
        if self.mailbox and getattr(self, "_fused_totals", False) and hasattr(b, "mailbox_update_resample"):
            # one call: CDF, windows, stop rule, adoption of this rank's share (bpf_shard_mailbox_update_resample)
            leaf_in = self._global_leaf_count() if b.resample_model() == 1 else self.leaf_count
            try:
                M, leaf, bins, wins, hint = b.mailbox_update_resample(self.flags, self.sample_count, leaf_in,
                                                                      self.window_hint)
            except Exception as err:  # noqa: BLE001 -- only the exchange time-out is handled, the rest goes up
                committed = hasattr(b, "resample_committed") and b.resample_committed()
                if committed:
                    # the AUTO rebalance behind the resample failed: the new, uneven set is current.  Take it into the
                    # books first (whatever the error), never resample again (see _recover_exchange)
                    exchange = self._is_exchange_error(err)
                    if exchange:
                        self._recover_exchange(committed=True)
                    self._after_one_call_resample(*b.last_resample)
                    if not exchange:
                        raise
                    self.rebalance()
                    self._finish_recovery()
                    return
                if not self._is_exchange_error(err):
                    raise
                self._recover_exchange()
                self._update_resample_stages()
                self._finish_recovery()
                return
            self._after_one_call_resample(M, leaf, bins, wins, hint)
            return
        self._update_resample_stages()

    def _after_one_call_resample(self, M, leaf, bins, wins, hint):
        """The books after the engine's one-call resample made its new set current."""
        b = self.b
        self.counts = self._even_counts(M)
        self.form_used = "window"
        if self._in_place_wanted() and b.slice()[2] == RESAMPLE_IN_PLACE:
            # the slices are uneven: every rank's count (the engines hold them; one small gather tells the host)
            n = torch.tensor([b.n_local()], dtype=torch.int64, device=self.device)
            self.counts = [int(v) for v in self._all_gather(n).cpu().tolist()]
            self.form_used = "in_place"
            self.rebalanced = b.rebalance_last() if self.rebalance_mode == "auto" else 0
        self.sample_count, self.leaf_count, self.bin_count = M, leaf, bins
        self.windows_used, self.window_hint = wins, hint
        self._drop_totals()

    def _in_place_wanted(self):
        """The in-place form is set for the resampler in use."""
        return (self.resample_form if self.b.resample_model() == 1 else self.multinomial_form) == "in_place"

    def _finish_recovery(self):
        if getattr(self, "_remake_mailbox", False):
            self._remake_mailbox = False
            self.mailbox = self._setup_mailbox()

    def _update_resample_stages(self):
        """updateResample stage by stage (collectives, or a mailbox with the host between the stages)."""
        b, W = self.b, self.world
        if b.resample_model() == 1:  # PF_RESAMPLE_SYSTEMATIC
            return self._update_resample_systematic()
        b.build_cdf(self.flags)
        if self.totals is not None:
            sums, sums_are_totals = self.totals, True   # slices from the sensor update's totals
        else:
            sums, sums_are_totals = self._all_gather(b.local_sum()), False
        rng = b.rng_state()
        b.begin_resample(rng, self.leaf_count)  # w_diff; with w_diff > 0 the draws follow the resolved chain
        self.form_used = "window"
        if self.multinomial_form == "in_place" and self._resample_in_place_mn(rng, sums, sums_are_totals):
            return
        b.kld_reset()
        m0, stop = 0, -1
        win = max(1024, min(self.window_hint, self.max_global))
        self.windows_used = 0
        windows = []
        device_counts = None
        device_min = b.kld_device_min
        if win > 4096 and self.max_global - 4096 >= device_min:
            win = 4096  # keep the host's first window short when the device tree can take over after it
        need = 0  # after a window without a stop: draws still missing to the bound for the leaves seen so far
        while m0 < self.max_global and stop < 0:
            if m0 > 0 and self.max_global - m0 >= device_min and need >= device_min:
                # no stop in the first window and a long stream ahead (a spread cloud): one window with every
                # remaining candidate, and the ordered kd-tree replay runs on the device (every rank, redundantly)
                whole = self._window("whole", self.max_global)
                b.draw_window(rng, 0, self.max_global, sums, sums_are_totals, self.rank, W, whole, self.flags)
                self._assemble(whole)
                handled, dstop, dleaf, dbins = b.kld_stop_window(whole, self.max_global)
                self.windows_used += 1
                if handled:
                    stop = dstop
                    windows = [(0, self.max_global, whole)]
                    device_counts = (dleaf, dbins)
                    break
                device_min = 1 << 62  # this stream is outside what the device tree takes: host replay
            m1 = min(self.max_global, m0 + win)
            cnt = m1 - m0
            window = self._window((cnt, len(windows)), cnt)
            b.draw_window(rng, m0, m1, sums, sums_are_totals, self.rank, W, window, self.flags)
            self._assemble(window)
            stop = b.kld_feed_window(window, cnt, m0)  # the one host wait of the window
            if self.mailbox and stop < 0:
                # a mailbox window is overwritten two exchanges later: keep its poses now, the stream goes on
                self.out[:, m0:m0 + cnt] = window[0:3, :cnt].view(torch.float64)
                window = None
            windows.append((m0, cnt, window))
            self.windows_used += 1
            m0 = m1
            if stop < 0:
                # next window: up to a quarter past the bound for the leaves seen so far (a lower estimate of the stop)
                need = b.resample_limit(b.kld_counts()[0]) - m0
                win = resample_window_for(need)
        M = stop if stop > 0 else self.max_global
        leaf, bins = device_counts if device_counts is not None else b.kld_counts()
        lo, hi = (M * self.rank) // W, (M * (self.rank + 1)) // W
        if len(windows) == 1 and M <= 8192 and windows[0][2] is not None:
            # the common case: one window, small set -> adopt + weights + updateConverged in one launch
            pose = self._pose_rows(windows[0][2])
            b.tail_small(pose[0], pose[1], pose[2], M, lo, hi, leaf, bins)
        else:
            for (w0, cnt, window) in windows:
                if window is not None:
                    self.out[:, w0:w0 + cnt] = window[0:3, :cnt].view(torch.float64)
            b.adopt(self.out[0, lo:hi], self.out[1, lo:hi], self.out[2, lo:hi], hi - lo, M, leaf, bins)
            b.converged(self.out[0, :M], self.out[1, :M], M)
        b.set_rng_state(b.end_resample(M))
        self.counts = self._even_counts(M)
        self.sample_count = M
        self.leaf_count, self.bin_count = leaf, bins
        self.window_hint = resample_window_for(M)
        self.totals = None  # the weights are 1/M now; the old totals no longer describe them

    def restore(self, counts, leaf_count=0):
        """Bench helper: the shards were put back by pf.restore(); reset the bookkeeping."""
        self.counts = list(counts)
        self.sample_count = sum(counts)
        self._drop_totals()
        self._stats_valid = False
        self.leaf_count = leaf_count

    # ---- cluster statistics of the GLOBAL set (particle_filter.cpp:505-636, node_2d.cpp:588-617)
    STATS_GATHER_MAX = 4096  # kStatBlockMax: up to here every rank evaluates the gathered set in one launch

    def _gather_ragged(self, mine, counts):
        """All-gather of [rows, counts[rank]] tensors of different widths: padded to the widest, [world, rows, pad]."""
        pad = max(max(counts), 1)
        buf = torch.zeros((mine.shape[0], pad), dtype=mine.dtype, device=mine.device)
        buf[:, :mine.shape[1]] = mine
        return self._all_gather(buf.reshape(-1)).reshape(self.world, mine.shape[0], pad), pad

    def _ensure_stats(self):
        """Lazy, like the single engine: evaluated at the first query after the set changed.  Every rank has to
        make the query (the exchanges are collective)."""
        if self._stats_valid:
            return
        b, n = self.b, self.sample_count
        route = None
        if n <= self.STATS_GATHER_MAX:
            # the tracking regime: the whole set on every rank, evaluated redundantly
            allv, _ = self._gather_ragged(b.stats_local_soa(), self.counts)
            soa = self._concat_ragged(allv, self.counts).contiguous()
            handled = b.stats_gathered(soa, n)
            if handled > 0:
                route = "gathered"
            elif handled < 0:
                route = "host"
        if route is None:
            bin_counts, host_route, all_bins, pad = self._exchange_bin_lists(
                *b.stats_local_bins(sum(self.counts[:self.rank])))
            if host_route:
                route = "host"
            else:
                b.stats_label(all_bins, bin_counts, pad)
                sums = b.stats_local_sums()
                self._all_reduce_sum(sums)  # limb form: the lane-wise int64 sum is exact
                # (a backend without a range to leave returns None)
                route = "host" if b.stats_finish(sums) is False else "distributed"
        if route == "host":
            local = torch.from_numpy(np.ascontiguousarray(b.stats_local_samples_host()[:, :4].T))
            allv, _ = self._gather_ragged(local.to(self.device), self.counts)
            b.stats_host(self._concat_ragged(allv.cpu(), self.counts).T.contiguous().numpy())
        self.stats_route = route
        self._stats_valid = True

    def compute_cluster_stats(self):
        """(cluster_count, set_mean[3], set_cov[5]) of the global set; cov entries (0,0) (0,1) (1,0) (1,1) (2,2)."""
        self._ensure_stats()
        return self.b.stats_result()

    def get_cluster(self, k):
        """(weight, mean[3], count, cov[5]) of cluster k of the global set, None past the last cluster."""
        self._ensure_stats()
        return self.b.stats_cluster(k)

    def get_max_weight_pose(self):
        """Node2D::getMaxWeightPose over the global set: (weight, pose) of the heaviest cluster."""
        self._ensure_stats()
        return self.b.stats_max_weight_pose()

    # ---- the particle cloud (Node::publishParticleCloud, node.cpp:335-357) of the GLOBAL set
    def get_pose_array(self, root=0, first=0, stride=1):
        """[count, 7] float64 rows {x, y, 0, qx, qy, qz, qw} of the global samples first, first + stride, ... in
        global order, on rank `root` (root = -1: on every rank); None on the other ranks.  Collective: every rank
        calls it with the same arguments.  One ragged all-gather of the selected x / y / theta bits; the statistics,
        the totals and the set stay as they are."""
        if not -1 <= root < self.world:
            raise ValueError("get_pose_array: root in [-1, world)")
        sel = pose_selection(self.counts, first, stride)
        count = sum(n for _, n in sel)
        if self.mailbox and hasattr(self.b, "get_pose_array_all"):
            return self.b.get_pose_array_all(root, first, stride, count)
        receives = root < 0 or root == self.rank
        if count == 0:
            return np.empty((0, 7), dtype=np.float64) if receives else None
        mine = self.b.pose_rows(sum(self.counts[:self.rank]), first, stride)
        sel_counts = [n for _, n in sel]
        assert mine.shape[1] == sel_counts[self.rank]
        allr, _ = self._gather_ragged(mine, sel_counts)
        if not receives:
            return None
        rows = self._concat_ragged(allr, sel_counts).contiguous()
        return self.b.pose_array_from_rows(rows, count)

    # ---- global localisation: pose search over the ranks
    def _engine_exchange(self):
        """The engine's own transport carries the one-call searches: the mailbox, or a world the engines were
        connected to outside this class (bpf_shard_bootstrap, bpf_shard_connect_local)."""
        return self.mailbox or (hasattr(self.b, "exchange_mode") and self.b.exchange_mode() != 0)

    def _share(self, first, total):
        lo, hi = (total * self.rank) // self.world, (total * (self.rank + 1)) // self.world
        return first + lo, hi - lo

    def _merge_rows(self, rows, k):
        """The ranks' hit rows (at most k each) gathered as int64 words and merged on the host."""
        words = np.zeros(7 * int(k) + 1, dtype=np.int64)
        words[0] = rows.shape[0]
        words[1:1 + 7 * rows.shape[0]] = np.ascontiguousarray(rows).view(np.int64)
        allw = self._all_gather(torch.from_numpy(words).to(self.device)).cpu().numpy().reshape(self.world, -1)
        lists = [np.ascontiguousarray(w[1:1 + 7 * int(w[0])]).view(POSE_HIT_DTYPE) for w in allw]
        return merge_pose_hits(lists, k)

    def search_poses(self, data, headings, cell_stride, k, first=0, count=-1):
        """The scanner's searchPoses (planar scan or cloud, by the data) over the ranks: collective, the same
        arguments on every rank, the single engine's rows for the range on every rank.  Rank r scores candidates
        [first + T r / W, first + T (r + 1) / W) of the T given.  On the engine's own transport the lists are merged
        on the device (bpf_shard_search_poses); on collectives the rows are gathered as int64 words and merged on the
        host."""
        sc = self.b.sc
        total = sc.searchSpace(headings, cell_stride)[0]
        if not (1 <= int(k) <= 1024) or first < 0 or first > total or count < -1 or count > total - first:
            raise ValueError("search_poses: 1 <= k <= 1024 and first / count inside the candidate space")
        if hasattr(self.b, "search_poses_all") and self._engine_exchange():
            return self.b.search_poses_all(data, headings, cell_stride, k, first, count)
        lo, n = self._share(first, total - first if count < 0 else count)
        mine = sc.searchPoses(data, headings, cell_stride, k, lo, n)
        return self._merge_rows(mine, k)

    def search_poses_pruned(self, data, headings, cell_stride, k, block=None, first_block=0, block_count=-1):
        """The scanner's searchPosesPruned over the ranks: (rows, this rank's stats); the block range is split like
        the candidates of search_poses.  On the engine's own transport the ranks share their tau behind the seed
        (bpf_shard_search_poses_pruned).  On collectives there is NO shared tau: every rank prunes against the k-th
        score of its own share, and the stats are those of the stand-alone range call."""
        sc = self.b.sc
        opt = {} if block is None else {"block": int(block)}
        if block is None:
            block = sc.searchPosesPruned.__defaults__[0]
        total = sc.searchBlocks(cell_stride, block)
        if (not (1 <= int(k) <= 1024) or first_block < 0 or first_block > total or block_count < -1
                or block_count > total - first_block):
            raise ValueError("search_poses_pruned: 1 <= k <= 1024 and first_block / block_count inside the block list")
        if hasattr(self.b, "search_poses_pruned_all") and self._engine_exchange():
            return self.b.search_poses_pruned_all(data, headings, cell_stride, k, block, first_block, block_count)
        lo, n = self._share(first_block, total - first_block if block_count < 0 else block_count)
        mine, stats = sc.searchPosesPruned(data, headings, cell_stride, k, first_block=lo, block_count=n, stats=True,
                                           **opt)
        return self._merge_rows(mine, k), stats

    cloud_search_poses = search_poses
    cloud_search_poses_pruned = search_poses_pruned

    def localize(self, data, headings, cell_stride, k, refine, moments, mixture, pruned=True, block=None):
        """Global localisation in one call, host composition only: the sharded search; refinePoses and poseMoments on
        every rank (replicated: at most 1024 lattices, identical inputs on identical devices); mixtureFromHits and
        mixtureApplyMoments; init_with_mixture.  refine = (xy_radius, xy_step, theta_radius, theta_step, levels);
        moments = (xy_radius, xy_step, theta_radius, theta_step, baseline, sigma_floor, sigma_cap); mixture =
        (xy_merge, theta_merge, max_components, sigma).  Returns the components."""
        if pruned:
            hits, _ = self.search_poses_pruned(data, headings, cell_stride, k, block)
        else:
            hits = self.search_poses(data, headings, cell_stride, k)
        comps = mixture_of_hits(self.b.sc, data, hits, self.max_global, refine, moments, mixture)
        self.init_with_mixture(comps)
        return comps

    def set_random_pose_generator(self, mode):
        """random_pose_fn of this rank's engine (pf.RANDOM_POSE_*); every rank sets the same mode.  Every rank
        resolves the same draw chain, shard 0 writes the random poses."""
        self.b.set_random_pose_generator(mode)

    def set_uniform_pose_check(self, threshold, multiplier, scoring=0):
        """Node::uniformPoseGenerator's score check on this rank's engine (pf.ParticleFilter.setUniformPoseCheck);
        every rank sets the same values.  The sharded resample takes pf.POSE_CHECK_AS_REFERENCE only."""
        self.b.set_uniform_pose_check(threshold, multiplier, scoring)

    def state(self):
        st = self.b.state()
        miss = self._all_reduce_sum(self.flags.clone())
        return ShardedState(sample_count=self.sample_count, local_count=st.sample_count, leaf_count=self.leaf_count,
                            bin_count=self.bin_count, converged=st.converged,
                            percent_converged=st.percent_converged, w_slow=st.w_slow, w_fast=st.w_fast,
                            total=st.total, cdf_miss=int(miss[0].item()) != 0, windows=self.windows_used)
