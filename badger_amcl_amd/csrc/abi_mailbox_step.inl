// C-ABI: the sharded sensor update and resample as single calls for the mailbox mode.  With the exchanges inside the
// kernels there is nothing left for a host-side collective layer to do between the stage functions, so the whole
// sequence of badger_amcl_amd/sharded.py runs here, stage function by stage function (same order, same arguments),
// and the host pays one call per update instead of a dozen.
//
// The same sequence also runs with RCCL collectives between the stages (bpf_shard_bootstrap falls back to that when the
// mailbox cannot be set up): the totals go through ncclAllGather after the scoring stage and every draw window through
// an integer ncclAllReduce(sum) before its first consumer -- ShardExchange hides which of the two it is.
//
// ShardExchange also carries the two general small exchanges of the one-call forms (abi_shard_node.inl, the beam-skip
// counts below): a ragged all-gather and an integer all-reduce(sum), over the mailbox's window region
// (k_mailbox_post_words / k_mailbox_take_ragged / k_mailbox_take_sum) or over RCCL.  The sequences of such exchanges
// that several one-call forms share (sample counts, bin lists, the global tree) are at the head of abi_shard_node.inl,
// and the in-place resamples' common tail, inplace_finish, is in abi_shard_inplace.inl.
namespace
{
struct ShardExchange
{
  bpf_engine* e;
  bool collective() const { return !e->mb.active; }

  // a fresh [6][stride] int64 window for `count` draws
  long long* next_window(int count, int* stride)
  {
    if (!collective())
    {
      void* w = nullptr;
      if (bpf_shard_mailbox_window(e, &w, stride) != BPF_OK)
        return nullptr;
      return static_cast<long long*>(w);
    }
    // two buffers in turn: the previous window stays readable while the next one is assembled
    DevBuf<long long>& buf = e->coll.window[e->coll.window_turn ^= 1];
    const size_t cols = (size_t)((count + 255) / 256) * 256;
    if (buf.reserve(6 * cols) != hipSuccess)
    {
      e->fail(BPF_ERR_HIP, "collective window allocation");
      return nullptr;
    }
    *stride = (int)cols;
    return buf.p;
  }

  // every shard's columns into every shard's copy of the window
  int assemble(long long* window, int stride)
  {
    if (!collective())
      return BPF_OK;  // the draw kernel stored them into all peers; the window's first consumer waits for them
    ++e->coll.exchanges;
    if (e->coll.fn.allreduce_sum_i64(e->coll.comm, window, (size_t)6 * stride, e->stream) != 0)
      return e->fail(BPF_ERR_EXCHANGE, std::string("RCCL window all-reduce: ") + e->coll.fn.last_error());
    return BPF_OK;
  }

  // the next generation of the window region for an exchange addressed by word offset
  int next_words(unsigned long long* gen)
  {
    if (e->mb.win_wait)
      return e->fail(BPF_ERR_NOT_CONFIGURED, "mailbox: the previous window was never consumed");
    *gen = ++e->mb.win_gen;
    return BPF_OK;
  }
  // blocks of 256 for `words` words, never more than a grid may wait with
  static int small_grid(long long words)
  {
    return (int)std::max<long long>(1, std::min<long long>((words + 255) / 256, kMailboxFusedWaitBlocks));
  }

  // Ragged all-gather of int64 words: this rank contributes `rows` rows of counts[rank] words (row k at src[k]), every
  // rank ends with rank r's row k at dst[dst_off[r] + k * dst_stride ...].  counts: host, the same on every rank.
  // Asynchronous on the engine's stream; after a mailbox wait that ran out dst is left alone (finish() tells).
  int gather(const long long* const* src, int rows, const long long* counts, long long* dst, const long long* dst_off,
             long long dst_stride)
  {
    const int W = e->shard_world, rank = e->shard_rank;
    if (rows < 1 || rows > 4 || W < 1 || W > kMailboxMaxWorld)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "shard gather: 1 .. 4 rows, at most 16 ranks");
    MbRagged L{};
    L.world = W;
    L.rows = rows;
    L.dst_stride = dst_stride;
    long long total = 0, widest = 1;
    for (int r = 0; r < W; ++r)
    {
      L.count[r] = counts[r];
      L.dst_off[r] = dst_off[r];
      L.src_off[r] = total;
      L.src_stride[r] = counts[r];
      total += (long long)rows * counts[r];
      widest = std::max(widest, counts[r]);
    }
    if (!collective())
    {
      if (total > 6 * e->mb.max_window)
        return e->fail(BPF_ERR_CAPACITY, "mailbox windows are smaller than the gathered payload");
      unsigned long long g = 0;
      int rc = next_words(&g);
      if (rc != BPF_OK)
        return rc;
      MbPostArgs A{};
      for (int k = 0; k < rows; ++k)
        A.src[k] = src[k];
      A.rows = rows;
      A.count = counts[rank];
      A.word_off = L.src_off[rank];
      hipLaunchKernelGGL(k_mailbox_post_words, dim3(small_grid(rows * counts[rank])), dim3(256), 0, e->stream,
                         mailbox_dev(e), A, (int)(g & 1), g, e->d_mb_counter.p);
      hipLaunchKernelGGL(k_mailbox_take_ragged, dim3(small_grid(rows * widest)), dim3(256), 0, e->stream, mailbox_dev(e),
                         (const long long*)nullptr, dst, L, (int)(g & 1), g);
      HIPCHK(e, hipGetLastError());
      return BPF_OK;
    }
    // RCCL: every contribution padded to the widest one, then the same re-layout out of the receive buffer
    ++e->coll.exchanges;
    const size_t per = (size_t)rows * (size_t)widest;
    HIPCHK(e, e->coll.send.reserve(per));
    HIPCHK(e, e->coll.recv.reserve(per * (size_t)W));
    HIPCHK(e, hipMemsetAsync(e->coll.send.p, 0, per * sizeof(long long), e->stream));
    for (int k = 0; k < rows && counts[rank] > 0; ++k)
      HIPCHK(e, copy_d2d(e->coll.send.p + (size_t)k * widest, src[k], (size_t)counts[rank], e->stream));
    if (e->coll.fn.allgather_i64(e->coll.comm, e->coll.send.p, e->coll.recv.p, per, e->stream) != 0)
      return e->fail(BPF_ERR_EXCHANGE, std::string("RCCL all-gather: ") + e->coll.fn.last_error());
    for (int r = 0; r < W; ++r)
    {
      L.src_off[r] = (long long)r * (long long)per;
      L.src_stride[r] = widest;
    }
    hipLaunchKernelGGL(k_mailbox_take_ragged, dim3(small_grid(rows * widest)), dim3(256), 0, e->stream, MailboxDev{},
                       (const long long*)e->coll.recv.p, dst, L, 0, 0ull);
    HIPCHK(e, hipGetLastError());
    return BPF_OK;
  }

  // All-reduce(sum) in place of n integer words (int32 when i32, else int64).  Mailbox: gather-then-sum in rank order, in
  // as many rounds as the window region takes (W spans per round).
  int reduce_sum(void* buf, size_t n, bool i32)
  {
    if (collective())
    {
      ++e->coll.exchanges;
      const int bad = i32 ? e->coll.fn.allreduce_sum_i32(e->coll.comm, static_cast<int*>(buf), n, e->stream)
                          : e->coll.fn.allreduce_sum_i64(e->coll.comm, static_cast<long long*>(buf), n, e->stream);
      if (bad)
        return e->fail(BPF_ERR_EXCHANGE, std::string("RCCL all-reduce: ") + e->coll.fn.last_error());
      return BPF_OK;
    }
    const int W = e->shard_world, rank = e->shard_rank;
    const size_t per = (size_t)(6 * e->mb.max_window) / (size_t)W;
    if (per == 0)
      return e->fail(BPF_ERR_CAPACITY, "mailbox windows are smaller than one word per rank");
    for (size_t done = 0; done < n; done += per)
    {
      const size_t chunk = std::min(per, n - done);
      unsigned long long g = 0;
      int rc = next_words(&g);
      if (rc != BPF_OK)
        return rc;
      void* at = i32 ? static_cast<void*>(static_cast<int*>(buf) + done)
                     : static_cast<void*>(static_cast<long long*>(buf) + done);
      MbPostArgs A{};
      A.src[0] = static_cast<const long long*>(at);
      A.rows = 1;
      A.widen32 = i32 ? 1 : 0;
      A.count = (long long)chunk;
      A.word_off = (long long)rank * (long long)chunk;
      hipLaunchKernelGGL(k_mailbox_post_words, dim3(small_grid((long long)chunk)), dim3(256), 0, e->stream,
                         mailbox_dev(e), A, (int)(g & 1), g, e->d_mb_counter.p);
      hipLaunchKernelGGL(k_mailbox_take_sum, dim3(small_grid((long long)chunk)), dim3(256), 0, e->stream, mailbox_dev(e),
                         at, (long long)chunk, i32 ? 1 : 0, (int)(g & 1), g);
      HIPCHK(e, hipGetLastError());
    }
    return BPF_OK;
  }

  // the host's check behind exchanges whose result it (or a stage that must not run on half of it) depends on
  int finish()
  {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return collective() ? BPF_OK : mailbox_check(e);
  }

  // the W weight totals of the scoring stage just issued
  int totals(void** out)
  {
    if (!collective())
      return bpf_shard_mailbox_totals(e, out);
    ++e->coll.exchanges;
    HIPCHK(e, e->coll.totals.reserve((size_t)e->shard_world));
    if (e->coll.fn.allgather_f64(e->coll.comm, &e->d_scalars.p->v[0], e->coll.totals.p, 1, e->stream) != 0)
      return e->fail(BPF_ERR_EXCHANGE, std::string("RCCL totals all-gather: ") + e->coll.fn.last_error());
    *out = e->coll.totals.p;
    return BPF_OK;
  }
};

int shard_step_ready(bpf_engine* e)
{
  if (!e->mb.active && !e->coll.active)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "no shard exchange set up (bpf_shard_bootstrap / bpf_shard_mailbox_connect)");
  return BPF_OK;
}
}  // namespace

namespace
{
// totals of the scoring stage just issued, normalisation, and what bpf_shard_mailbox_update_resample requires of
// "the totals of this update"
int shard_totals_and_normalize(bpf_engine* e, ShardExchange& X, long long global_count)
{
  void* totals = nullptr;
  int rc = X.totals(&totals);
  if (rc != BPF_OK)
    return rc;
  rc = bpf_shard_normalize_dev(e, totals, e->shard_world, (int)global_count);
  if (rc != BPF_OK)
    return rc;
  e->mb_totals = totals;
  e->mb_totals_valid = true;
  return BPF_OK;
}

// counts_over_mailbox: sum the beam-skip counts over the mailbox too (bpf_shard_update_sensor_planar); false hands
// BPF_SHARD_NEED_BEAM_COUNTS back in mailbox mode (bpf_shard_mailbox_update_sensor_planar, whose caller sums them)
int shard_update_sensor_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                               double range_max, long long global_count, bool counts_over_mailbox)
{
  if (!e || global_count <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  ShardExchange X{ e };
  e->mb_totals_valid = false;
  rc = bpf_shard_score_planar(e, ranges, angles, range_count, range_max);
  if (rc == BPF_SHARD_NEED_BEAM_COUNTS && (X.collective() || counts_over_mailbox))
  {
    // beam skipping: the per-beam agreement counts are summed over the shards between the two passes
    void* counts = nullptr;
    int n_counts = 0;
    rc = bpf_shard_beam_counts_dev(e, &counts, &n_counts);
    if (rc != BPF_OK)
      return rc;
    rc = X.reduce_sum(counts, (size_t)n_counts, true);
    if (rc == BPF_OK && !X.collective())
      rc = X.finish();  // the second pass must not score against one shard's counts
    if (rc != BPF_OK)
      return rc;
    rc = bpf_shard_score_planar_finish(e, ranges, angles, range_count, range_max, global_count);
  }
  if (rc != BPF_OK)
    return rc;  // includes BPF_SHARD_NEED_BEAM_COUNTS (mailbox form): the caller sums the counts in between
  if (e->pm.max_beams < 2)
    return BPF_OK;
  return shard_totals_and_normalize(e, X, global_count);
}
}  // namespace

int bpf_shard_mailbox_update_sensor_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                           double range_max, long long global_count)
{
  return shard_update_sensor_planar(e, ranges, angles, range_count, range_max, global_count, false);
}

namespace
{
// abi_shard_inplace.inl: the systematic resample with BPF_SHARD_RESAMPLE_IN_PLACE set
int shard_update_resample_in_place(bpf_engine* e, void* flags_dev, uint64_t rng, int count, bool* done, int* leaf_out,
                                   int* bins_out);
// abi_shard_inplace_mn.inl: the multinomial resample with bpf_shard_set_multinomial_form(BPF_SHARD_RESAMPLE_IN_PLACE)
int shard_update_resample_in_place_mn(bpf_engine* e, void* flags_dev, uint64_t rng, bool* done, int* M_out, int* leaf_out,
                                      int* bins_out);
// abi_shard_rebalance.inl: BPF_SHARD_REBALANCE_AUTO behind an in-place resample
int shard_rebalance_auto(bpf_engine* e);
}  // namespace

namespace
{
// ---- the window forms of the sharded resample: what one call's forms share ...
struct ShardResample
{
  bpf_engine* e;
  ShardExchange& X;
  void* flags_dev;
  uint64_t rng;  // the stream state the resample began from
  int rank, W, max_global;
};

// ... and an exchanged window of candidate poses: rows x, y, theta (as doubles), then the three key rows
struct ShardWindow
{
  long long* p = nullptr;
  int stride = 0;
  const double* row(int k) const { return reinterpret_cast<const double*>(p + (size_t)k * stride); }
};

// this rank's share of the new set of out.M samples out of the rows of all of them, weights 1/M, updateConverged
int shard_adopt_from(const ShardResample& S, const ResampleOutcome& out, const double* x, const double* y,
                     const double* th)
{
  bpf_engine* e = S.e;
  const int M = out.M;
  const int lo = (int)(((long long)M * S.rank) / S.W), hi = (int)(((long long)M * (S.rank + 1)) / S.W);
  if (M <= 8192)
    return bpf_shard_tail_small_dev(e, x, y, th, M, lo, hi, out.leaf, out.bins);
  int rc = bpf_shard_adopt_dev(e, x + lo, y + lo, th + lo, hi - lo, M, out.leaf, out.bins);
  if (rc != BPF_OK)
    return rc;
  return bpf_shard_converged_dev(e, x, y, M);
}

// The systematic window form: one window with every sample.  Tracking regime: the new set's tree (no stop rule), the
// adoption and updateConverged in one launch; otherwise, or when that declines, the host's tree and the tail.
int shard_systematic_window(const ShardResample& S, int sys_count, ResampleOutcome* out)
{
  bpf_engine* e = S.e;
  ShardWindow win;
  win.p = S.X.next_window(sys_count, &win.stride);
  if (!win.p)
    return e->last_status;
  const bool tracking = e->fused_resample && sys_count <= kFusedWindow;
  const bool merged = tracking && !S.X.collective();  // mailbox: the draws and their consumer in ONE launch
  WindowArgs draw{};
  int rc;
  if (merged)
  {
    size_t lds_unused = 0;
    rc = systematic_window_args(e, S.rng, sys_count, e->mb_totals, 1, S.rank, S.W, win.p, win.stride, S.flags_dev, &draw,
                                &lds_unused);
  }
  else
    rc = bpf_shard_systematic_window_dev(e, S.rng, sys_count, e->mb_totals, 1, S.rank, S.W, win.p, win.stride,
                                         S.flags_dev);
  if (rc != BPF_OK)
    return rc;
  H2D_OR_RETURN(S.X.assemble(win.p, win.stride));
  out->windows = 1;
  int fused_status = BPF_FUSED_TOO_MANY_BINS;
  if (tracking)
  {
    rc = shard_stop_block(e, win.p, win.stride, sys_count, true, &fused_status, out, merged ? &draw : nullptr);
    if (rc == BPF_OK && merged)
      rc = systematic_targets_in_use(e);
    if (rc != BPF_OK)
      return rc;
  }
  if (fused_status == BPF_FUSED_OK)
    return BPF_OK;
  bpf_kld_reset(e);
  H2D_OR_RETURN(bpf_kld_insert_dev(e, win.p, win.stride, sys_count));  // the host's tree
  counted_by_host_tree(e, out);
  out->M = sys_count;
  return shard_adopt_from(S, *out, win.row(0), win.row(1), win.row(2));
}

// ---- the multinomial window form, by the schedule of resample_plan.hpp
// what its windows leave behind for the adoption at the end
struct ShardReplay
{
  int stop = -1;
  ShardWindow last;      // the latest window: the set is adopted from it when nothing had to be kept
  int host_windows = 0;  // windows the host replayed
  bool kept = false;     // poses were copied to e->d_shard_out
};

// The sharded driver's tracking predicate: the first window (AFTER the schedule's cap at 4096) and the hint both fit
// one block.  (The single engine's differs: multinomial_tracking in host_resample.inl.)
bool shard_tracking(const bpf_engine* e, int m0, int count, int hint)
{
  return m0 == 0 && e->fused_resample && count <= kFusedWindow && hint <= kFusedWindow;
}

// a fresh window with the draws [m0, m1) of every shard; `merged_draw`: the arguments only, for a consumer that makes
// the draws in its own launch
int shard_draw_window(const ShardResample& S, int m0, int m1, ShardWindow* win, WindowArgs* merged_draw)
{
  bpf_engine* e = S.e;
  win->p = S.X.next_window(m1 - m0, &win->stride);
  if (!win->p)
    return e->last_status;
  int rc;
  if (merged_draw)
  {
    size_t lds_unused = 0;
    rc = draw_window_args(e, S.rng, m0, m1, e->mb_totals, 1, S.rank, S.W, win->p, win->stride, S.flags_dev, merged_draw,
                          &lds_unused);
  }
  else
    rc = bpf_shard_draw_window_dev(e, S.rng, m0, m1, e->mb_totals, 1, S.rank, S.W, win->p, win->stride, S.flags_dev);
  if (rc != BPF_OK)
    return rc;
  return S.X.assemble(win->p, win->stride);
}

// No stop so far and a long stream ahead (a spread cloud): one window with every candidate, and the ordered kd-tree
// replay runs on the device (every rank, redundantly).  *handled = false: this stream is outside what the device tree
// takes, host replay.
int shard_whole_stream_window(const ShardResample& S, ShardReplay* R, ResampleOutcome* out, bool* handled)
{
  ShardWindow whole;
  H2D_OR_RETURN(shard_draw_window(S, 0, S.max_global, &whole, nullptr));
  int ok = 0, stop = -1, leaf = 0, bins = 0;
  H2D_OR_RETURN(bpf_kld_stop_dev(S.e, whole.p, whole.stride, S.max_global, &ok, &stop, &leaf, &bins));
  ++out->windows;
  *handled = ok != 0;
  if (!*handled)
    return BPF_OK;
  R->stop = stop;
  out->counted(COUNTED_BY_DEVICE_TREE, leaf, bins);
  R->last = whole;
  R->kept = false;
  return BPF_OK;
}

// The tracking regime: the stream is expected to stop inside this first window, and the stop rule, the adoption of
// this rank's share and updateConverged run in one single-block launch on every rank.  *adopted = false: no stop in
// the window, or keys / bins beyond what the kernel takes -- the host replays this same window.
int shard_tracking_window(const ShardResample& S, int m0, int m1, ShardWindow* win, ResampleOutcome* out, bool* adopted)
{
  const bool merged = !S.X.collective();  // mailbox: the draws and their consumer in ONE launch
  WindowArgs draw{};
  H2D_OR_RETURN(shard_draw_window(S, m0, m1, win, merged ? &draw : nullptr));
  int fused_status = BPF_FUSED_TOO_MANY_BINS;
  H2D_OR_RETURN(shard_stop_block(S.e, win->p, win->stride, m1 - m0, false, &fused_status, out, merged ? &draw : nullptr));
  *adopted = fused_status == BPF_FUSED_OK;
  if (*adopted)
    ++out->windows;
  return BPF_OK;
}

// A mailbox window is overwritten two exchanges later, and a set that spans windows is adopted from one buffer: keep
// this window's poses
int shard_keep_window(const ShardResample& S, const ShardWindow& win, int m0, int count, ShardReplay* R)
{
  bpf_engine* e = S.e;
  HIPCHK(e, e->d_shard_out.reserve((size_t)3 * S.max_global));
  for (int k = 0; k < 3; ++k)
    HIPCHK(e, copy_d2d(e->d_shard_out.p + (size_t)k * S.max_global + m0, (const double*)win.row(k), (size_t)count,
                       e->stream));
  R->kept = true;
  return BPF_OK;
}

// the host's ordered replay of the window's keys (the one host wait of the window)
int shard_host_window(const ShardResample& S, const ShardWindow& win, int m0, int count, ShardReplay* R,
                      ResampleOutcome* out)
{
  H2D_OR_RETURN(bpf_kld_feed_dev(S.e, win.p, win.stride, count, m0, &R->stop));
  ++out->windows;
  ++R->host_windows;
  R->last = win;
  if (R->stop < 0 || R->host_windows > 1)
    return shard_keep_window(S, win, m0, count, R);
  return BPF_OK;
}

int shard_multinomial_windows(const ShardResample& S, int* window_hint_io, ResampleOutcome* out)
{
  bpf_engine* e = S.e;
  bpf_kld_reset(e);
  // whole_stream_at_start = false: this driver replays a first window whatever the hint says
  WindowSchedule s = window_schedule(*window_hint_io, S.max_global, e->kld_device_min, false);
  ShardReplay R;
  int limit = 0;  // the bound for the leaves the host has seen so far
  bool adopted = false, on_device = false;
  while (s.m0 < S.max_global && R.stop < 0)
  {
    if (s.whole_stream_due(limit))
    {
      H2D_OR_RETURN(shard_whole_stream_window(S, &R, out, &on_device));
      if (on_device)
        break;
      s.device_declined = true;
    }
    const int m1 = s.m1(), count = m1 - s.m0;
    ShardWindow win;
    if (shard_tracking(e, s.m0, count, *window_hint_io))
    {
      H2D_OR_RETURN(shard_tracking_window(S, s.m0, m1, &win, out, &adopted));
      if (adopted)
        break;
    }
    else
      H2D_OR_RETURN(shard_draw_window(S, s.m0, m1, &win, nullptr));
    H2D_OR_RETURN(shard_host_window(S, win, s.m0, count, &R, out));
    limit = resample_limit(kld_host_k(e), e->min_samples, e->max_samples, e->pop_err, e->pop_z);
    s.next(limit);
  }
  if (!adopted)
  {
    out->M = R.stop > 0 ? R.stop : S.max_global;
    if (!on_device)
      counted_by_host_tree(e, out);
    const size_t mg = (size_t)S.max_global;
    H2D_OR_RETURN(R.kept ? shard_adopt_from(S, *out, e->d_shard_out.p, e->d_shard_out.p + mg, e->d_shard_out.p + 2 * mg)
                         : shard_adopt_from(S, *out, R.last.row(0), R.last.row(1), R.last.row(2)));
  }
  *window_hint_io = resample_window_for(out->M);
  return BPF_OK;
}
}  // namespace

// The sharded resample in one call: validation, CDF, begin, the form (in place, or one of the window forms above),
// end, commit, rebalance
int bpf_shard_mailbox_update_resample(bpf_engine* e, void* flags_dev, int* global_count_io, int* leaf_count_io,
                                      int* bin_count_out, int* windows_out, int* window_hint_io)
{
  if (!e || !flags_dev || !global_count_io || !leaf_count_io || !bin_count_out || !windows_out || !window_hint_io)
    return BPF_ERR_INVALID_ARGUMENT;
  e->resample_committed = false;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  if (!e->mb_totals_valid)
    return e->fail(BPF_ERR_NOT_CONFIGURED,
                   "sharded resample: needs the totals of bpf_shard_mailbox_update_sensor_planar of this update");
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  rc = bpf_shard_build_cdf(e, flags_dev);
  if (rc != BPF_OK)
    return rc;
  // engines of a sharded filter carry the GLOBAL bounds
  const ShardResample S{ e, X, flags_dev, e->rng, e->shard_rank, e->shard_world, e->max_samples };
  double w_diff = 0.0;
  int sys_count = 0;
  rc = bpf_shard_begin_resample(e, S.rng, *leaf_count_io, &w_diff, &sys_count);
  if (rc != BPF_OK)
    return rc;
  ResampleOutcome out;
  *windows_out = 0;
  bool in_place = false;
  if (e->resample_model == BPF_RESAMPLE_SYSTEMATIC && e->shard_form == BPF_SHARD_RESAMPLE_IN_PLACE)
  {
    // every rank resamples its own slice into its own slice; the imbalance cap hands this resample to the window below
    rc = shard_update_resample_in_place(e, flags_dev, S.rng, sys_count, &in_place, &out.leaf, &out.bins);
    out.M = sys_count;
  }
  else if (e->resample_model == BPF_RESAMPLE_MULTINOMIAL && e->shard_mn_form == BPF_SHARD_RESAMPLE_IN_PLACE)
    // every rank keeps the candidate draws of its own slice and finds the stop from the merged bin lists; the imbalance
    // cap, or a key outside the packing, hands this resample to the windows below
    rc = shard_update_resample_in_place_mn(e, flags_dev, S.rng, &in_place, &out.M, &out.leaf, &out.bins);
  if (rc != BPF_OK)
    return rc;
  if (in_place)
  {
    // nothing left to do: the slice is current, with the global set's tree counts and updateConverged's count
  }
  else if (!X.collective() && S.max_global > e->mb.max_window)  // (the in-place form needs no window of that size)
    return e->fail(BPF_ERR_CAPACITY, "mailbox windows are smaller than max_samples");
  else
    rc = e->resample_model == BPF_RESAMPLE_SYSTEMATIC ? shard_systematic_window(S, sys_count, &out)
                                                      : shard_multinomial_windows(S, window_hint_io, &out);
  if (rc != BPF_OK)
    return rc;
  uint64_t rng_after = 0;
  rc = bpf_shard_end_resample(e, out.M, &rng_after);
  if (rc != BPF_OK)
    return rc;
  // commit: the stream, the split, and the caller's record of the new set
  e->rng = rng_after;
  e->mb_totals_valid = false;  // the weights are 1/M now
  if (!in_place)
  {
    // the window forms leave the even split
    e->slice_first = ((long long)out.M * S.rank) / S.W;
    e->slice_global = out.M;
    e->shard_form_used = BPF_SHARD_RESAMPLE_WINDOW;
  }
  *global_count_io = out.M;
  *leaf_count_io = out.leaf;
  *bin_count_out = out.bins;
  *windows_out = out.windows;
  e->resample_committed = true;
  // the resample is complete and committed: a rebalance that fails from here on leaves the uneven set current and valid
  if (in_place && e->shard_rebalance == BPF_SHARD_REBALANCE_AUTO)
    return shard_rebalance_auto(e);
  return BPF_OK;
}
