// C-ABI: rebalancing the slices of a sharded set (kernels_shard_rebalance.hpp, shard_rebalance_plan.hpp).  The slices
// go back to the even split in global order and only the samples on the wrong rank move: one ragged all-gather of the
// outgoing rows.  Stage functions for a host with a transport of its own -- no call here waits for another rank --, the
// one-call form over the engine's exchange (ShardExchange, abi_mailbox_step.inl), and the AUTO mode that
// bpf_shard_update_resample runs behind an in-place resample.
// ---------------------------------------------------------------------- rebalance
namespace
{
static_assert(kRebalanceMaxWorld == kMailboxMaxWorld, "the plan and the exchange take the same worlds");

// the plan for `counts`, checked against this engine's slice and bounds
int rebalance_make_plan(bpf_engine* e, const long long* counts, int rank, int world, RebalancePlan* R)
{
  if (!counts || world < 1 || world > kMailboxMaxWorld || rank < 0 || rank >= world)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance: 1 .. 16 ranks and a rank among them");
  if (!rebalance_plan(counts, world, R))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance: a negative sample count");
  if (counts[rank] != (long long)e->sample_count)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance: counts[rank] is not this engine's sample count");
  if (R->P[world] > (long long)e->max_samples)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance: the global set is beyond max_samples");
  return BPF_OK;
}

// this rank's outgoing samples into d_rb_rows = int64[4][out[rank]]
int rebalance_pack(bpf_engine* e, const RebalancePlan& R, int rank)
{
  const long long n_out = R.out[rank];
  HIPCHK(e, e->d_rb_rows.reserve((size_t)std::max<long long>(4 * n_out, 4)));
  if (n_out == 0)
    return BPF_OK;
  RebalancePackArgs A{};
  A.src = e->sets[e->cur].dev();
  A.head = R.keep_lo[rank] - R.P[rank];
  A.keep_n = R.keep_n[rank];
  A.n_out = n_out;
  A.rows = e->d_rb_rows.p;
  // a latency-bound copy: the grid of the small exchanges (ShardExchange::small_grid), the loop takes the rest
  hipLaunchKernelGGL(k_rebalance_pack, dim3((unsigned)ShardExchange::small_grid(n_out)), dim3(256), 0, e->stream, A);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// this rank's new slice into the set that is NOT current; nothing of the engine's filter state changes
int rebalance_assemble(bpf_engine* e, const RebalancePlan& R, int rank, const long long* rows, const long long* rank_off,
                       long long row_stride)
{
  RebalanceAssembleArgs A{};
  A.world = R.world;
  A.rank = rank;
  A.q_first = R.Q[rank];
  A.n_new = R.Q[rank + 1] - R.Q[rank];
  if (A.n_new == 0)
    return BPF_OK;
  for (int r = 0; r < R.world; ++r)
  {
    A.P[r] = R.P[r];
    A.keep_lo[r] = R.keep_lo[r];
    A.keep_n[r] = R.keep_n[r];
    A.rank_off[r] = rank_off[r];
  }
  A.P[R.world] = R.P[R.world];
  A.row_stride = row_stride;
  A.rows = rows;
  A.src = e->sets[e->cur].dev();
  A.dst = e->sets[e->cur ^ 1].dev();
  hipLaunchKernelGGL(k_rebalance_assemble, dim3((unsigned)((A.n_new + 255) / 256)), dim3(256), 0, e->stream, A);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// the split is even already: the set, its epoch and its caches stay; where the slice sits is now known
void rebalance_record_slice(bpf_engine* e, const RebalancePlan& R, int rank)
{
  e->slice_first = R.P[rank];
  e->slice_global = R.P[R.world];
}

// plan, pack, one gather, assemble, transition -- over the engine's exchange, from counts every rank holds alike
int shard_rebalance_run(bpf_engine* e, ShardExchange& X, const long long* counts, long long* moved_out)
{
  const int rank = e->shard_rank, W = e->shard_world;
  RebalancePlan R;
  int rc = rebalance_make_plan(e, counts, rank, W, &R);
  if (rc != BPF_OK)
    return rc;
  e->rb_rank = -1;  // a staged plan does not outlive this
  *moved_out = 0;     // what a failed exchange below reports: nothing has moved
  e->rb_last_moved = 0;
  if (R.moved == 0)
  {
    rebalance_record_slice(e, R, rank);
    return BPF_OK;
  }
  rc = rebalance_pack(e, R, rank);
  if (rc != BPF_OK)
    return rc;
  const long long T = R.moved, n_out = R.out[rank];
  HIPCHK(e, e->d_rb_gather.reserve((size_t)4 * (size_t)T));
  long long offs[kMailboxMaxWorld] = { 0 }, at = 0;
  for (int r = 0; r < W; ++r)
  {
    offs[r] = at;
    at += R.out[r];
  }
  const long long* src[4] = { e->d_rb_rows.p, e->d_rb_rows.p + n_out, e->d_rb_rows.p + 2 * n_out,
                              e->d_rb_rows.p + 3 * n_out };
  rc = X.gather(src, 4, R.out, e->d_rb_gather.p, offs, T);
  if (rc == BPF_OK)
    rc = X.finish();  // every exchange is finished before the new slice becomes current
  if (rc != BPF_OK)
    return rc;
  rc = rebalance_assemble(e, R, rank, e->d_rb_gather.p, offs, T);
  if (rc != BPF_OK)
    return rc;
  e->slice_rebalanced((int)(R.Q[rank + 1] - R.Q[rank]), R.Q[rank], R.P[W]);
  *moved_out = R.moved;
  e->rb_last_moved = R.moved;
  return BPF_OK;
}

// bpf_shard_update_resample behind an in-place resample with BPF_SHARD_REBALANCE_AUTO set: the counts are the
// resample's own (e->ip_counts, the same on every rank), so every rank decides alike and no count crosses
int shard_rebalance_auto(bpf_engine* e)
{
  const int W = e->shard_world;
  long long counts[kMailboxMaxWorld] = { 0 }, largest = 0, total = 0;
  for (int r = 0; r < W; ++r)
  {
    counts[r] = e->ip_counts[r];
    largest = std::max(largest, counts[r]);
    total += counts[r];
  }
  e->rb_last_moved = 0;
  const long long even = (total + W - 1) / W;
  if (!((double)largest > e->shard_trigger_share * (double)even))
    return BPF_OK;
  ShardExchange X{ e };
  long long moved = 0;
  return shard_rebalance_run(e, X, counts, &moved);
}

int rebalance_staged_ready(bpf_engine* e, const char* what)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  if (e->rb_rank < 0 || e->rb_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, what);
  return BPF_OK;
}
}  // namespace

int bpf_shard_set_rebalance(bpf_engine* e, int mode, double trigger_share)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (mode != BPF_SHARD_REBALANCE_OFF && mode != BPF_SHARD_REBALANCE_AUTO)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance mode: BPF_SHARD_REBALANCE_OFF or BPF_SHARD_REBALANCE_AUTO");
  if (!(trigger_share >= 1.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance: trigger_share >= 1 (1: any uneven split is rebalanced)");
  e->shard_rebalance = mode;
  e->shard_trigger_share = trigger_share;
  return BPF_OK;
}

int bpf_shard_get_rebalance(const bpf_engine* e, int* mode_out, double* trigger_share_out)
{
  if (!e || !mode_out || !trigger_share_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *mode_out = e->shard_rebalance;
  *trigger_share_out = e->shard_trigger_share;
  return BPF_OK;
}

int bpf_shard_rebalance_last(const bpf_engine* e, long long* moved_out)
{
  if (!e || !moved_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *moved_out = e->rb_last_moved;
  return BPF_OK;
}

int bpf_shard_resample_committed(const bpf_engine* e, int* committed_out)
{
  if (!e || !committed_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *committed_out = e->resample_committed ? 1 : 0;
  return BPF_OK;
}

int bpf_shard_rebalance(bpf_engine* e, long long* moved_out)
{
  if (!e || !moved_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  long long counts[kMailboxMaxWorld] = { 0 }, first = 0, total = 0;
  rc = shard_gather_counts(e, X, "rebalance", counts, &first, &total);
  if (rc != BPF_OK)
    return rc;
  return shard_rebalance_run(e, X, counts, moved_out);
}

int bpf_shard_rebalance_plan(bpf_engine* e, const long long* counts, int rank, int world, long long* out_counts,
                             long long* new_first_out, int* new_count_out)
{
  if (!e || !out_counts || !new_first_out || !new_count_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  RebalancePlan R;
  int rc = rebalance_make_plan(e, counts, rank, world, &R);
  if (rc != BPF_OK)
    return rc;
  for (int r = 0; r < world; ++r)
    out_counts[r] = R.out[r];
  *new_first_out = R.Q[rank];
  *new_count_out = (int)(R.Q[rank + 1] - R.Q[rank]);
  e->rb_plan = R;
  e->rb_rank = rank;
  e->rb_epoch = e->set_epoch;
  return BPF_OK;
}

int bpf_shard_rebalance_export_dev(bpf_engine* e, void** rows_dev, long long* n_out)
{
  if (!e || !rows_dev || !n_out)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = rebalance_staged_ready(e, "rebalance: bpf_shard_rebalance_plan of the current set first");
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  rc = rebalance_pack(e, e->rb_plan, e->rb_rank);
  if (rc != BPF_OK)
    return rc;
  *rows_dev = e->d_rb_rows.p;
  *n_out = e->rb_plan.out[e->rb_rank];
  return BPF_OK;
}

int bpf_shard_rebalance_import_dev(bpf_engine* e, const void* rows_dev, const long long* rank_off, long long row_stride)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = rebalance_staged_ready(e, "rebalance: bpf_shard_rebalance_plan of the current set first");
  if (rc != BPF_OK)
    return rc;
  const RebalancePlan& R = e->rb_plan;
  const int rank = e->rb_rank;
  if (R.moved == 0)
  {
    rebalance_record_slice(e, R, rank);
    e->rb_last_moved = 0;
    e->rb_rank = -1;
    return BPF_OK;
  }
  if (!rows_dev || !rank_off || row_stride < 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance import: the gathered rows, their offsets and their row stride");
  for (int r = 0; r < R.world; ++r)
    if (rank_off[r] < 0 || R.out[r] > row_stride)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "rebalance import: a negative offset, or a row shorter than a rank's list");
  HIPCHK(e, hipSetDevice(e->device));
  rc = rebalance_assemble(e, R, rank, static_cast<const long long*>(rows_dev), rank_off, row_stride);
  if (rc != BPF_OK)
    return rc;
  e->rb_last_moved = R.moved;
  e->slice_rebalanced((int)(R.Q[rank + 1] - R.Q[rank]), R.Q[rank], R.P[R.world]);
  e->rb_rank = -1;
  return BPF_OK;
}
