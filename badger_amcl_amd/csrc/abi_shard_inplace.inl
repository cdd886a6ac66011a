// C-ABI: the systematic resample of a sharded set in place (kernels_shard_inplace.hpp).  Stage functions for a host
// with a transport of its own -- no call here waits for another rank -- and the one-call form that
// bpf_shard_update_resample takes over the engine's exchange (ShardExchange, abi_mailbox_step.inl).
// ---------------------------------------------------------------------- in-place systematic resample
namespace
{
struct InplacePlan
{
  int counts[kMailboxMaxWorld];        // samples of every rank's new slice (rank 0: its random poses included)
  int first_tooth[kMailboxMaxWorld];   // rank's first tooth in ascending-target order
  double edge[kMailboxMaxWorld + 1];   // the slices of the global CDF: shard q owns [edge[q], edge[q + 1])
  int n_random = 0;
  bool in_place = false;               // false: the imbalance cap sends this resample to the window form
};

// The slices of the global CDF, edge[0 .. world], from the ranks' weight sums on the device (one wait for the stream).
// They are shard_slice's: the same additions and quotients in the same order, so every rank -- and the window kernel
// -- gets the same doubles.  Both in-place resamples, systematic and multinomial, take their slices from here.
int inplace_edges(bpf_engine* e, const void* sums_dev, int sums_are_totals, int world, double* edge)
{
  double sums[kMailboxMaxWorld];
  H2D_OR_RETURN(small_down_sync(e, sums, static_cast<const double*>(sums_dev), (size_t)world, e->stream));
  double T = 1.0;
  if (sums_are_totals)
  {
    T = 0.0;
    for (int r = 0; r < world; ++r)
      T += sums[r];
  }
  double offset = 0.0;
  edge[0] = 0.0;
  for (int r = 0; r < world; ++r)
  {
    offset += sums_are_totals ? sums[r] / T : sums[r];
    if (!(offset >= edge[r]))
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample: a shard's weight sum is negative or not a number");
    edge[r + 1] = offset;
  }
  return BPF_OK;
}

// The ascending targets into e->h_targets and every rank's share of them.  The targets are the reference's serial
// chain (particle_filter.cpp:337-341) as systematic_window_args forms it; the teeth formed after the subtraction are
// the small ones, so the ascending order is the chain rotated by i_wrap.
int inplace_plan(bpf_engine* e, uint64_t rng_state48, int count, const void* sums_dev, int sums_are_totals, int world,
                 InplacePlan* P)
{
  const int n_random = e->shard_n_random;
  if (n_random < 0 || n_random >= count)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample: random pose count out of range");
  H2D_OR_RETURN(inplace_edges(e, sums_dev, sums_are_totals, world, P->edge));
  const int n = count - n_random;
  HIPCHK(e, e->h_targets.reserve((size_t)std::max(count, e->max_samples)));
  if (e->targets_read)  // a previous kernel may still be reading the pinned targets
    HIPCHK(e, hipEventSynchronize(e->targets_read));
  double* t = e->h_targets.p;
  const uint64_t st = lcg_skip_host(rng_state48 & ((1ull << 48) - 1), 1, e->jump);
  double target = std::ldexp((double)st, -48);
  const double delta = 1.0 / n;
  int i_wrap = n;  // the first tooth formed after the subtraction
  for (int i = 0; i < n; ++i)
  {
    t[i] = target;
    target += delta;
    if (target > 1.0)
    {
      target -= 1.0;
      if (i_wrap == n)
        i_wrap = i + 1;
    }
  }
  std::rotate(t, t + i_wrap, t + n);
  for (int j = 1; j < n; ++j)
    if (t[j] < t[j - 1])
      return e->fail(BPF_ERR_HIP, "in-place resample: the rotated targets do not ascend (internal error)");
  P->n_random = n_random;
  P->first_tooth[0] = 0;
  for (int q = 1; q < world; ++q)
    P->first_tooth[q] = (int)(std::lower_bound(t, t + n, P->edge[q]) - t);  // teeth below the slice: not >= offset
  int largest = 0;
  for (int q = 0; q < world; ++q)
  {
    P->counts[q] = (q + 1 < world ? P->first_tooth[q + 1] : n) - P->first_tooth[q] + (q == 0 ? n_random : 0);
    largest = std::max(largest, P->counts[q]);
  }
  const long long even = ((long long)count + world - 1) / world;
  // BPF_SHARD_REBALANCE_AUTO: the select always runs in place (a slice never exceeds count <= max_samples) and the
  // rebalance behind the resample evens the slices out; otherwise the cap decides
  P->in_place = e->shard_rebalance == BPF_SHARD_REBALANCE_AUTO || !((double)largest > e->shard_max_share * (double)even);
  return BPF_OK;
}

// this rank's new slice into the set that is NOT current; nothing of the engine's filter state changes
int inplace_select_write(bpf_engine* e, uint64_t rng_state48, int count, int rank, int world, void* flags_dev,
                         const InplacePlan& P)
{
  const int n_new = P.counts[rank];
  if (n_new > e->max_samples)
    return e->fail(BPF_ERR_CAPACITY, "in-place resample: slice larger than max_samples");
  if (n_new == 0)
    return BPF_OK;
  if (e->sample_count > 0 && !e->d_cdf.p)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_build_cdf first");
  InplaceSelectArgs A{};
  A.W.src = e->sets[e->cur].dev();
  A.W.n_src = e->sample_count;
  A.W.cdf = e->d_cdf.p;
  A.W.rank = rank;
  A.W.world = world;
  A.W.m0 = 0;
  A.W.m1 = n_new;
  A.W.rng_state = rng_state48 & ((1ull << 48) - 1);
  A.W.jump = e->jump;
  A.W.flags = static_cast<int*>(flags_dev);
  A.W.targets = e->h_targets.p + P.first_tooth[rank];
  if (rank == 0 && P.n_random > 0)
  {
    A.W.n_random = P.n_random;
    A.W.write_random = 1;
    int rcf = ensure_free_space(e, &A.W.free_space);
    if (rcf != BPF_OK)
      return rcf;
  }
  A.offset = P.edge[rank];
  A.top = P.edge[rank + 1];
  A.dst = e->sets[e->cur ^ 1].dev();
  A.weight = 1.0 / (double)count;
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_systematic_select_local, dim3(blocks_for(n_new, 256)), dim3(256), 0, e->stream, A);
  }
  HIPCHK(e, hipGetLastError());
  return systematic_targets_in_use(e);
}

int inplace_check_begin(bpf_engine* e, uint64_t rng_state48, int count, const void* sums_dev, int rank, int world,
                        void* flags_dev)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  if (!sums_dev || !flags_dev || count <= 0 || count > e->max_samples || rank < 0 || rank >= world ||
      world > kMailboxMaxWorld)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "bad in-place resample arguments");
  if (e->resample_model != BPF_RESAMPLE_SYSTEMATIC)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample: the multinomial resampler keeps the draw window");
  if ((rng_state48 & ((1ull << 48) - 1)) != e->shard_rng0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample does not belong to the resample begun");
  return BPF_OK;
}

// the selected slice becomes the current set; its tree counts follow from the bin lists (bpf_shard_tree_*)
void inplace_commit(bpf_engine* e, int n_new, long long first, int count)
{
  e->new_set(n_new, true, TreeCounts{ -1, -1, e->tree.gt_route, false });
  e->slice_first = first;
  e->slice_global = count;
  e->shard_form_used = BPF_SHARD_RESAMPLE_IN_PLACE;
}

int inplace_words(bpf_engine* e)
{
  HIPCHK(e, e->d_ip_words.reserve(32));
  return BPF_OK;
}

// limb sums of x and y of `n` samples of `s`, and the flag: d_ip_words[0 .. kInplaceSumWords)
int inplace_xy_sums(bpf_engine* e, SampleSet& s, int n)
{
  int rc = inplace_words(e);
  if (rc != BPF_OK)
    return rc;
  long long* p = e->d_ip_words.p;
  HIPCHK(e, hipMemsetAsync(p, 0, 32 * sizeof(long long), e->stream));
  long long *acc_hi = p + 24, *acc_top = p + 26;
  unsigned long long* acc_lo = reinterpret_cast<unsigned long long*>(p + 28);
  if (n > 0)
    hipLaunchKernelGGL(k_inplace_xy_sums, dim3(std::min(blocks_for(n, 256), 1024)), dim3(256), 0, e->stream,
                       (const double*)s.x.p, (const double*)s.y.p, n, acc_top, acc_hi, acc_lo, p);
  hipLaunchKernelGGL(k_inplace_export, dim3(1), dim3(64), 0, e->stream, (const long long*)acc_top,
                     (const long long*)acc_hi, (const unsigned long long*)acc_lo, p);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// the slice's particles within dist_threshold of the mean of the reduced sums: d_ip_words[16]
int inplace_count(bpf_engine* e, SampleSet& s, int n, const void* reduced_dev, int global_count)
{
  long long* cnt = e->d_ip_words.p + 16;
  HIPCHK(e, hipMemsetAsync(cnt, 0, sizeof(long long), e->stream));
  if (n > 0)
  {
    hipLaunchKernelGGL(k_inplace_converged_count, dim3(std::min(blocks_for(n, 256), 1024)), dim3(256), 0, e->stream,
                       (const double*)s.x.p, (const double*)s.y.p, n, static_cast<const long long*>(reduced_dev),
                       global_count, e->dist_threshold, cnt);
    HIPCHK(e, hipGetLastError());
  }
  return BPF_OK;
}

// the reduced count where fetch_scalars turns it into `converged` (the single engine's float percentage test)
int inplace_converged_install(bpf_engine* e, const void* reduced_count_dev, int global_count)
{
  HIPCHK(e, e->d_flags.reserve(8));
  HIPCHK(e, copy_d2d(e->d_flags.p + 1, static_cast<const int*>(reduced_count_dev), 1, e->stream));
  e->converged_pending = true;
  e->conv_n = global_count;
  return BPF_OK;
}

// The tail of both in-place forms over the engine's exchange (the multinomial one: abi_shard_inplace_mn.inl).  The spare
// set holds this rank's counts[rank] samples of the new set of `count`: the converged test's two reductions, and --
// every exchange finished -- the slice becomes current with the counts of the global set's tree.
int inplace_finish(bpf_engine* e, ShardExchange& X, const int* counts, int count, int leaf, int bins, int route,
                   int* leaf_out, int* bins_out)
{
  const int rank = e->shard_rank, W = e->shard_world, n_new = counts[rank];
  long long first = 0;
  for (int r = 0; r < rank; ++r)
    first += counts[r];
  SampleSet& s = e->sets[e->cur ^ 1];
  int rc = inplace_xy_sums(e, s, n_new);
  if (rc == BPF_OK)
    rc = X.reduce_sum(e->d_ip_words.p, (size_t)kInplaceSumWords, false);  // limb form: the lane-wise sum is exact
  if (rc == BPF_OK)
    rc = inplace_count(e, s, n_new, e->d_ip_words.p, count);
  if (rc == BPF_OK)
    rc = X.reduce_sum(e->d_ip_words.p + 16, 1, false);
  if (rc == BPF_OK)
    rc = X.finish();
  if (rc != BPF_OK)
    return rc;
  inplace_commit(e, n_new, first, count);
  for (int r = 0; r < W; ++r)
    e->ip_counts[r] = counts[r];
  tree_install(e, leaf, bins, route);
  rc = inplace_converged_install(e, e->d_ip_words.p + 16, count);
  if (rc != BPF_OK)
    return rc;
  *leaf_out = e->tree.leaf_count;
  *bins_out = e->tree.bin_count;
  return BPF_OK;
}

// bpf_shard_update_resample's systematic branch with the in-place form set: *done = false when the imbalance cap sends
// this resample to the window form (nothing was changed).  Every exchange is finished before the new slice becomes
// current, so a wait that runs out leaves the set as it was, as the window form does.
int shard_update_resample_in_place(bpf_engine* e, void* flags_dev, uint64_t rng, int count, bool* done, int* leaf_out,
                                   int* bins_out)
{
  *done = false;
  const int rank = e->shard_rank, W = e->shard_world;
  int rc = inplace_check_begin(e, rng, count, e->mb_totals, rank, W, flags_dev);
  if (rc != BPF_OK)
    return rc;
  InplacePlan P;
  rc = inplace_plan(e, rng, count, e->mb_totals, 1, W, &P);
  if (rc != BPF_OK)
    return rc;
  if (!P.in_place)
    return BPF_OK;
  rc = inplace_select_write(e, rng, count, rank, W, flags_dev, P);
  if (rc != BPF_OK)
    return rc;
  ShardExchange X{ e };
  long long counts[kMailboxMaxWorld] = { 0 }, first = 0;
  for (int r = 0; r < W; ++r)
  {
    counts[r] = P.counts[r];
    if (r < rank)
      first += P.counts[r];
  }
  int leaf = 0, bins = 0, route = 0;
  rc = shard_spare_tree(e, X, P.counts[rank], first, counts, &leaf, &bins, &route);
  if (rc == BPF_OK)
    rc = inplace_finish(e, X, P.counts, count, leaf, bins, route, leaf_out, bins_out);
  *done = rc == BPF_OK;
  return rc;
}
}  // namespace

int bpf_shard_set_resample_form(bpf_engine* e, int form, double max_share)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (form != BPF_SHARD_RESAMPLE_WINDOW && form != BPF_SHARD_RESAMPLE_IN_PLACE)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "resample form: BPF_SHARD_RESAMPLE_WINDOW or BPF_SHARD_RESAMPLE_IN_PLACE");
  if (!(max_share >= 1.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "resample form: max_share >= 1 (1: only an even split stays in place)");
  e->shard_form = form;
  e->shard_max_share = max_share;
  return BPF_OK;
}

int bpf_shard_get_resample_form(const bpf_engine* e, int* form_out, double* max_share_out)
{
  if (!e || !form_out || !max_share_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *form_out = e->shard_form;
  *max_share_out = e->shard_max_share;
  return BPF_OK;
}

int bpf_shard_slice(bpf_engine* e, long long* global_first_out, int* local_count_out, int* form_used_out)
{
  if (!e || !global_first_out || !local_count_out || !form_used_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  if (e->slice_first < 0)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "no sharded init or resample has recorded this engine's slice");
  *global_first_out = e->slice_first;
  *local_count_out = e->sample_count;
  *form_used_out = e->shard_form_used;
  return BPF_OK;
}

int bpf_shard_inplace_select_dev(bpf_engine* e, uint64_t rng_state48, int count, const void* sums_dev,
                                 int sums_are_totals, int rank, int world, void* flags_dev, int* counts_out,
                                 long long* global_first_out, int* form_used_out)
{
  if (!e || !counts_out || !global_first_out || !form_used_out)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = inplace_check_begin(e, rng_state48, count, sums_dev, rank, world, flags_dev);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  InplacePlan P;
  rc = inplace_plan(e, rng_state48, count, sums_dev, sums_are_totals, world, &P);
  if (rc != BPF_OK)
    return rc;
  long long first = 0;
  for (int r = 0; r < world; ++r)
  {
    counts_out[r] = P.counts[r];
    if (r < rank)
      first += P.counts[r];
  }
  *global_first_out = first;
  *form_used_out = P.in_place ? BPF_SHARD_RESAMPLE_IN_PLACE : BPF_SHARD_RESAMPLE_WINDOW;
  e->ip_stage = 0;
  if (!P.in_place)
    return BPF_OK;
  rc = inplace_select_write(e, rng_state48, count, rank, world, flags_dev, P);
  if (rc != BPF_OK)
    return rc;
  inplace_commit(e, P.counts[rank], first, count);
  e->ip_stage = 1;
  e->ip_epoch = e->set_epoch;
  return BPF_OK;
}

int bpf_shard_inplace_xy_sums_dev(bpf_engine* e, void** words_dev, size_t* n_words_out)
{
  if (!e || !words_dev || !n_words_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (e->ip_stage < 1 || e->ip_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_inplace_select_dev first");
  HIPCHK(e, hipSetDevice(e->device));
  int rc = inplace_xy_sums(e, e->sets[e->cur], e->sample_count);
  if (rc != BPF_OK)
    return rc;
  e->ip_stage = 2;
  *words_dev = e->d_ip_words.p;
  *n_words_out = (size_t)kInplaceSumWords;
  return BPF_OK;
}

int bpf_shard_inplace_converged_dev(bpf_engine* e, const void* reduced_words_dev, int global_count, void** count_dev)
{
  if (!e || !reduced_words_dev || !count_dev || global_count <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (e->ip_stage != 2 || e->ip_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_inplace_xy_sums_dev first");
  HIPCHK(e, hipSetDevice(e->device));
  int rc = inplace_count(e, e->sets[e->cur], e->sample_count, reduced_words_dev, global_count);
  if (rc != BPF_OK)
    return rc;
  e->ip_stage = 3;
  *count_dev = e->d_ip_words.p + 16;
  return BPF_OK;
}

int bpf_shard_inplace_converged_finish(bpf_engine* e, const void* reduced_count_dev, int global_count)
{
  if (!e || !reduced_count_dev || global_count <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (e->ip_stage != 3 || e->ip_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_inplace_converged_dev first");
  HIPCHK(e, hipSetDevice(e->device));
  e->ip_stage = 0;
  return inplace_converged_install(e, reduced_count_dev, global_count);
}
