// C-ABI: what a C / C++ host of a sharded filter still needed a transport of its own for -- the 3-D sensor update and
// the statistics of the GLOBAL set -- as one collective call each.  Every exchange goes through ShardExchange
// (abi_mailbox_step.inl): the mailbox's peer stores, or RCCL after the bootstrap's fallback.  The stage functions run
// in the order badger_amcl_amd/sharded.py runs them (update_sensor, _ensure_stats); there is no arithmetic here.
// The sequences that more than one of the one-call forms runs are written once, here: shard_gather_counts (the sample
// counts, this rank's first index, the total), shard_gather_slices_host, shard_exchange_bin_lists
// (ShardedFilter._exchange_bin_lists), shard_global_tree and shard_spare_tree (ShardedFilter._global_tree).  The checks
// of gathered bin lists are bin_lists_check (abi_shard_stats.inl) and gtree_merge_begin (abi_shard_init.inl); the tail
// of both in-place resamples is inplace_finish (abi_shard_inplace.inl: ShardedFilter._finish_in_place).
namespace
{
// a few int64 words of every rank into host memory: all[r * n_each + k], in rank order (waits for the stream)
int shard_gather_host_words(bpf_engine* e, ShardExchange& X, const long long* mine, int n_each, long long* all)
{
  const int W = e->shard_world;
  const size_t n_all = (size_t)W * (size_t)n_each;
  HIPCHK(e, e->d_x_words.reserve((size_t)(kMailboxMaxWorld + 1) * 4));
  HIPCHK(e, e->h_x_words.reserve((size_t)(kMailboxMaxWorld + 1) * 4));
  if (n_each < 1 || n_each > 4)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "shard gather: 1 .. 4 words per rank");
  long long counts[kMailboxMaxWorld], offs[kMailboxMaxWorld];
  for (int r = 0; r < W; ++r)
  {
    counts[r] = n_each;
    offs[r] = (long long)r * n_each;
  }
  for (int k = 0; k < n_each; ++k)
    e->h_x_words.p[k] = mine[k];
  H2D_OR_RETURN(pinned_up(e, e->d_x_words, 0, e->h_x_words, 0, (size_t)n_each, e->stream));
  const long long* src[1] = { e->d_x_words.p };
  int rc = X.gather(src, 1, counts, e->d_x_words.p + 4, offs, 0);
  if (rc != BPF_OK)
    return rc;
  H2D_OR_RETURN(pinned_down(e, e->h_x_words, 4, e->d_x_words, 4, n_all, e->stream));
  rc = X.finish();
  if (rc != BPF_OK)
    return rc;
  for (size_t i = 0; i < n_all; ++i)
    all[i] = e->h_x_words.p[4 + i];
  return BPF_OK;
}

// every rank's sample count (one exchange), this rank's first global index and the total; the bound on the total is
// the caller's
int shard_gather_counts(bpf_engine* e, ShardExchange& X, const std::string& prefix, long long* counts, long long* first,
                        long long* total)
{
  const long long mine = e->sample_count;
  int rc = shard_gather_host_words(e, X, &mine, 1, counts);
  if (rc != BPF_OK)
    return rc;
  *first = *total = 0;
  for (int r = 0; r < e->shard_world; ++r)
  {
    if (counts[r] < 0)
      return e->fail(BPF_ERR_EXCHANGE, prefix + ": a negative sample count arrived");
    if (r < e->shard_rank)
      *first += counts[r];
    *total += counts[r];
  }
  return BPF_OK;
}

// x / y / theta / weight of every slice, concatenated in rank order: d_x_gather = double[4][n]
int shard_gather_slices(bpf_engine* e, ShardExchange& X, const long long* counts, int n, SampleSet* set = nullptr)
{
  const int W = e->shard_world;
  HIPCHK(e, e->d_x_gather.reserve((size_t)4 * (size_t)n));
  SampleSet& s = set ? *set : e->sets[e->cur];
  const long long* src[4] = { reinterpret_cast<const long long*>(s.x.p), reinterpret_cast<const long long*>(s.y.p),
                              reinterpret_cast<const long long*>(s.th.p), reinterpret_cast<const long long*>(s.w.p) };
  long long offs[kMailboxMaxWorld], at = 0;
  for (int r = 0; r < W; ++r)
  {
    offs[r] = at;
    at += counts[r];
  }
  return X.gather(src, 4, counts, e->d_x_gather.p, offs, n);
}

// the same, and the first `rows` of the four in host memory behind X.finish(): soa = double[rows][n]
int shard_gather_slices_host(bpf_engine* e, ShardExchange& X, const long long* counts, int n, int rows,
                             std::vector<double>* soa, SampleSet* set = nullptr)
{
  int rc = shard_gather_slices(e, X, counts, n, set);
  if (rc != BPF_OK)
    return rc;
  soa->resize((size_t)rows * (size_t)n);
  // (the pageable way down returns with the stream drained: finish()'s wait finds nothing left to wait for)
  H2D_OR_RETURN(d2h_to_host(e, soa->data(), e->d_x_gather.p, soa->size() * sizeof(double), e->stream));
  return X.finish();
}

// The ranks' bin lists of a merge stage (statistics labels, the global tree).  Every rank's (n_bins, flag) pair crosses
// first and the counts are checked against the slices (counts[]); *any_flag: some rank raised its flag -- it
// travelled with the counts, so every rank turns off to its caller's other route here together, and no list crosses.
// Otherwise the lists (`bins`: this rank's int64[2][n_bins]) cross, as their readers take them:
// d_x_gather = int64[world][2][*pad_out], zero-filled.
int shard_exchange_bin_lists(bpf_engine* e, ShardExchange& X, const long long* bins, int n_bins, int flag,
                             const long long* counts, const char* bad_count, int* bin_counts_i, int* pad_out,
                             bool* any_flag)
{
  const int W = e->shard_world;
  const long long meta[2] = { n_bins, flag };
  long long metas[2 * kMailboxMaxWorld] = { 0 };
  int rc = shard_gather_host_words(e, X, meta, 2, metas);
  if (rc != BPF_OK)
    return rc;
  long long bin_counts[kMailboxMaxWorld], offs[kMailboxMaxWorld], pad = 1;
  *any_flag = false;
  for (int r = 0; r < W; ++r)
  {
    bin_counts[r] = metas[2 * r];
    if (bin_counts[r] < 0 || bin_counts[r] > counts[r])
      return e->fail(BPF_ERR_EXCHANGE, bad_count);
    bin_counts_i[r] = (int)bin_counts[r];
    pad = std::max(pad, bin_counts[r]);
    *any_flag = *any_flag || metas[2 * r + 1] != 0;
  }
  *pad_out = (int)pad;
  if (*any_flag)
    return BPF_OK;
  const size_t flat = (size_t)W * 2 * (size_t)pad;
  HIPCHK(e, e->d_x_gather.reserve(flat));
  HIPCHK(e, hipMemsetAsync(e->d_x_gather.p, 0, flat * sizeof(long long), e->stream));
  const long long* src[2] = { bins, bins + n_bins };
  for (int r = 0; r < W; ++r)
    offs[r] = (long long)r * 2 * pad;
  rc = X.gather(src, 2, bin_counts, e->d_x_gather.p, offs, pad);
  return rc == BPF_OK ? X.finish() : rc;
}

// ShardedFilter._ensure_stats
int shard_ensure_stats(bpf_engine* e)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  if (e->ss_global_epoch == e->set_epoch && e->stats_epoch == e->set_epoch)
    return BPF_OK;  // no slice has changed since the global figures were installed: no exchange
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  const int W = e->shard_world;
  long long counts[kMailboxMaxWorld] = { 0 }, total = 0, first = 0;
  rc = shard_gather_counts(e, X, "sharded statistics", counts, &first, &total);
  if (rc != BPF_OK)
    return rc;
  if (total <= 0 || total >= (1ll << 30))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "sharded statistics: the global set is empty, or beyond 2^30 samples");
  const int n = (int)total;
  int route = 0;
  if (n <= kStatBlockMax)
  {
    // the tracking regime: the whole set on every rank, evaluated redundantly
    rc = shard_gather_slices(e, X, counts, n);
    if (rc == BPF_OK)
      rc = X.finish();
    if (rc != BPF_OK)
      return rc;
    const double* d = reinterpret_cast<const double*>(e->d_x_gather.p);
    int handled = BPF_SHARD_STATS_DECLINED;
    rc = bpf_shard_stats_gathered_dev(e, d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, &handled);
    if (rc != BPF_OK)
      return rc;
    if (handled == BPF_SHARD_STATS_INSTALLED)
      route = BPF_SHARD_STATS_ROUTE_GATHERED;
    else if (handled == BPF_SHARD_STATS_HOST_ROUTE)
      route = BPF_SHARD_STATS_ROUTE_HOST;
  }
  if (route == 0)
  {
    void* bins = nullptr;
    int n_bins = 0, host_route = 0;
    rc = bpf_shard_stats_local_bins_dev(e, first, &bins, &n_bins, &host_route);
    if (rc != BPF_OK)
      return rc;
    int bin_counts_i[kMailboxMaxWorld], pad = 1;
    bool any_host = false;
    rc = shard_exchange_bin_lists(e, X, static_cast<const long long*>(bins), n_bins, host_route, counts,
                                  "sharded statistics: a bin count outside its slice arrived", bin_counts_i, &pad,
                                  &any_host);
    if (rc != BPF_OK)
      return rc;
    if (any_host)
      route = BPF_SHARD_STATS_ROUTE_HOST;
    else
    {
      int clusters = 0;
      rc = bpf_shard_stats_label_dev(e, e->d_x_gather.p, bin_counts_i, W, pad, &clusters);
      if (rc != BPF_OK)
        return rc;
      void* sums = nullptr;
      size_t n_words = 0;
      rc = bpf_shard_stats_local_sums_dev(e, &sums, &n_words);
      if (rc != BPF_OK)
        return rc;
      rc = X.reduce_sum(sums, n_words, false);  // limb form: the lane-wise int64 sum is exact
      if (rc == BPF_OK)
        rc = X.finish();
      if (rc != BPF_OK)
        return rc;
      rc = bpf_shard_stats_finish_dev(e, sums);
      if (rc != BPF_OK)
        return rc;
      // sums beyond the fixed-point format: every rank read the same reduced words and decides alike
      route = e->ss_finish_installed ? BPF_SHARD_STATS_ROUTE_DISTRIBUTED : BPF_SHARD_STATS_ROUTE_HOST;
    }
  }
  if (route == BPF_SHARD_STATS_ROUTE_HOST)
  {
    std::vector<double> soa, all((size_t)4 * (size_t)n);
    rc = shard_gather_slices_host(e, X, counts, n, 4, &soa);
    if (rc != BPF_OK)
      return rc;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 4; ++k)
        all[4 * (size_t)i + k] = soa[(size_t)k * (size_t)n + i];
    rc = bpf_shard_stats_host(e, all.data(), n);
    if (rc != BPF_OK)
      return rc;
  }
  e->ss_global_epoch = e->set_epoch;
  e->ss_route = route;
  return BPF_OK;
}
}  // namespace

int bpf_shard_update_sensor_cloud(bpf_engine* e, const float* points_xyz, int n_points, long long global_count)
{
  if (!e || global_count <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  ShardExchange X{ e };
  e->mb_totals_valid = false;
  rc = bpf_shard_score_cloud(e, points_xyz, n_points);
  if (rc != BPF_OK)
    return rc;
  if (e->cloud_max_beams < 2)
    return BPF_OK;  // PointCloudScanner::updateSensor returns false (point_cloud_scanner.cpp:95-96): nothing was posted
  return shard_totals_and_normalize(e, X, global_count);
}

int bpf_shard_compute_cluster_stats(bpf_engine* e, int* cluster_count_out, double set_mean[3], double set_cov[5],
                                    int* route_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_ensure_stats(e);
  if (rc != BPF_OK)
    return rc;
  if (route_out)
    *route_out = e->ss_route;
  return bpf_pf_compute_cluster_stats(e, cluster_count_out, set_mean, set_cov);
}

int bpf_shard_get_max_weight_pose(bpf_engine* e, double* max_weight, double pose[3])
{
  if (!e || !max_weight || !pose)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_ensure_stats(e);
  if (rc != BPF_OK)
    return rc;
  return bpf_pf_get_max_weight_pose(e, max_weight, pose);
}

namespace
{
// The tree of the GLOBAL set (abi_shard_init.inl) over the engine's exchange: `s` holds this rank's n samples from
// global index `first`, counts[] every rank's sample count.  Installs the counts; a failed exchange installs nothing.
int shard_global_tree(bpf_engine* e, ShardExchange& X, SampleSet& s, int n, long long first, const long long* counts,
                      int* leaf_out, int* bins_out)
{
  const int W = e->shard_world;
  int n_bins = 0, out_of_range = 0;
  int rc = tree_local_bins(e, s, n, first, &n_bins, &out_of_range);
  if (rc != BPF_OK)
    return rc;
  int bin_counts_i[kMailboxMaxWorld], pad = 1;
  bool any_out = false;
  rc = shard_exchange_bin_lists(e, X, e->d_gt_bins.p, n_bins, out_of_range, counts,
                                "global tree: a bin count outside its slice arrived", bin_counts_i, &pad, &any_out);
  if (rc != BPF_OK)
    return rc;
  if (any_out)
  {
    // the keys route: the slices cross, every pose's key goes through the host tree in index order
    long long total = 0;
    for (int r = 0; r < W; ++r)
      total += counts[r];
    const int N = (int)total;
    std::vector<double> soa;
    rc = shard_gather_slices_host(e, X, counts, N, 3, &soa, &s);
    if (rc != BPF_OK)
      return rc;
    std::vector<int> keys((size_t)3 * (size_t)N);
    for (int i = 0; i < N; ++i)
      host_pose_key(soa[i], soa[(size_t)N + i], soa[2 * (size_t)N + i], &keys[3 * (size_t)i]);
    return tree_from_keys(e, keys.data(), N, leaf_out, bins_out);
  }
  return tree_merge(e, e->d_x_gather.p, bin_counts_i, W, pad, leaf_out, bins_out);
}

// The same for the set that is NOT current yet (n samples written into the spare set): the engine's own counts keep
// describing the current set, and the caller installs leaf / bins / route once the new set is current.
int shard_spare_tree(bpf_engine* e, ShardExchange& X, int n, long long first, const long long* counts, int* leaf_out,
                     int* bins_out, int* route_out)
{
  const TreeCounts before = e->tree;
  const int rc = shard_global_tree(e, X, e->sets[e->cur ^ 1], n, first, counts, leaf_out, bins_out);
  *route_out = e->tree.gt_route;
  e->tree = before;
  return rc;
}

// write this rank's even share into the spare set, find the global tree, and only then make the set current
int shard_init_all(bpf_engine* e, bool spread, const std::function<int(long long, int, long long, uint64_t*)>& write)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  const int W = e->shard_world, rank = e->shard_rank;
  const long long G = e->max_samples;
  long long counts[kMailboxMaxWorld] = { 0 };
  for (int r = 0; r < W; ++r)
    counts[r] = (G * (r + 1)) / W - (G * r) / W;
  const long long first = (G * rank) / W;
  const int n = (int)counts[rank];
  uint64_t rng_after = 0;
  rc = write(first, n, G, &rng_after);
  if (rc != BPF_OK)
    return rc;
  int leaf = 0, bins = 0, route = 0;
  rc = shard_spare_tree(e, X, n, first, counts, &leaf, &bins, &route);
  if (rc != BPF_OK)
    return rc;
  rc = shard_init_commit(e, n, rng_after, spread);
  if (rc != BPF_OK)
    return rc;
  tree_install(e, leaf, bins, route);
  e->slice_first = first;
  e->slice_global = G;
  return BPF_OK;
}
}  // namespace

int bpf_shard_init_with_gaussian_all(bpf_engine* e, const double mean[3], const double rotation[9],
                                     const double sigma[3])
{
  if (!e || !mean || !rotation || !sigma)
    return BPF_ERR_INVALID_ARGUMENT;
  return shard_init_all(e, false, [&](long long first, int n, long long G, uint64_t* rng_after) {
    return shard_init_gaussian_write(e, mean, rotation, sigma, first, n, G, rng_after);
  });
}

int bpf_shard_init_with_mixture_all(bpf_engine* e, const bpf_mixture_component* comps, int n_components)
{
  if (!e || !comps)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  // the table's refusals come first on purpose (every rank holds the same table, so every rank refuses alike, and
  // before anything is exchanged); they need max_samples, hence the filter check here as well as in shard_init_all
  MixtureTable T;
  const int rc = mixture_table(e, comps, n_components, e->max_samples, &T);
  if (rc != BPF_OK)
    return rc;
  return shard_init_all(e, T.spread, [&](long long first, int n, long long G, uint64_t* rng_after) {
    return shard_init_mixture_write(e, T, first, n, G, rng_after);
  });
}

int bpf_shard_init_with_random_poses_all(bpf_engine* e)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  return shard_init_all(e, true, [&](long long first, int n, long long G, uint64_t* rng_after) {
    return shard_init_random_write(e, first, n, G, rng_after);
  });
}

int bpf_shard_global_leaf_count(bpf_engine* e, int* leaf_count_out, int* bin_count_out)
{
  if (!e || !leaf_count_out || !bin_count_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  if (!e->tree.tree_pending && e->tree.leaf_count > 0)
  {
    // of the global set (an init, this call or a resample installed it): no exchange
    *leaf_count_out = e->tree.leaf_count;
    *bin_count_out = e->tree.bin_count;
    return BPF_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  long long counts[kMailboxMaxWorld] = { 0 }, total = 0, first = 0;
  rc = shard_gather_counts(e, X, "global tree", counts, &first, &total);
  if (rc != BPF_OK)
    return rc;
  if (total <= 0 || total > (long long)e->max_samples)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "global tree: the global set is empty, or beyond max_samples");
  return shard_global_tree(e, X, e->sets[e->cur], e->sample_count, first, counts, leaf_count_out, bin_count_out);
}

int bpf_shard_exchange_count(bpf_engine* e, long long* out)
{
  if (!e || !out)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  *out = e->mb.active ? (long long)(e->mb.tot_gen + e->mb.win_gen - e->mb.gen_base) : (long long)e->coll.exchanges;
  return BPF_OK;
}
