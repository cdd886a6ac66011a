// C-ABI: cluster statistics of a sharded set (kernels_shard_stats.hpp).
// ---------------------------------------------------------------------- sharded cluster statistics
namespace
{
// the small result of the finishing kernels -> the engine, where the single path puts it
void install_device_stats(bpf_engine* e, const StatsResult& r)
{
  e->stats_cluster_count = r.cluster_count;
  e->stats_best = r.best;
  e->stats_best_weight = r.best_weight;
  std::memcpy(e->stats_best_pose, r.best_pose, sizeof(r.best_pose));
  std::memcpy(e->set_mean, r.set_mean, sizeof(r.set_mean));
  std::memcpy(e->set_cov, r.set_cov, sizeof(r.set_cov));
  e->clusters.clear();
  e->stats_clusters_fetched = false;
  e->stats_on_device = true;
  e->stats_own_set = false;  // the GLOBAL set's: no host evaluation of this rank's slice may stand in for them
  e->stats_epoch = e->set_epoch;
}

int shard_stats_flags(bpf_engine* e)
{
  HIPCHK(e, e->h_stats_flags.reserve(4));
  H2D_OR_RETURN(pinned_down_sync(e, e->h_stats_flags, 0, e->d_stats_flags, 0, 4, e->stream));
  if (e->h_stats_flags.p[3] != 0)
    return e->fail(BPF_ERR_HIP, "sharded statistics: a bounded table walk ran out (corrupt bin list?)");
  return BPF_OK;
}

// The gathered bin lists of a merge stage (statistics labels, the global tree, the multinomial stop): every count within
// [0, pad], a total of 1 .. max_total (0: no bound of its own), and world * pad -- the kernels' flat index -- below
// 2^30.  *table_out: the size of the merged keys' hash table.
int bin_lists_check(bpf_engine* e, const int* counts, int world, int pad, long long max_total, const std::string& prefix,
                    long long* total_out, unsigned* table_out)
{
  long long total_bins = 0;
  for (int r = 0; r < world; ++r)
  {
    if (counts[r] < 0 || counts[r] > pad)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, prefix + ": a bin count outside [0, pad]");
    total_bins += counts[r];
  }
  if (total_bins <= 0 || (long long)world * pad >= (1ll << 30) || (max_total > 0 && total_bins > max_total))
    return e->fail(BPF_ERR_INVALID_ARGUMENT,
                   prefix + (max_total > 0 ? ": no bins, or more than max_samples" : ": no bins, or too many"));
  *total_out = total_bins;
  *table_out = hash_table_size(total_bins);
  return BPF_OK;
}
}  // namespace

int bpf_shard_samples_dev(bpf_engine* e, void** x_dev, void** y_dev, void** theta_dev, void** w_dev, int* count_out)
{
  if (!e || !x_dev || !y_dev || !theta_dev || !w_dev || !count_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  SampleSet& s = e->sets[e->cur];
  *x_dev = s.x.p;
  *y_dev = s.y.p;
  *theta_dev = s.th.p;
  *w_dev = s.w.p;
  *count_out = e->sample_count;
  return BPF_OK;
}

int bpf_shard_stats_gathered_dev(bpf_engine* e, const void* x_all, const void* y_all, const void* theta_all,
                                 const void* w_all, int global_count, int* handled_out)
{
  if (!e || !x_all || !y_all || !theta_all || !handled_out || global_count <= 0 || global_count > kStatBlockMax)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  HIPCHK(e, hipSetDevice(e->device));
  *handled_out = BPF_SHARD_STATS_DECLINED;
  e->ss_stage = 0;
  if (e->stats_host)
  {
    *handled_out = BPF_SHARD_STATS_HOST_ROUTE;
    return BPF_OK;
  }
  ParticlesDev p{};
  p.x = const_cast<double*>(static_cast<const double*>(x_all));
  p.y = const_cast<double*>(static_cast<const double*>(y_all));
  p.th = const_cast<double*>(static_cast<const double*>(theta_all));
  p.w = const_cast<double*>(static_cast<const double*>(w_all));
  if (!w_all)
  {
    // the weights straight after a resample (particle_filter.cpp:409,458-462)
    HIPCHK(e, e->d_ss_w.reserve((size_t)kStatBlockMax));
    hipLaunchKernelGGL(k_sstat_fill, dim3(blocks_for(global_count, 256)), dim3(256), 0, e->stream, e->d_ss_w.p,
                       global_count, 1.0 / (double)global_count);
    p.w = e->d_ss_w.p;
  }
  int status = 0;
  int rc = stats_block_evaluate(e, p, global_count, &status);
  if (rc != BPF_OK)
    return rc;
  *handled_out = status == 0 ? BPF_SHARD_STATS_INSTALLED
                             : (status >= 10 ? BPF_SHARD_STATS_HOST_ROUTE : BPF_SHARD_STATS_DECLINED);
  return BPF_OK;
}

int bpf_shard_stats_local_bins_dev(bpf_engine* e, long long global_first, void** bins_dev, int* n_bins_out,
                                   int* host_route_out)
{
  if (!e || !bins_dev || !n_bins_out || !host_route_out || global_first < 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  const int n = e->sample_count;
  if (global_first + n >= (1ll << 30))
    return e->fail(BPF_ERR_CAPACITY, "sharded statistics: global sample index beyond 2^30");
  HIPCHK(e, hipSetDevice(e->device));
  e->ss_stage = 0;
  HIPCHK(e, e->d_ss_bins.reserve((size_t)2 * std::max(n, 1)));
  HIPCHK(e, e->d_stats_flags.reserve(4));
  *bins_dev = e->d_ss_bins.p;
  *n_bins_out = 0;
  *host_route_out = e->stats_host ? 1 : 0;
  HIPCHK(e, hipMemsetAsync(e->d_stats_flags.p, 0, 4 * sizeof(int), e->stream));
  if (n > 0)
  {
    SampleSet& s = e->sets[e->cur];
    const unsigned table = hash_table_size(n);
    const int tiles = blocks_for(n, kStatTile);
    HIPCHK(e, e->d_keys.reserve((size_t)n * 3));
    HIPCHK(e, e->d_kld_hkey.reserve(table));
    HIPCHK(e, e->d_kld_htmin.reserve(table));
    HIPCHK(e, e->d_kld_slot.reserve((size_t)n));
    HIPCHK(e, e->d_stats_tiles.reserve((size_t)tiles));
    e->kld_clean_table = 0;  // (the resampler's tables: in use here)
    HIPCHK(e, hipMemsetAsync(e->d_kld_hkey.p, 0xFF, (size_t)table * sizeof(unsigned long long), e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_kld_htmin.p, 0x7F, (size_t)table * sizeof(int), e->stream));
    const dim3 grid(blocks_for(n, 256)), block(256);
    hipLaunchKernelGGL(k_set_keys, grid, block, 0, e->stream, s.dev(), n, e->d_keys.p);
    KldArgs K{};
    K.keys = e->d_keys.p;
    K.n = n;
    K.h_key = e->d_kld_hkey.p;
    K.h_tmin = e->d_kld_htmin.p;
    K.h_mask = table - 1;
    K.slot = e->d_kld_slot.p;
    K.flags = e->d_stats_flags.p;
    hipLaunchKernelGGL(k_kld_hash, grid, block, 0, e->stream, K);
    ShardBinsArgs A{};
    A.p = s.dev();
    A.n = n;
    A.global_first = global_first;
    A.h_key = e->d_kld_hkey.p;
    A.h_tmin = e->d_kld_htmin.p;
    A.slot = e->d_kld_slot.p;
    A.flags = e->d_stats_flags.p;
    A.tile_sums = e->d_stats_tiles.p;
    A.bins = e->d_ss_bins.p;
    hipLaunchKernelGGL(k_sstat_first_count, dim3(tiles), block, 0, e->stream, A);
    hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_stats_tiles.p, tiles,
                       e->d_stats_flags.p);
    hipLaunchKernelGGL(k_sstat_compact, dim3(tiles), block, 0, e->stream, A);
    HIPCHK(e, hipGetLastError());
    int rc = shard_stats_flags(e);
    if (rc != BPF_OK)
      return rc;
    *n_bins_out = e->h_stats_flags.p[2];
    if (e->h_stats_flags.p[0] != 0 || e->h_stats_flags.p[1] != 0)
      *host_route_out = 1;
  }
  e->ss_stage = 1;
  e->ss_epoch = e->set_epoch;
  return BPF_OK;
}

int bpf_shard_stats_label_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                              int* cluster_count_out)
{
  if (!e || !all_bins_dev || !counts || !cluster_count_out || world <= 0 || world > kShardStatsMaxWorld || pad <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf || e->ss_stage < 1 || e->ss_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_shard_stats_local_bins_dev of the current set first");
  long long total_bins = 0;
  unsigned table = 0;
  int rc = bin_lists_check(e, counts, world, pad, 0, "sharded statistics", &total_bins, &table);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  e->ss_stage = 1;
  const int flat = world * pad, tiles = blocks_for(flat, kStatTile);
  HIPCHK(e, e->d_ss_gkey.reserve(table));
  HIPCHK(e, e->d_ss_gtmin.reserve(table));
  HIPCHK(e, e->d_ss_parent.reserve(table));
  HIPCHK(e, e->d_ss_label.reserve(table));
  HIPCHK(e, e->d_ss_binlabel.reserve(table));
  HIPCHK(e, e->d_ss_eslot.reserve((size_t)flat));
  HIPCHK(e, e->d_ss_eroot.reserve((size_t)flat));
  HIPCHK(e, e->d_stats_tiles.reserve((size_t)tiles));
  HIPCHK(e, hipMemsetAsync(e->d_ss_gkey.p, 0xFF, (size_t)table * sizeof(unsigned long long), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_ss_gtmin.p, 0x7F, (size_t)table * sizeof(int), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_ss_binlabel.p, 0xFF, (size_t)table * sizeof(int), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_stats_flags.p, 0, 4 * sizeof(int), e->stream));
  GlobalBinsArgs G{};
  G.all = static_cast<const long long*>(all_bins_dev);
  G.world = world;
  G.pad = pad;
  for (int r = 0; r < world; ++r)
    G.counts[r] = counts[r];
  G.g_key = e->d_ss_gkey.p;
  G.g_tmin = e->d_ss_gtmin.p;
  G.g_mask = table - 1;
  G.parent = e->d_ss_parent.p;
  G.eslot = e->d_ss_eslot.p;
  G.eroot = e->d_ss_eroot.p;
  G.label = e->d_ss_label.p;
  G.binlabel = e->d_ss_binlabel.p;
  G.flags = e->d_stats_flags.p;
  const dim3 grid(blocks_for(flat, 256)), block(256);
  hipLaunchKernelGGL(k_gstat_insert, grid, block, 0, e->stream, G);
  hipLaunchKernelGGL(k_gstat_init, dim3(blocks_for((int)table, 256)), block, 0, e->stream, G);
  hipLaunchKernelGGL(k_gstat_union, grid, block, 0, e->stream, G);
  hipLaunchKernelGGL(k_gstat_roots, dim3(tiles), block, 0, e->stream, G, e->d_stats_tiles.p);
  hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_stats_tiles.p, tiles,
                     e->d_stats_flags.p);
  hipLaunchKernelGGL(k_gstat_labels, dim3(tiles), block, 0, e->stream, G, (const int*)e->d_stats_tiles.p);
  hipLaunchKernelGGL(k_gstat_binlabel, grid, block, 0, e->stream, G);
  HIPCHK(e, hipGetLastError());
  rc = shard_stats_flags(e);
  if (rc != BPF_OK)
    return rc;
  e->ss_clusters = e->h_stats_flags.p[2];
  e->ss_gmask = table - 1;
  *cluster_count_out = e->ss_clusters;
  if (e->ss_clusters <= 0)
    return e->fail(BPF_ERR_HIP, "sharded statistics: no cluster found in a set with bins");
  e->ss_stage = 2;
  return BPF_OK;
}

int bpf_shard_stats_local_sums_dev(bpf_engine* e, void** sums_dev, size_t* n_words_out)
{
  if (!e || !sums_dev || !n_words_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf || e->ss_stage < 2 || e->ss_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_shard_stats_label_dev of the current set first");
  HIPCHK(e, hipSetDevice(e->device));
  const int n = e->sample_count, C = e->ss_clusters;
  const int n_sums = kStatTerms * C;
  HIPCHK(e, e->d_stats_hi.reserve((size_t)n_sums));
  HIPCHK(e, e->d_stats_lo.reserve((size_t)n_sums));
  HIPCHK(e, e->d_ss_limbs.reserve((size_t)kStatLimbs * n_sums));
  HIPCHK(e, hipMemsetAsync(e->d_stats_hi.p, 0, (size_t)n_sums * sizeof(long long), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_stats_lo.p, 0, (size_t)n_sums * sizeof(unsigned long long), e->stream));
  if (n > 0)
  {
    ShardSumsArgs A{};
    A.p = e->sets[e->cur].dev();
    A.n = n;
    A.keys = e->d_keys.p;
    A.g_key = e->d_ss_gkey.p;
    A.g_mask = e->ss_gmask;
    A.binlabel = e->d_ss_binlabel.p;
    A.clusters = C;
    A.acc_hi = e->d_stats_hi.p;
    A.acc_lo = e->d_stats_lo.p;
    A.flags = e->d_stats_flags.p;
    hipLaunchKernelGGL(k_sstat_accumulate, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, A);
  }
  hipLaunchKernelGGL(k_sstat_export, dim3(blocks_for(n_sums, 256)), dim3(256), 0, e->stream,
                     (const long long*)e->d_stats_hi.p, (const unsigned long long*)e->d_stats_lo.p, n_sums,
                     e->d_ss_limbs.p, (const int*)e->d_stats_flags.p);
  HIPCHK(e, hipGetLastError());
  *sums_dev = e->d_ss_limbs.p;
  *n_words_out = (size_t)kStatLimbs * n_sums;
  e->ss_stage = 3;
  return BPF_OK;
}

int bpf_shard_stats_finish_dev(bpf_engine* e, const void* reduced_sums_dev)
{
  if (!e || !reduced_sums_dev)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf || e->ss_stage < 3 || e->ss_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_shard_stats_local_sums_dev of the current set first");
  HIPCHK(e, hipSetDevice(e->device));
  const int C = e->ss_clusters;
  const int n_sums = kStatTerms * C;
  HIPCHK(e, e->d_stats_clusters.reserve((size_t)C));
  HIPCHK(e, e->d_stats_result.reserve(1));
  HIPCHK(e, e->h_stats_result.reserve(1));
  hipLaunchKernelGGL(k_sstat_import, dim3(blocks_for(n_sums, 256)), dim3(256), 0, e->stream,
                     static_cast<const long long*>(reduced_sums_dev), n_sums, e->d_stats_hi.p, e->d_stats_lo.p,
                     e->d_stats_flags.p, C);
  // the single engine's own finishing kernels on the reduced sums (the accumulators' stride is the cluster count)
  StatsArgs A{};
  A.n = C;
  A.flags = e->d_stats_flags.p;
  A.acc_hi = e->d_stats_hi.p;
  A.acc_lo = e->d_stats_lo.p;
  ClusterDev* clusters = reinterpret_cast<ClusterDev*>(e->d_stats_clusters.p);
  hipLaunchKernelGGL(k_stats_clusters, dim3(blocks_for(C, 256)), dim3(256), 0, e->stream, A, clusters);
  hipLaunchKernelGGL(k_stats_set, dim3(1), dim3(1024), 0, e->stream, A, (const ClusterDev*)clusters,
                     e->d_stats_result.p);
  HIPCHK(e, hipGetLastError());
  H2D_OR_RETURN(pinned_down(e, e->h_stats_result, 0, e->d_stats_result, 0, 1, e->stream));
  int rc = shard_stats_flags(e);
  e->ss_stage = 0;
  e->ss_finish_installed = false;
  if (rc != BPF_OK)
    return rc;
  if (e->h_stats_flags.p[1] != 0)
    return BPF_OK;  // a sum beyond the fixed-point format, on every rank alike (kernels_shard_stats.hpp): the host route
  install_device_stats(e, *e->h_stats_result.p);
  e->ss_finish_installed = true;
  return BPF_OK;
}

int bpf_shard_stats_finish_installed(bpf_engine* e, int* installed_out)
{
  if (!e || !installed_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *installed_out = e->ss_finish_installed ? 1 : 0;
  return BPF_OK;
}

int bpf_shard_stats_host(bpf_engine* e, const double* all_samples, int global_count)
{
  if (!e || !all_samples || global_count <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  // the histogram of the WHOLE set, every pose inserted in index order (as initWith* / the resamplers build it); the
  // engine's own histogram describes its slice and is left alone
  KdHistogram hist;
  for (int i = 0; i < global_count; ++i)
  {
    int key[3];
    host_pose_key(all_samples[4 * (size_t)i], all_samples[4 * (size_t)i + 1], all_samples[4 * (size_t)i + 2], key);
    hist.insert(key[0], key[1], key[2]);
  }
  e->ss_stage = 0;
  e->stats_on_device = false;
  int rc = host_cluster_stats(e, all_samples, global_count, hist, std::max(global_count, e->max_samples));
  if (rc == BPF_OK)
    e->stats_epoch = e->set_epoch;
  return rc;
}
