// C-ABI: a sharded set initialised on its ranks, and the histogram tree of the GLOBAL set from the ranks' bin lists
// (kernels_shard_init.hpp).  Stage functions: no call here waits for another rank; the one-call forms that do their
// own exchanges are in abi_shard_node.inl.
// ---------------------------------------------------------------------- sharded init
namespace
{
int shard_init_check(bpf_engine* e, long long global_first, int local_count, long long global_count)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  if (global_count != (long long)e->max_samples)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "sharded init: global_count must be the engine's max_samples");
  if (global_first < 0 || local_count < 0 || global_first + local_count > global_count)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "sharded init: shard range outside the global set");
  return BPF_OK;
}

// ParticleFilter::initWithGaussian for samples [first, first + n) into the set that is NOT current; nothing of the
// engine's filter state changes.  *rng_after = the stream state after the WHOLE set's draws.
int shard_init_gaussian_write(bpf_engine* e, const double mean[3], const double rotation[9], const double sigma[3],
                              long long first, int n, long long global_count, uint64_t* rng_after)
{
  HIPCHK(e, e->d_init_rot.reserve(9));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_init_rot.p, rotation, 9 * sizeof(double)));  // the caller's memory
  SampleSet& dst = e->sets[e->cur ^ 1];
  long long consumed = 0;
  int rc = generate_gaussians(e, 3 * global_count, 3 * first, 3ll * n, sigma, &consumed, [&]() {
    if (n > 0)
      hipLaunchKernelGGL(k_init_gaussian, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, dst.dev(), n,
                         (const double*)e->d_gauss.p, mean[0], mean[1], mean[2], (const double*)e->d_init_rot.p,
                         1.0 / (double)global_count);
  });
  if (rc != BPF_OK)
    return rc;
  *rng_after = lcg_skip_host(e->rng, (uint64_t)consumed, e->jump);
  return BPF_OK;
}

// the mixture initialiser (bpf_pf_init_with_mixture), as above; the table's counts are those of the GLOBAL set
int shard_init_mixture_write(bpf_engine* e, const MixtureTable& T, long long first, int n, long long global_count,
                             uint64_t* rng_after)
{
  MixtureDev X{};
  int rc = mixture_upload(e, T, &X);
  if (rc != BPF_OK)
    return rc;
  SampleSet& dst = e->sets[e->cur ^ 1];
  long long consumed = 0;
  rc = generate_gaussians(
      e, 3 * global_count, 3 * first, 3ll * n, nullptr, &consumed,
      [&]() {
        if (n > 0)
          hipLaunchKernelGGL(k_init_mixture, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, dst.dev(), n,
                             (int)first, (const double*)e->d_gauss.p, X, 1.0 / (double)global_count);
      },
      &X);
  if (rc != BPF_OK)
    return rc;
  *rng_after = lcg_skip_host(e->rng, (uint64_t)consumed, e->jump);
  return BPF_OK;
}

// ParticleFilter::initWithPoseFn with Node::uniformPoseGenerator, as above
int shard_init_random_write(bpf_engine* e, long long first, int n, long long global_count, uint64_t* rng_after)
{
  if (e->pose_check_scoring == BPF_POSE_CHECK_SENSOR_MODEL)
    return e->fail(BPF_ERR_UNSUPPORTED, "BPF_POSE_CHECK_SENSOR_MODEL is not available on the sharded path");
  FreeSpaceDev fs{};
  int rc = ensure_free_space(e, &fs);
  if (rc != BPF_OK)
    return rc;
  // global_count back-to-back calls from element 1, 2 (retries + 1) elements each: the GLOBAL stream use
  const uint64_t consumed = (2ull * (uint64_t)fs.retries + 2ull) * (uint64_t)global_count;
  if (consumed >= 0x7fffffffull)
    return e->fail(BPF_ERR_CAPACITY, "random pose calls would pass 31-bit stream positions");
  if (n > 0)
  {
    hipLaunchKernelGGL(k_init_free_space_range, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream,
                       e->sets[e->cur ^ 1].dev(), n, first, e->rng, e->jump, fs, 1.0 / (double)global_count);
    HIPCHK(e, hipGetLastError());
  }
  *rng_after = lcg_skip_host(e->rng, consumed, e->jump);
  return BPF_OK;
}

// the written set becomes the current one: what finish_init leaves, except the tree (the tree of the GLOBAL set comes
// from the bin lists: bpf_shard_tree_*)
int shard_init_commit(bpf_engine* e, int n, uint64_t rng_after, bool spread)
{
  e->rng = rng_after;
  e->wc.shard_cdf_dropped();
  e->mb_totals_valid = false;
  return e->fresh_filter(n, true, TreeCounts{ -1, -1, 0, false }, spread);
}

int gtree_flags(bpf_engine* e)
{
  HIPCHK(e, e->h_gt_flags.reserve(4));
  H2D_OR_RETURN(pinned_down_sync(e, e->h_gt_flags, 0, e->d_gt_flags, 0, 4, e->stream));
  if (e->h_gt_flags.p[3] != 0)
    return e->fail(BPF_ERR_HIP, "global tree: a bounded table walk ran out (corrupt bin list?)");
  return BPF_OK;
}

// The distinct packed keys of `n` samples of set `s` with the global index of each key's first sample, in first-index
// order: d_gt_bins = int64[2][*n_bins_out].  The statistics stages' state is not touched (the scratch tables of the
// resampler's tree are, as by every tree build).
int tree_local_bins(bpf_engine* e, SampleSet& s, int n, long long global_first, int* n_bins_out, int* out_of_range_out)
{
  if (global_first + n >= (1ll << 30))
    return e->fail(BPF_ERR_CAPACITY, "global tree: global sample index beyond 2^30");
  HIPCHK(e, e->d_gt_bins.reserve((size_t)2 * std::max(n, 1)));
  HIPCHK(e, e->d_gt_flags.reserve(4));
  *n_bins_out = 0;
  *out_of_range_out = 0;
  if (n == 0)
    return BPF_OK;
  HIPCHK(e, hipMemsetAsync(e->d_gt_flags.p, 0, 4 * sizeof(int), e->stream));
  const unsigned table = hash_table_size(n);
  const int tiles = blocks_for(n, kStatTile);
  HIPCHK(e, e->d_keys.reserve((size_t)n * 3));
  HIPCHK(e, e->d_kld_hkey.reserve(table));
  HIPCHK(e, e->d_kld_htmin.reserve(table));
  HIPCHK(e, e->d_kld_slot.reserve((size_t)n));
  HIPCHK(e, e->d_gt_tiles.reserve((size_t)tiles));
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
  K.flags = e->d_gt_flags.p;
  hipLaunchKernelGGL(k_kld_hash, grid, block, 0, e->stream, K);
  ShardBinsArgs A{};
  A.p = s.dev();
  A.n = n;
  A.global_first = global_first;
  A.h_key = e->d_kld_hkey.p;
  A.h_tmin = e->d_kld_htmin.p;
  A.slot = e->d_kld_slot.p;
  A.flags = e->d_gt_flags.p;
  A.tile_sums = e->d_gt_tiles.p;
  A.bins = e->d_gt_bins.p;
  hipLaunchKernelGGL(k_sstat_first_count, dim3(tiles), block, 0, e->stream, A);
  hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_gt_tiles.p, tiles, e->d_gt_flags.p);
  hipLaunchKernelGGL(k_sstat_compact, dim3(tiles), block, 0, e->stream, A);
  HIPCHK(e, hipGetLastError());
  int rc = gtree_flags(e);
  if (rc != BPF_OK)
    return rc;
  *n_bins_out = e->h_gt_flags.p[2];
  *out_of_range_out = e->h_gt_flags.p[0] != 0 ? 1 : 0;  // ([1], a non-finite statistics term, is of no concern here)
  if (*n_bins_out < 0 || *n_bins_out > n)
    return e->fail(BPF_ERR_HIP, "global tree: bin count outside the slice (internal error)");
  return BPF_OK;
}

// leaf / bin counts of the global set where bpf_shard_adopt_dev installs them
void tree_install(bpf_engine* e, int leaf, int bins, int route)
{
  e->tree_installed(kld_bins(e) ? bins : leaf, bins, route);
}

// What the two merges of gathered bin lists share (tree_merge, and mn_merge_stop of abi_shard_inplace_mn.inl): the
// checked lists, the cleared table of the merged keys and the cleared flags on the stream, and *G filled but for
// tile_sums, which is the caller's (G->cap: the lists' total)
int gtree_merge_begin(bpf_engine* e, const long long* all, const int* counts, int world, int pad, const char* prefix,
                      GlobalTreeArgs* G)
{
  long long total_bins = 0;
  unsigned table = 0;
  int rc = bin_lists_check(e, counts, world, pad, e->max_samples, prefix, &total_bins, &table);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, e->d_gt_key.reserve(table));
  HIPCHK(e, e->d_gt_tmin.reserve(table));
  HIPCHK(e, e->d_gt_eslot.reserve((size_t)world * (size_t)pad));
  HIPCHK(e, e->d_gt_flags.reserve(4));
  HIPCHK(e, e->d_keys.reserve((size_t)total_bins * 3));
  // d_keys is about to hold the merged keys: statistics stages in progress would read it as the slice's keys, so
  // they start over (their own check then says so instead of summing into the wrong bins)
  e->ss_stage = 0;
  HIPCHK(e, hipMemsetAsync(e->d_gt_key.p, 0xFF, (size_t)table * sizeof(unsigned long long), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_gt_tmin.p, 0x7F, (size_t)table * sizeof(int), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_gt_flags.p, 0, 4 * sizeof(int), e->stream));
  *G = GlobalTreeArgs{};
  G->all = all;
  G->world = world;
  G->pad = pad;
  for (int r = 0; r < world; ++r)
    G->counts[r] = counts[r];
  G->g_key = e->d_gt_key.p;
  G->g_tmin = e->d_gt_tmin.p;
  G->g_mask = table - 1;
  G->eslot = e->d_gt_eslot.p;
  G->flags = e->d_gt_flags.p;
  G->keys_out = e->d_keys.p;
  G->cap = (int)total_bins;
  return BPF_OK;
}

// the merge stage and the tree on the merged keys
int tree_merge(bpf_engine* e, const long long* all, const int* counts, int world, int pad, int* leaf_out, int* bins_out)
{
  GlobalTreeArgs G;
  int rc = gtree_merge_begin(e, all, counts, world, pad, "global tree", &G);
  if (rc != BPF_OK)
    return rc;
  const int flat = world * pad, tiles = blocks_for(flat, kStatTile);
  HIPCHK(e, e->d_gt_tiles.reserve((size_t)tiles));
  G.tile_sums = e->d_gt_tiles.p;
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_gtree_insert, dim3(blocks_for(flat, 256)), dim3(256), 0, e->stream, G);
    hipLaunchKernelGGL(k_gtree_first_count, dim3(tiles), dim3(256), 0, e->stream, G);
    hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_gt_tiles.p, tiles,
                       e->d_gt_flags.p);
    hipLaunchKernelGGL(k_gtree_compact, dim3(tiles), dim3(256), 0, e->stream, G);
    HIPCHK(e, hipGetLastError());
  }
  rc = gtree_flags(e);
  if (rc != BPF_OK)
    return rc;
  const int n_distinct = e->h_gt_flags.p[2];
  if (n_distinct <= 0 || n_distinct > G.cap)
    return e->fail(BPF_ERR_HIP, "global tree: distinct key count outside the lists (internal error)");
  int leaf = n_distinct, route = BPF_SHARD_TREE_ROUTE_BIN_COUNT;
  if (!kld_bins(e))
  {
    KldOutcome dev;
    if (n_distinct >= 8192)
    {
      H2D_OR_RETURN(kld_tree_on_device(e, n_distinct, &dev, true));
      if (dev.handled && dev.bins != n_distinct)
        return e->fail(BPF_ERR_HIP, "global tree: the device tree saw repeated keys (internal error)");
      leaf = dev.leaf;
      route = BPF_SHARD_TREE_ROUTE_DEVICE;
    }
    if (!dev.handled)
    {
      std::vector<int> keys((size_t)n_distinct * 3);
      H2D_OR_RETURN(d2h_to_host(e, keys.data(), e->d_keys.p, keys.size() * sizeof(int), e->stream));
      e->hist.clear();
      for (int i = 0; i < n_distinct; ++i)
        e->hist.insert(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2]);
      leaf = e->hist.leaf_count();
      route = BPF_SHARD_TREE_ROUTE_HOST;
    }
  }
  tree_install(e, leaf, n_distinct, route);
  *leaf_out = e->tree.leaf_count;
  *bins_out = e->tree.bin_count;
  return BPF_OK;
}

// the keys route: every raw key of the global set, in index order, through the host tree
int tree_from_keys(bpf_engine* e, const int* keys, int n, int* leaf_out, int* bins_out)
{
  kld_host_reset(e, std::min(std::max(n, 1024), 1 << 20));
  for (int i = 0; i < n; ++i)
    kld_host_insert(e, keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2]);
  tree_install(e, kld_host_k(e), kld_bins(e) ? e->kld_host_bins : e->hist.bin_count(), BPF_SHARD_TREE_ROUTE_KEYS);
  *leaf_out = e->tree.leaf_count;
  *bins_out = e->tree.bin_count;
  return BPF_OK;
}
}  // namespace

int bpf_shard_init_with_gaussian(bpf_engine* e, const double mean[3], const double rotation[9], const double sigma[3],
                                 long long global_first, int local_count, long long global_count)
{
  if (!e || !mean || !rotation || !sigma)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_init_check(e, global_first, local_count, global_count);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t rng_after = 0;
  rc = shard_init_gaussian_write(e, mean, rotation, sigma, global_first, local_count, global_count, &rng_after);
  if (rc != BPF_OK)
    return rc;
  rc = shard_init_commit(e, local_count, rng_after, false);
  e->slice_first = rc == BPF_OK ? global_first : -1;
  e->slice_global = global_count;
  return rc;
}

int bpf_shard_init_with_mixture(bpf_engine* e, const bpf_mixture_component* comps, int n_components,
                                long long global_first, int local_count, long long global_count)
{
  if (!e || !comps)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_init_check(e, global_first, local_count, global_count);
  if (rc != BPF_OK)
    return rc;
  MixtureTable T;
  rc = mixture_table(e, comps, n_components, global_count, &T);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t rng_after = 0;
  rc = shard_init_mixture_write(e, T, global_first, local_count, global_count, &rng_after);
  if (rc != BPF_OK)
    return rc;
  rc = shard_init_commit(e, local_count, rng_after, T.spread);
  e->slice_first = rc == BPF_OK ? global_first : -1;
  e->slice_global = global_count;
  return rc;
}

int bpf_shard_init_with_random_poses(bpf_engine* e, long long global_first, int local_count, long long global_count)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  int rc = shard_init_check(e, global_first, local_count, global_count);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t rng_after = 0;
  rc = shard_init_random_write(e, global_first, local_count, global_count, &rng_after);
  if (rc != BPF_OK)
    return rc;
  rc = shard_init_commit(e, local_count, rng_after, true);  // uniform over the free space: scored in tile order
  e->slice_first = rc == BPF_OK ? global_first : -1;
  e->slice_global = global_count;
  return rc;
}

int bpf_shard_tree_local_bins_dev(bpf_engine* e, long long global_first, void** bins_dev, int* n_bins_out,
                                  int* out_of_range_out)
{
  if (!e || !bins_dev || !n_bins_out || !out_of_range_out || global_first < 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  HIPCHK(e, hipSetDevice(e->device));
  int rc = tree_local_bins(e, e->sets[e->cur], e->sample_count, global_first, n_bins_out, out_of_range_out);
  *bins_dev = e->d_gt_bins.p;
  return rc;
}

int bpf_shard_tree_merge_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                             int* leaf_count_out, int* bin_count_out)
{
  if (!e || !all_bins_dev || !counts || !leaf_count_out || !bin_count_out || world <= 0 ||
      world > kShardStatsMaxWorld || pad <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  HIPCHK(e, hipSetDevice(e->device));
  return tree_merge(e, static_cast<const long long*>(all_bins_dev), counts, world, pad, leaf_count_out, bin_count_out);
}

int bpf_shard_tree_local_keys_dev(bpf_engine* e, void** keys_dev, int* n_keys_out)
{
  if (!e || !keys_dev || !n_keys_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  HIPCHK(e, hipSetDevice(e->device));
  const int n = e->sample_count;
  HIPCHK(e, e->d_keys.reserve((size_t)std::max(n, 1) * 3));
  if (n > 0)
  {
    hipLaunchKernelGGL(k_set_keys, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->sets[e->cur].dev(), n,
                       e->d_keys.p);
    HIPCHK(e, hipGetLastError());
  }
  *keys_dev = e->d_keys.p;
  *n_keys_out = n;
  return BPF_OK;
}

int bpf_shard_tree_from_keys(bpf_engine* e, const int* all_keys, int global_count, int* leaf_count_out,
                             int* bin_count_out)
{
  if (!e || !all_keys || global_count <= 0 || !leaf_count_out || !bin_count_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  return tree_from_keys(e, all_keys, global_count, leaf_count_out, bin_count_out);
}

int bpf_shard_tree_last_route(bpf_engine* e, int* route_out)
{
  if (!e || !route_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *route_out = e->tree.gt_route;
  return BPF_OK;
}
