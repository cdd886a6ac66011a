// C-ABI: the multinomial resample of a sharded set in place (kernels_shard_inplace_mn.hpp).  Stage functions for a host
// with a transport of its own -- no call here waits for another rank -- and the one-call form that
// bpf_shard_update_resample takes over the engine's exchange when bpf_shard_set_multinomial_form says so.
// ---------------------------------------------------------------------- in-place multinomial resample
namespace
{
int mn_check_begin(bpf_engine* e, uint64_t rng_state48, const void* sums_dev, int rank, int world, void* flags_dev)
{
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  if (!sums_dev || !flags_dev || world < 1 || rank < 0 || rank >= world || world > kMailboxMaxWorld)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "bad in-place resample arguments");
  if (e->resample_model != BPF_RESAMPLE_MULTINOMIAL)
    return e->fail(BPF_ERR_INVALID_ARGUMENT,
                   "in-place multinomial resample: the systematic resampler has bpf_shard_inplace_select_dev");
  if ((rng_state48 & ((1ull << 48) - 1)) != e->shard_rng0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample does not belong to the resample begun");
  return BPF_OK;
}

// what the draws of this resample read from the stream (draw_window_args' branches, without a window)
int mn_draw_args(bpf_engine* e, int rank, int world, WindowArgs* out)
{
  WindowArgs& A = *out;
  A = WindowArgs{};
  A.src = e->sets[e->cur].dev();
  A.n_src = e->sample_count;
  A.cdf = e->d_cdf.p;
  A.rank = rank;
  A.world = world;
  A.m0 = 0;
  A.m1 = e->max_samples;
  A.rng_state = e->shard_rng0;
  A.jump = e->jump;
  if (e->shard_chain)
  {
    A.chain = e->d_chain.p;
    A.write_random = rank == 0;
    int rcf = ensure_free_space(e, &A.free_space);
    if (rcf != BPF_OK)
      return rcf;
  }
  else
  {
    int rcj = ensure_fused_jump(e);
    if (rcj != BPF_OK)
      return rcj;
    A.jump_table = e->d_fused_jump.p;
    A.jump_table_n = kFusedWindow;
  }
  return BPF_OK;
}

int mn_buffers(bpf_engine* e)
{
  const size_t maxs = (size_t)e->max_samples;
  HIPCHK(e, e->d_mn_idx.reserve(maxs));
  HIPCHK(e, e->d_mn_mark.reserve(maxs));
  HIPCHK(e, e->d_mn_tiles.reserve((size_t)blocks_for(e->max_samples, kMnTile)));
  HIPCHK(e, e->d_mn_words.reserve(8 + kMailboxMaxWorld + 1));
  HIPCHK(e, e->d_gt_flags.reserve(4));
  return BPF_OK;
}

// this rank's candidates, in draw order, into the set that is NOT current; nothing of the engine's filter state changes
int mn_select(bpf_engine* e, int rank, int world, const double* edge, int* n_kept_out)
{
  if (e->sample_count > 0 && !e->d_cdf.p)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_build_cdf first");
  int rc = mn_buffers(e);
  if (rc != BPF_OK)
    return rc;
  const int maxs = e->max_samples, tiles = blocks_for(maxs, kMnTile);
  MnSelectArgs A{};
  rc = mn_draw_args(e, rank, world, &A.W);
  if (rc != BPF_OK)
    return rc;
  size_t lds = 0;
  if (e->wc.cdf_coarse_n == A.W.n_src && A.W.n_src > 0)
  {
    A.W.coarse = e->d_cdf_coarse.p;
    A.W.coarse_shift = fused_coarse_shift(A.W.n_src);
    lds = ((size_t)((A.W.n_src - 1) >> A.W.coarse_shift) + 2) * sizeof(double);
  }
  A.offset = edge[rank];
  A.top = edge[rank + 1];
  A.dst = e->sets[e->cur ^ 1].dev();
  A.draw_idx = e->d_mn_idx.p;
  A.tile_sums = e->d_mn_tiles.p;
  A.W.flags = e->d_mn_words.p + 8 + kMailboxMaxWorld;  // draw_window_column's flag: a word nobody reads
  A.first_miss = e->d_mn_words.p;
  HIPCHK(e, hipMemsetAsync(e->d_mn_words.p, 0x7F, sizeof(int), e->stream));  // no miss: beyond every draw index
  HIPCHK(e, hipMemsetAsync(e->d_gt_flags.p, 0, 4 * sizeof(int), e->stream));
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_mn_select_count, dim3(tiles), dim3(kMnTile), lds, e->stream, A);
    hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_mn_tiles.p, tiles, e->d_gt_flags.p);
    hipLaunchKernelGGL(k_mn_select_scatter, dim3(tiles), dim3(kMnTile), lds, e->stream, A);
  }
  HIPCHK(e, hipGetLastError());
  rc = gtree_flags(e);
  if (rc != BPF_OK)
    return rc;
  const int n_kept = e->h_gt_flags.p[2];
  if (n_kept < 0 || n_kept > maxs)
    return e->fail(BPF_ERR_HIP, "in-place resample: kept count outside the candidates (internal error)");
  *n_kept_out = n_kept;
  return BPF_OK;
}

// the kept candidates' distinct keys with each key's smallest draw index: d_gt_bins = int64[2][*n_bins_out]
int mn_bins(bpf_engine* e, int n_kept, int* n_bins_out, int* out_of_range_out)
{
  int rc = tree_local_bins(e, e->sets[e->cur ^ 1], n_kept, 0, n_bins_out, out_of_range_out);
  if (rc != BPF_OK || *n_bins_out == 0)
    return rc;
  hipLaunchKernelGGL(k_mn_remap_bins, dim3(blocks_for(*n_bins_out, 256)), dim3(256), 0, e->stream,
                     e->d_gt_bins.p + *n_bins_out, *n_bins_out, (const int*)e->d_mn_idx.p, n_kept);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// The merged lists in first-draw order (d_keys, d_mn_t) and the stop rule on them:
//   c_j = max(t_j + 1, limit(L_j) + 1), M = the smallest c_j <= t_{j+1} with t_B = max_samples, else max_samples.
// The first branch is the draw that adds key j itself; it decides where the leaf count falls with a new key.
int mn_merge_stop(bpf_engine* e, const long long* all, const int* counts, int world, int pad, int* M_out, int* leaf_out,
                  int* bins_out, int* route_out)
{
  const int maxs = e->max_samples;
  GlobalTreeArgs G;
  int rc = gtree_merge_begin(e, all, counts, world, pad, "in-place resample", &G);
  if (rc == BPF_OK)
    rc = mn_buffers(e);
  if (rc != BPF_OK)
    return rc;
  const int flat = world * pad, tiles = blocks_for(maxs, kMnTile);
  HIPCHK(e, e->d_mn_t.reserve((size_t)G.cap));
  HIPCHK(e, hipMemsetAsync(e->d_mn_mark.p, 0, (size_t)maxs * sizeof(int), e->stream));
  G.tile_sums = e->d_mn_tiles.p;
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_gtree_insert, dim3(blocks_for(flat, 256)), dim3(256), 0, e->stream, G);
    hipLaunchKernelGGL(k_mn_mark, dim3(blocks_for(flat, 256)), dim3(256), 0, e->stream, G, e->d_mn_mark.p, maxs);
    hipLaunchKernelGGL(k_mn_mark_count, dim3(tiles), dim3(kMnTile), 0, e->stream, (const int*)e->d_mn_mark.p, maxs,
                       e->d_mn_tiles.p);
    hipLaunchKernelGGL(k_stats_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_mn_tiles.p, tiles, e->d_gt_flags.p);
    hipLaunchKernelGGL(k_mn_mark_compact, dim3(tiles), dim3(kMnTile), 0, e->stream, G, (const int*)e->d_mn_mark.p, maxs,
                       (const int*)e->d_mn_tiles.p, e->d_mn_t.p);
    HIPCHK(e, hipGetLastError());
  }
  rc = gtree_flags(e);
  if (rc != BPF_OK)
    return rc;
  const int B = e->h_gt_flags.p[2];
  if (B <= 0 || B > G.cap)
    return e->fail(BPF_ERR_HIP, "in-place resample: distinct key count outside the lists (internal error)");
  const bool bins_mode = kld_bins(e);
  bool done = false;
  if (B >= 8192 && !e->kld_persistent)
  {
    // the device tree over the whole list leaves the leaf count after every key behind (d_kld_counts)
    bool handled = bins_mode;
    if (!bins_mode)
    {
      KldOutcome dev;
      H2D_OR_RETURN(kld_tree_on_device(e, B, &dev, true));
      handled = dev.handled;
      if (handled && dev.bins != B)
        return e->fail(BPF_ERR_HIP, "in-place resample: the device tree saw repeated keys (internal error)");
    }
    else
    {
      rc = ensure_limit_table(e, B);
      if (rc != BPF_OK)
        return rc;
    }
    if (handled)
    {
      int* words = e->d_mn_words.p;
      const int2* cnt = bins_mode ? nullptr : (const int2*)e->d_kld_counts.p;
      HIPCHK(e, hipMemsetAsync(words + 1, 0x7F, sizeof(int), e->stream));
      hipLaunchKernelGGL(k_mn_stop, dim3(blocks_for(B, 256)), dim3(256), 0, e->stream, (const int*)e->d_mn_t.p, B, cnt,
                         (const int*)e->d_kld_limit.p, maxs, words + 1);
      hipLaunchKernelGGL(k_mn_stop_result, dim3(1), dim3(64), 0, e->stream, (const int*)e->d_mn_t.p, B, cnt,
                         (const int*)e->d_kld_limit.p, maxs, (const int*)(words + 1), words + 2);
      HIPCHK(e, hipGetLastError());
      int res[3] = { 0, 0, 0 };
      H2D_OR_RETURN(d2h_to_host(e, res, words + 2, sizeof(res), e->stream));
      *M_out = res[0];
      *leaf_out = res[1];
      *bins_out = res[2];
      *route_out = bins_mode ? BPF_SHARD_TREE_ROUTE_BIN_COUNT : BPF_SHARD_TREE_ROUTE_DEVICE;
      done = true;
    }
  }
  if (!done)
  {
    std::vector<int> t((size_t)B), keys;
    H2D_OR_RETURN(d2h_to_host(e, t.data(), e->d_mn_t.p, t.size() * sizeof(int), e->stream));
    if (!bins_mode)
    {
      keys.resize((size_t)B * 3);
      H2D_OR_RETURN(d2h_to_host(e, keys.data(), e->d_keys.p, keys.size() * sizeof(int), e->stream));
      e->hist.clear();
    }
    int M = maxs, L = 0, at = B - 1, cached_L = -1, cached_limit = 0;
    for (int j = 0; j < B; ++j)
    {
      if (!bins_mode)
      {
        e->hist.insert(keys[3 * (size_t)j], keys[3 * (size_t)j + 1], keys[3 * (size_t)j + 2]);
        L = e->hist.leaf_count();
      }
      else
        L = j + 1;
      if (L != cached_L)
      {
        cached_L = L;
        cached_limit = resample_limit(L, e->min_samples, e->max_samples, e->pop_err, e->pop_z);
      }
      const int c = std::max(t[(size_t)j] + 1, cached_limit + 1);
      const int t_next = j + 1 < B ? t[(size_t)j + 1] : maxs;
      if (c <= t_next)
      {
        M = c;
        at = j;
        break;
      }
    }
    *M_out = M;
    *leaf_out = L;
    *bins_out = at + 1;
    *route_out = bins_mode ? BPF_SHARD_TREE_ROUTE_BIN_COUNT : BPF_SHARD_TREE_ROUTE_HOST;
  }
  if (*M_out < 1 || *M_out > maxs)
    return e->fail(BPF_ERR_HIP, "in-place resample: stop count outside the stream (internal error)");
  return BPF_OK;
}

// every rank's count of the new set (no exchange), the check of this rank's truncation, and the miss flag: a candidate
// beyond the stop is a draw the reference never made
int mn_owner_counts(bpf_engine* e, int rank, int world, const double* edge, int n_kept, int M, void* flags_dev,
                    int* counts_out)
{
  MnOwnerArgs A{};
  int rc = mn_draw_args(e, rank, world, &A.W);
  if (rc != BPF_OK)
    return rc;
  for (int q = 0; q <= world; ++q)
    A.edge[q] = edge[q];
  A.world = world;
  A.M = M;
  int* words = e->d_mn_words.p;
  A.counts = words + 8;
  HIPCHK(e, hipMemsetAsync(words + 5, 0, (3 + kMailboxMaxWorld) * sizeof(int), e->stream));
  hipLaunchKernelGGL(k_mn_owner_hist, dim3(std::min(blocks_for(M, 256), 1024)), dim3(256), 0, e->stream, A);
  hipLaunchKernelGGL(k_mn_owner_check, dim3(1), dim3(64), 0, e->stream, (const int*)e->d_mn_idx.p, n_kept,
                     (const int*)(words + 8), rank, M, words + 5);
  HIPCHK(e, hipGetLastError());
  int h[8 + kMailboxMaxWorld];
  H2D_OR_RETURN(d2h_to_host(e, h, words, sizeof(h), e->stream));
  long long total = 0;
  for (int q = 0; q < world; ++q)
  {
    counts_out[q] = h[8 + q];
    total += h[8 + q];
  }
  if (h[5] != 1 || total != M)
    return e->fail(BPF_ERR_HIP, "in-place resample: the kept draws do not match the owners' counts (internal error)");
  if (h[0] >= 0 && h[0] < M)
    HIPCHK(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flags_dev), 1, 1, e->stream));
  return BPF_OK;
}

bool mn_cap_allows(const bpf_engine* e, const int* counts, int world, int M)
{
  int largest = 0;
  for (int q = 0; q < world; ++q)
    largest = std::max(largest, counts[q]);
  const long long even = ((long long)M + world - 1) / world;
  return e->shard_rebalance == BPF_SHARD_REBALANCE_AUTO || !((double)largest > e->shard_max_share * (double)even);
}

int mn_fill_weights(bpf_engine* e, int n_new, int M)
{
  if (n_new > 0)
  {
    hipLaunchKernelGGL(k_mn_fill_weight, dim3(blocks_for(n_new, 256)), dim3(256), 0, e->stream, e->sets[e->cur ^ 1].w.p,
                       n_new, 1.0 / (double)M);
    HIPCHK(e, hipGetLastError());
  }
  return BPF_OK;
}

// bpf_shard_update_resample's multinomial branch with the in-place form set: *done = false when this resample goes to the
// window form -- the imbalance cap, or a key outside the packing (the keys route would need the draw indices beside the
// keys) -- and nothing was changed.  Every exchange is finished before the new slice becomes current.
int shard_update_resample_in_place_mn(bpf_engine* e, void* flags_dev, uint64_t rng, bool* done, int* M_out, int* leaf_out,
                                      int* bins_out)
{
  *done = false;
  const int rank = e->shard_rank, W = e->shard_world;
  int rc = mn_check_begin(e, rng, e->mb_totals, rank, W, flags_dev);
  if (rc != BPF_OK)
    return rc;
  double edge[kMailboxMaxWorld + 1];
  rc = inplace_edges(e, e->mb_totals, 1, W, edge);
  if (rc != BPF_OK)
    return rc;
  int n_kept = 0, n_bins = 0, out_of_range = 0;
  rc = mn_select(e, rank, W, edge, &n_kept);
  if (rc == BPF_OK)
    rc = mn_bins(e, n_kept, &n_bins, &out_of_range);
  if (rc != BPF_OK)
    return rc;
  ShardExchange X{ e };
  long long bound[kMailboxMaxWorld];
  for (int r = 0; r < W; ++r)
    bound[r] = e->max_samples;  // (a rank may keep every candidate)
  int bin_counts_i[kMailboxMaxWorld], pad = 1;
  bool any_out = false;
  rc = shard_exchange_bin_lists(e, X, e->d_gt_bins.p, n_bins, out_of_range, bound,
                                "in-place resample: a bin count beyond the candidates arrived", bin_counts_i, &pad,
                                &any_out);
  if (rc != BPF_OK || any_out)
    return rc;
  int M = 0, leaf = 0, bins = 0, route = 0, counts[kMailboxMaxWorld] = { 0 };
  rc = mn_merge_stop(e, e->d_x_gather.p, bin_counts_i, W, pad, &M, &leaf, &bins, &route);
  if (rc == BPF_OK)
    rc = mn_owner_counts(e, rank, W, edge, n_kept, M, flags_dev, counts);
  if (rc != BPF_OK)
    return rc;
  if (!mn_cap_allows(e, counts, W, M))
    return BPF_OK;
  rc = mn_fill_weights(e, counts[rank], M);
  if (rc == BPF_OK)
    rc = inplace_finish(e, X, counts, M, leaf, bins, route, leaf_out, bins_out);
  if (rc != BPF_OK)
    return rc;
  *M_out = M;
  *done = true;
  return BPF_OK;
}
}  // namespace

int bpf_shard_set_multinomial_form(bpf_engine* e, int form)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (form != BPF_SHARD_RESAMPLE_WINDOW && form != BPF_SHARD_RESAMPLE_IN_PLACE)
    return e->fail(BPF_ERR_INVALID_ARGUMENT,
                   "multinomial form: BPF_SHARD_RESAMPLE_WINDOW or BPF_SHARD_RESAMPLE_IN_PLACE");
  e->shard_mn_form = form;
  return BPF_OK;
}

int bpf_shard_get_multinomial_form(const bpf_engine* e, int* form_out)
{
  if (!e || !form_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *form_out = e->shard_mn_form;
  return BPF_OK;
}

int bpf_shard_inplace_mn_select_dev(bpf_engine* e, uint64_t rng_state48, const void* sums_dev, int sums_are_totals,
                                    int rank, int world, void* flags_dev, int* n_kept_out)
{
  if (!e || !n_kept_out)
    return BPF_ERR_INVALID_ARGUMENT;
  e->ip_stage = 0;
  int rc = mn_check_begin(e, rng_state48, sums_dev, rank, world, flags_dev);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipSetDevice(e->device));
  rc = inplace_edges(e, sums_dev, sums_are_totals, world, e->mn.edge);
  if (rc != BPF_OK)
    return rc;
  rc = mn_select(e, rank, world, e->mn.edge, n_kept_out);
  if (rc != BPF_OK)
    return rc;
  e->mn.rank = rank;
  e->mn.world = world;
  e->mn.n_kept = *n_kept_out;
  e->mn.flags_dev = flags_dev;
  e->ip_stage = -1;
  e->ip_epoch = e->set_epoch;
  return BPF_OK;
}

int bpf_shard_inplace_mn_bins_dev(bpf_engine* e, void** bins_dev, int* n_bins_out, int* out_of_range_out)
{
  if (!e || !bins_dev || !n_bins_out || !out_of_range_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (e->ip_stage != -1 || e->ip_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_inplace_mn_select_dev first");
  HIPCHK(e, hipSetDevice(e->device));
  int rc = mn_bins(e, e->mn.n_kept, n_bins_out, out_of_range_out);
  if (rc != BPF_OK)
    return rc;
  *bins_dev = e->d_gt_bins.p;
  e->ip_stage = -2;
  return BPF_OK;
}

int bpf_shard_inplace_mn_stop_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                                  int* sample_count_out, int* leaf_count_out, int* bin_count_out, int* counts_out,
                                  long long* global_first_out, int* form_used_out)
{
  if (!e || !all_bins_dev || !counts || !sample_count_out || !leaf_count_out || !bin_count_out || !counts_out ||
      !global_first_out || !form_used_out || pad <= 0)
    return BPF_ERR_INVALID_ARGUMENT;
  if (e->ip_stage != -2 || e->ip_epoch != e->set_epoch)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "in-place resample: bpf_shard_inplace_mn_bins_dev first");
  if (world != e->mn.world)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "in-place resample: another world size than the select's");
  HIPCHK(e, hipSetDevice(e->device));
  e->ip_stage = 0;
  const int rank = e->mn.rank;
  int M = 0, leaf = 0, bins = 0, route = 0;
  int rc = mn_merge_stop(e, static_cast<const long long*>(all_bins_dev), counts, world, pad, &M, &leaf, &bins, &route);
  if (rc == BPF_OK)
    rc = mn_owner_counts(e, rank, world, e->mn.edge, e->mn.n_kept, M, e->mn.flags_dev, counts_out);
  if (rc != BPF_OK)
    return rc;
  long long first = 0;
  for (int r = 0; r < rank; ++r)
    first += counts_out[r];
  *sample_count_out = M;
  *global_first_out = first;
  *form_used_out = BPF_SHARD_RESAMPLE_WINDOW;
  *leaf_count_out = *bin_count_out = 0;
  if (!mn_cap_allows(e, counts_out, world, M))
    return BPF_OK;
  rc = mn_fill_weights(e, counts_out[rank], M);
  if (rc != BPF_OK)
    return rc;
  inplace_commit(e, counts_out[rank], first, M);
  tree_install(e, leaf, bins, route);
  *leaf_count_out = e->tree.leaf_count;
  *bin_count_out = e->tree.bin_count;
  *form_used_out = BPF_SHARD_RESAMPLE_IN_PLACE;
  e->ip_stage = 1;
  e->ip_epoch = e->set_epoch;
  return BPF_OK;
}
