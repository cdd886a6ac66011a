// C-ABI: pose search over a sharded filter (include/badger_pf.h) -- the four searches as one collective call each.
// Every rank runs the single-engine search (search_poses, search_poses_pruned, cloud_search_poses,
// cloud_search_poses_pruned) on its share of the range given, with a SearchShard (abi_pose_search.inl) that
//   - splits the range after the whole of it was checked, so that every rank refuses alike and before any exchange,
//   - behind the pruned forms' seed gathers one word per rank, the key of the K-th exact score, and folds the W words
//     into a floor under tau on the device (k_prune_floor_word, ShardExchange::gather, k_prune_floor),
//   - and in place of search_finish gathers the ranks' lists (k_search_pack_list: K + 1 entries of 16 bytes each),
//     folds them on the device (k_search_merge_lists) and fetches the K rows with search_finish itself.
// Every exchange goes through ShardExchange (abi_mailbox_step.inl).  The host waits where the single-engine call
// waits: the floor's exchange is checked behind the wait for the survivor counts, the lists' behind the rows'.
namespace
{
// the floor: enqueued behind the seed's last fold, in front of k_prune_survivors
int shard_search_share_floor(bpf_engine* e, SearchShard* sh, int k)
{
  ShardExchange X{ e };
  const int W = e->shard_world;
  HIPCHK(e, e->d_shard_floor.reserve((size_t)2 + kMailboxMaxWorld));
  unsigned long long* words = e->d_shard_floor.p;
  // (a gather that a mailbox wait gave up on leaves its destination alone: zeros, which set no floor)
  HIPCHK(e, hipMemsetAsync(words + 1, 0, (size_t)(1 + W) * sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(k_prune_floor_word, dim3(1), dim3(64), 0, e->stream, (const SearchEntry*)e->d_search_best.p,
                     (const int*)e->d_search_counts.p, k, words);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_prune_floor_word launch");
  long long counts[kMailboxMaxWorld], offs[kMailboxMaxWorld];
  for (int r = 0; r < W; ++r)
  {
    counts[r] = 1;
    offs[r] = r;
  }
  const long long* src[1] = { reinterpret_cast<const long long*>(words) };
  const int rc = X.gather(src, 1, counts, reinterpret_cast<long long*>(words + 2), offs, 0);
  if (rc != BPF_OK)
    return rc;
  hipLaunchKernelGGL(k_prune_floor, dim3(1), dim3(64), 0, e->stream, (const unsigned long long*)(words + 2), W,
                     words + 1);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_prune_floor launch");
  sh->floor_key = words + 1;
  return BPF_OK;
}

// behind the call's wait for the survivor counts: the stream is drained, what is left is the exchange's own check
int shard_search_floor_arrived(bpf_engine* e, SearchShard*)
{
  ShardExchange X{ e };
  return X.finish();
}

// the ranks' lists -> the best k of them all in d_search_best, then the rows as search_finish fetches them
int shard_search_finish(bpf_engine* e, SearchShard*, const SearchSpace& S, int k, bpf_pose_hit* hits_out,
                        int* n_hits_out)
{
  ShardExchange X{ e };
  const int W = e->shard_world;
  const size_t per = (size_t)k + 1;
  HIPCHK(e, e->d_shard_lists.reserve(per * (size_t)(1 + W)));
  SearchEntry* mine = e->d_shard_lists.p;
  SearchEntry* all = e->d_shard_lists.p + per;
  // (counts of zero where a mailbox wait gave up: finish() below tells, and the rows are not handed out)
  HIPCHK(e, hipMemsetAsync(all, 0, per * (size_t)W * sizeof(SearchEntry), e->stream));
  hipLaunchKernelGGL(k_search_pack_list, dim3(1), dim3(kSearchThreads), 0, e->stream,
                     (const SearchEntry*)e->d_search_best.p, (const int*)e->d_search_counts.p, k, mine);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_search_pack_list launch");
  long long counts[kMailboxMaxWorld], offs[kMailboxMaxWorld];
  for (int r = 0; r < W; ++r)
  {
    counts[r] = 2 * (long long)per;
    offs[r] = (long long)r * 2 * (long long)per;
  }
  const long long* src[1] = { reinterpret_cast<const long long*>(mine) };
  int rc = X.gather(src, 1, counts, reinterpret_cast<long long*>(all), offs, 0);
  if (rc != BPF_OK)
    return rc;
  int kp = 2;
  while (kp < k)
    kp <<= 1;
  HIPCHK(e, hipMemsetAsync(e->d_search_counts.p, 0, sizeof(int), e->stream));
  hipLaunchKernelGGL(k_search_merge_lists, dim3(1), dim3(kSearchThreads), 0, e->stream, e->d_search_best.p,
                     e->d_search_counts.p, k, kp, (const SearchEntry*)all, W);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_search_merge_lists launch");
  int n_hits = 0;
  rc = search_finish(e, S, k, hits_out, &n_hits);  // (waits for the rows)
  if (rc == BPF_OK)
    rc = X.finish();
  if (rc != BPF_OK)
    return rc;
  *n_hits_out = n_hits;
  return BPF_OK;
}

// what every sharded search checks first: a connected world whose exchange can carry the lists
int shard_search_ready(bpf_engine* e, int k, SearchShard* sh)
{
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  const int W = e->shard_world;
  if (W < 1 || W > kMailboxMaxWorld)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "sharded pose search: 1 .. 16 ranks");
  if (k >= 1 && k <= kSearchMaxK && e->mb.active && (long long)W * (2 * k + 2) > 6 * e->mb.max_window)
    return e->fail(BPF_ERR_CAPACITY, "sharded pose search: the mailbox windows are smaller than the ranks' lists");
  sh->rank = e->shard_rank;
  sh->world = W;
  sh->floor_key = nullptr;
  return BPF_OK;
}
}  // namespace

int bpf_shard_search_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                           double range_max, int headings, int cell_stride, long long first, long long count, int k,
                           bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchShard sh;
  int rc = shard_search_ready(e, k, &sh);
  if (rc != BPF_OK)
    return rc;
  SearchStateGuard guard(e);
  rc = search_poses(e, ranges, angles, range_count, range_max, headings, cell_stride, first, count, k, hits_out,
                    n_hits_out, &sh);
  guard.restore();
  return rc;
}

int bpf_shard_search_poses_pruned(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                  double range_max, int headings, int cell_stride, int block, int first_block,
                                  int block_count, int k, bpf_pose_hit* hits_out, int* n_hits_out,
                                  bpf_pose_search_stats* stats_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchShard sh;
  int rc = shard_search_ready(e, k, &sh);
  if (rc != BPF_OK)
    return rc;
  SearchStateGuard guard(e);
  rc = search_poses_pruned(e, ranges, angles, range_count, range_max, headings, cell_stride, block, first_block,
                           block_count, k, hits_out, n_hits_out, stats_out, &sh);
  guard.restore();
  return rc;
}

int bpf_shard_cloud_search_poses(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                                 long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchShard sh;
  int rc = shard_search_ready(e, k, &sh);
  if (rc != BPF_OK)
    return rc;
  CloudSearchStateGuard guard(e);
  rc = cloud_search_poses(e, points_xyz, n_points, headings, cell_stride, first, count, k, hits_out, n_hits_out, &sh);
  guard.restore();
  return rc;
}

int bpf_shard_cloud_search_poses_pruned(bpf_engine* e, const float* points_xyz, int n_points, int headings,
                                        int cell_stride, int block, int first_block, int block_count, int k,
                                        bpf_pose_hit* hits_out, int* n_hits_out, bpf_pose_search_stats* stats_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchShard sh;
  int rc = shard_search_ready(e, k, &sh);
  if (rc != BPF_OK)
    return rc;
  CloudSearchStateGuard guard(e);
  rc = cloud_search_poses_pruned(e, points_xyz, n_points, headings, cell_stride, block, first_block, block_count, k,
                                 hits_out, n_hits_out, stats_out, &sh);
  guard.restore();
  return rc;
}
