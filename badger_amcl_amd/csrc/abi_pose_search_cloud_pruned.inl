// C-ABI: pruned pose search with the 3-D map and the cloud scanner (include/badger_pf.h,
// kernels_pose_search_cloud_pruned.hpp) -- the rows of bpf_cloud_search_poses from fewer exact evaluations.  The call
// is the planar one (abi_pose_search_pruned.inl) over the rectangle form of the space: the cloud and the term table
// staged once, the bounds of all block candidates (anchor poses scored by launch_cloud against the pooled volume P_B
// with a neutral off-map factor), the seed expanded and scored exactly, then the block candidates whose bound is not
// below tau.  Everything is enqueued on the engine's stream; behind the staging this thread waits for the number of
// survivors (it sizes the expansion's windows) and for the rows.
//
// Read-only for the filter, as bpf_cloud_search_poses is: the entry points save and put back what the scoring
// launches reset, and profiling is off for the call.
namespace
{
// floor(a / b) for b > 0 and a of either sign
int floor_div(int a, int b)
{
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// what both entry points check alike before anything is launched: the kernel form the bound pass needs, the model's
// monotone epilogue, the factor; fills the bound's form
int prune3_model_check(bpf_engine* e, PruneBoundForm* F)
{
  const CloudModelDev& cm = e->cm;
  if (!(cm.tf_quat[0] == 0.0 && cm.tf_quat[1] == 0.0))
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned cloud pose search: a mounting with roll or pitch");
  if (!cloud_border_form(e))
    return e->fail(BPF_ERR_UNSUPPORTED,
                   "pruned cloud pose search: needs the dense volume and two free distance ratios (border codes)");
  const bool gompertz = cm.model == BPF_CLOUD_MODEL_GOMPERTZ;
  if (gompertz && !(cm.g.a > 0.0 && cm.g.b > 0.0 && cm.g.c > 0.0 && cm.g.input_scale > 0.0))
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned cloud pose search: Gompertz needs a, b, c and input_scale > 0");
  if (!(cm.off_map_factor >= 0.0))
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned cloud pose search: off_map_factor below zero or NaN");
  F->f_max = std::max(1.0, cm.off_map_factor);
  F->f_min = std::min(1.0, cm.off_map_factor);
  // Gompertz: 16 ulp of (a + |p|), DESIGN.md section 5
  F->margin_abs = gompertz ? 16.0 * 2.220446049250313e-16 * cm.g.a : 0.0;
  F->margin_rel = gompertz ? 16.0 * 2.220446049250313e-16 : 0.0;
  return BPF_OK;
}

// (a) of the proof: every coordinate the float transform can form for an anchor or a member -- the rotated point, the
// mounting's offset, a pose of the rectangle extended by B cells -- stays so small that the few float roundings
// between an anchor's and a member's world coordinate are below half a cell.  A point with a non-finite coordinate
// is replaced by 1e30 at staging (k_cloud_score): rotated, one of its world coordinates is beyond 7e29 at every
// heading, for the anchor and the members alike, so it is off the map for all of them and not counted here.
int prune3_cloud_check(bpf_engine* e, const float* points_xyz, int n_points, int block)
{
  const Map3dDev& M = e->map3;
  double cloud = 0.0;
  for (int q = 0; q < n_points; ++q)
  {
    const float x = points_xyz[3 * q], y = points_xyz[3 * q + 1], z = points_xyz[3 * q + 2];
    if (!(std::fabs(x) <= 3.0e38f) || !(std::fabs(y) <= 3.0e38f) || !(std::fabs(z) <= 3.0e38f))
      continue;
    cloud = std::max(cloud, (double)std::fabs(x) + (double)std::fabs(y));
  }
  int cells = 0;
  for (int d = 0; d < 2; ++d)
    cells = std::max(cells, std::max(std::abs(M.min_c[d]), std::abs(M.max_c[d])));
  const double largest =
      cloud + std::fabs(e->cm.tf_xyz[0]) + std::fabs(e->cm.tf_xyz[1]) + (double)(cells + block) * M.resolution;
  if (!(largest * 4.76837158203125e-07 < M.resolution))  // 2^-21
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned cloud pose search: coordinates too large for the resolution (2^-21 rule)");
  return BPF_OK;
}

// (b) of the proof, on the host copy of the table stage_cloud just filled
int prune3_table_check(bpf_engine* e)
{
  const double* t = e->h_cloud_table.p;
  for (int k = 0; k <= 256; ++k)
    if (!(t[k] == t[k]) || (k > 0 && !(t[k] <= t[k - 1])))
      return e->fail(BPF_ERR_UNSUPPORTED, "pruned cloud pose search: the per-ratio terms are not non-increasing");
  return BPF_OK;
}

// P_B on the device for the current 3-D map, cached per (map version, B); reserved on first use
int ensure_pooled_volume(bpf_engine* e, int block, const uint8_t** vol_out)
{
  bpf_engine::PrunePool3& pool = e->prune_pool3[prune_slot_of(block)];
  if (pool.map3_version != e->map3_version)
  {
    const Map3dDev& M = e->map3;
    const int nz = M.max_c[2] - M.min_c[2] + 1;
    Pool3Geom G{};
    G.w2 = M.max_c[0] - M.min_c[0] + 3;
    G.h2 = M.max_c[1] - M.min_c[1] + 3;
    G.ntx = (int)((M.dense_k + 1) / 8);
    G.nty = (int)(M.dense_plane / ((unsigned)G.ntx * 64u));
    G.plane = M.dense_plane;
    G.border = (unsigned)M.border_code;
    G.B = block;
    HIPCHK(e, pool.vol.reserve((size_t)M.dense_plane * ((size_t)nz + 1)));
    // the row pass of as many planes at a time as 64 MiB of scratch hold
    const size_t per_plane = (size_t)G.w2 * G.h2;
    const int zc = (int)std::max<size_t>(1, std::min<size_t>(std::min(nz, 65535), ((size_t)64 << 20) / per_plane));
    HIPCHK(e, e->d_prune_rows3.reserve(per_plane * zc));
    for (int z0 = 0; z0 < nz; z0 += zc)
    {
      const int nzc = std::min(zc, nz - z0);
      hipLaunchKernelGGL(k_pool3_rows, dim3(blocks_for(G.w2, 256), G.h2, nzc), dim3(256), 0, e->stream, G,
                         M.dense + (size_t)z0 * M.dense_plane, e->d_prune_rows3.p);
      hipLaunchKernelGGL(k_pool3_cols, dim3(blocks_for(G.ntx * 8, 64), blocks_for(G.nty * 8, 64), nzc), dim3(256), 0,
                         e->stream, G, (const uint8_t*)e->d_prune_rows3.p, pool.vol.p + (size_t)z0 * M.dense_plane);
    }
    if (hipGetLastError() != hipSuccess)
      return e->fail(BPF_ERR_HIP, "pooled volume launch");
    HIPCHK(e, hipMemsetAsync(pool.vol.p + (size_t)nz * M.dense_plane, M.zero_code, M.dense_plane, e->stream));
    pool.map3_version = e->map3_version;
  }
  *vol_out = pool.vol.p;
  return BPF_OK;
}

// one axis of the block list: the blocks that hold a column first + a * stride, a in [0, n), as (block index, first
// a) pairs in ascending order, closed by n
void block_axis_of(int first, int n, int stride, int block, std::vector<int>* index, std::vector<int>* start)
{
  index->clear();
  start->clear();
  for (int a = 0; a < n; ++a)
  {
    const int b = floor_div(first + a * stride, block);
    if (index->empty() || index->back() != b)
    {
      index->push_back(b);
      start->push_back(a);
    }
  }
  start->push_back(n);
}

// the block list of (stride, B) over the rectangle C_s: per-axis arrays, per-block starts and anchors, cached per
// (3-D map version, stride, B)
int ensure_block_rect(bpf_engine* e, const SearchSpace& S, int block, bpf_engine::PruneRect** out)
{
  bpf_engine::PruneRect& L = e->prune_rect[prune_slot_of(block)];
  *out = &L;
  if (L.map3_version == e->map3_version && L.stride == S.stride)
    return BPF_OK;
  const int n_i = S.n_j > 0 ? S.n_cells / S.n_j : 0;
  std::vector<int> bi, ai, bj, aj;
  block_axis_of(S.i0, n_i, S.stride, block, &bi, &ai);
  block_axis_of(S.j0, S.n_j, S.stride, block, &bj, &aj);
  const long long n_blocks = (long long)bi.size() * (long long)bj.size();
  if (n_blocks > (1ll << 26))
    return e->fail(BPF_ERR_CAPACITY, "pruned cloud pose search: more than 2^26 blocks (raise block)");
  std::vector<int2> anchor((size_t)n_blocks);
  L.h_start.assign(1, 0);
  L.h_start.reserve((size_t)n_blocks + 1);
  L.max_members = 0;
  for (size_t ib = 0; ib < bi.size(); ++ib)
    for (size_t jb = 0; jb < bj.size(); ++jb)
    {
      const int members = (ai[ib + 1] - ai[ib]) * (aj[jb + 1] - aj[jb]);
      anchor[ib * bj.size() + jb] = make_int2(bi[ib] * block, bj[jb] * block);
      L.h_start.push_back(L.h_start.back() + members);
      L.max_members = std::max(L.max_members, members);
    }
  L.n_blocks = (int)n_blocks;
  L.nbj = (int)bj.size();
  HIPCHK(e, L.start.reserve(L.h_start.size()));
  HIPCHK(e, L.axis_i.reserve(ai.size()));
  HIPCHK(e, L.axis_j.reserve(aj.size()));
  HIPCHK(e, L.anchor.reserve(std::max<size_t>(anchor.size(), 1)));
  L.map3_version = -1;  // (until every array is up)
  H2D_OR_RETURN(h2d_from_host(e, L.start.p, L.h_start.data(), L.h_start.size() * sizeof(int), e->stream));
  H2D_OR_RETURN(h2d_from_host(e, L.axis_i.p, ai.data(), ai.size() * sizeof(int), e->stream));
  H2D_OR_RETURN(h2d_from_host(e, L.axis_j.p, aj.data(), aj.size() * sizeof(int), e->stream));
  H2D_OR_RETURN(h2d_from_host_sync(e, L.anchor.p, anchor.data(), anchor.size() * sizeof(int2)));
  L.map3_version = e->map3_version;
  L.stride = S.stride;
  return BPF_OK;
}

struct Prune3Call
{
  SearchSpace S;
  bpf_engine::PruneRect* list;
  const uint8_t* pool;
  PruneBoundForm form;
  int headings, n_points;
  bool scored;
};

// argument checks, refusals and the block list, shared by the search and the bounds call
int prune3_prepare(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride, int block,
                   Prune3Call* call)
{
  if (!points_xyz || n_points <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pruned pose search: a cloud is needed");
  if (prune_slot_of(block) < 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pruned pose search: block is one of 2, 4, 8, 16, 32, 64");
  long long total = 0;
  int rc = cloud_search_space_of(e, headings, cell_stride, &call->S, &total);
  if (rc != BPF_OK)
    return rc;
  if (!e->cloud_configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the point-cloud model: none is set");
  rc = prune3_model_check(e, &call->form);
  if (rc != BPF_OK)
    return rc;
  rc = prune3_cloud_check(e, points_xyz, n_points, block);
  if (rc != BPF_OK)
    return rc;
  if (total > 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "pose search: more than 2^31 - 1 candidates (raise cell_stride or lower headings)");
  HIPCHK(e, hipSetDevice(e->device));
  rc = ensure_block_rect(e, call->S, block, &call->list);
  if (rc != BPF_OK)
    return rc;
  call->headings = headings;
  call->n_points = n_points;
  call->scored = e->cloud_max_beams >= 2;  // (below that applyModelToSampleSet leaves the weight 1.0)
  call->pool = nullptr;
  return BPF_OK;
}

// the cloud and the table on the device, the table checked, P_B, and the scoring scratch for a full window
int prune3_stage(bpf_engine* e, const float* points_xyz, int block, Prune3Call* call)
{
  HIPCHK(e, e->cand.reserve((size_t)kSearchWindow));
  if (!call->scored)  // every score and every bound is the weight 1.0 the candidates are written with
    return BPF_OK;
  int rc = stage_cloud(e, points_xyz, call->n_points);  // (waits for the stream: nothing below frees a buffer in use)
  if (rc != BPF_OK)
    return rc;
  rc = prune3_table_check(e);
  if (rc != BPF_OK)
    return rc;
  rc = ensure_pooled_volume(e, block, &call->pool);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, e->d_affine.reserve((size_t)kSearchWindow * 12));
  HIPCHK(e, e->d_cloud_partials.reserve((size_t)blocks_for(call->n_points, kCloudChunk) * kSearchWindow));
  return BPF_OK;
}

PruneBlocks prune3_blocks_of(const Prune3Call& call, int first_block)
{
  PruneBlocks b{};
  b.start = call.list->start.p;
  b.member = nullptr;
  b.anchor = call.list->anchor.p;
  b.first_block = first_block;
  b.headings = call.headings;
  b.axis_i = call.list->axis_i.p;
  b.axis_j = call.list->axis_j.p;
  b.nbj = call.list->nbj;
  b.n_j = call.S.n_j;
  return b;
}

// one exact window as it stands in e->cand (poses) and e->d_prune_ids: scored, folded into the exact list
int prune3_score_fold(bpf_engine* e, const Prune3Call& call, int n, int k)
{
  if (call.scored)
  {
    const int rc = launch_cloud(e, e->cand.dev(), n, call.n_points);
    if (rc != BPF_OK)
      return rc;
  }
  return prune_fold(e, n, k);
}

// bounds of the global block candidates q0 .. q0 + nq - 1 into e->d_prune_bounds[0 .. nq), window by window; k > 0:
// folded into the bound list (ids = index into the range) as they come
int prune3_bound_pass(bpf_engine* e, const Prune3Call& call, long long q0, long long nq, int k, long long* windows)
{
  int kp = 2;
  while (kp < k)
    kp <<= 1;
  for (long long done = 0; done < nq; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(nq - done, kSearchWindow);
    hipLaunchKernelGGL(k_prune_anchors, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(), n, q0 + done,
                       (const int2*)call.list->anchor.p, call.S);
    if (hipGetLastError() != hipSuccess)
      return e->fail(BPF_ERR_HIP, "k_prune_anchors launch");
    if (call.scored)
    {
      const int rc = launch_cloud(e, e->cand.dev(), n, call.n_points, call.pool);
      if (rc != BPF_OK)
        return rc;
    }
    hipLaunchKernelGGL(k_prune_bounds, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, (const double*)e->cand.w.p, n,
                       e->d_prune_bounds.p + done, call.form);
    if (k > 0)
    {
      const int tiles = blocks_for(n, kSearchTile);
      hipLaunchKernelGGL(k_search_select, dim3(tiles), dim3(kSearchThreads), 0, e->stream,
                         (const double*)(e->d_prune_bounds.p + done), n, done, k,
                         (const SearchEntry*)e->d_prune_best.p, (const int*)e->d_prune_best_count.p,
                         e->d_search_tiles.p, e->d_search_counts.p + 1);
      hipLaunchKernelGGL(k_search_merge, dim3(1), dim3(kSearchThreads), 0, e->stream, e->d_prune_best.p,
                         e->d_prune_best_count.p, k, kp, (const SearchEntry*)e->d_search_tiles.p,
                         (const int*)(e->d_search_counts.p + 1), tiles);
    }
    if (hipGetLastError() != hipSuccess)
      return e->fail(BPF_ERR_HIP, "pruned pose search bound launch");
    ++*windows;
  }
  return BPF_OK;
}

int cloud_search_poses_pruned(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                              int block, int first_block, int block_count, int k, bpf_pose_hit* hits_out,
                              int* n_hits_out, bpf_pose_search_stats* stats_out, SearchShard* sh = nullptr)
{
  if (!hits_out || !n_hits_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: an output is needed");
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  Prune3Call call;
  int rc = prune3_prepare(e, points_xyz, n_points, headings, cell_stride, block, &call);
  if (rc != BPF_OK)
    return rc;
  const bpf_engine::PruneRect& L = *call.list;
  if (first_block < 0 || first_block > L.n_blocks || block_count < -1 ||
      (block_count >= 0 && block_count > L.n_blocks - first_block))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pruned pose search: first_block / block_count outside the block list");
  if (block_count < 0)
    block_count = L.n_blocks - first_block;
  if (sh)
  {
    // the capacity limit holds for every rank's share, checked on every rank alike; then this rank's share
    long long mine_first = first_block, mine = block_count;
    for (int r = 0; r < sh->world; ++r)
    {
      long long f, c;
      shard_search_share(r, sh->world, first_block, block_count, &f, &c);
      if (c * headings > kPruneMaxBlockCandidates)
        return e->fail(BPF_ERR_CAPACITY, "pruned pose search: more than 2^24 block candidates in a rank's share");
      if (r == sh->rank)
        mine_first = f, mine = c;
    }
    first_block = (int)mine_first;
    block_count = (int)mine;
  }
  const long long nq = (long long)block_count * headings;
  if (nq > kPruneMaxBlockCandidates)
    return e->fail(BPF_ERR_CAPACITY, "pruned pose search: more than 2^24 block candidates (split the range or raise block)");
  bpf_pose_search_stats st{};
  st.candidates = (long long)(L.h_start[(size_t)first_block + block_count] - L.h_start[(size_t)first_block]) * headings;
  st.block_candidates = nq;
  *n_hits_out = 0;
  if (stats_out)
    *stats_out = st;
  if (nq == 0 && !sh)
    return BPF_OK;
  rc = prune3_stage(e, points_xyz, block, &call);  // (the table's refusal: before any exchange, on every rank alike)
  if (rc != BPF_OK)
    return rc;
  if (nq == 0)
  {
    // an empty share: nothing is scored, the list stays empty, and the rank takes part in every exchange
    rc = search_begin(e);
    if (rc == BPF_OK)
      rc = shard_search_share_floor(e, sh, k);
    if (rc == BPF_OK)
      rc = shard_search_floor_arrived(e, sh);
    if (rc == BPF_OK)
      rc = shard_search_finish(e, sh, call.S, k, hits_out, n_hits_out);
    if (rc != BPF_OK)
      (void)hipStreamSynchronize(e->stream);
    return rc;
  }

  const int n_chunks = blocks_for((int)nq, kPruneChunk);
  HIPCHK(e, e->d_prune_bounds.reserve((size_t)nq));
  HIPCHK(e, e->d_prune_in_seed.reserve((size_t)nq));
  HIPCHK(e, e->d_prune_best.reserve(kSearchMaxK));
  HIPCHK(e, e->d_prune_best_count.reserve(1));
  HIPCHK(e, e->d_prune_seed.reserve(2 * kSearchMaxK + 1));
  HIPCHK(e, e->d_prune_ids.reserve((size_t)kSearchWindow));
  HIPCHK(e, e->d_prune_surv.reserve((size_t)2 * n_chunks * kPruneChunk));
  HIPCHK(e, e->d_prune_state.reserve((size_t)n_chunks * kPruneChunk));
  HIPCHK(e, e->d_prune_chunks.reserve((size_t)n_chunks));
  HIPCHK(e, e->d_prune_chunk_off.reserve((size_t)n_chunks + 1));
  HIPCHK(e, e->d_prune_words.reserve(kPruneWords));
  HIPCHK(e, e->h_prune_chunks.reserve((size_t)n_chunks));
  HIPCHK(e, e->h_prune_chunk_off.reserve((size_t)n_chunks + 1));
  HIPCHK(e, e->h_prune_words.reserve(kPruneWords));
  rc = search_begin(e);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, hipMemsetAsync(e->d_prune_best_count.p, 0, sizeof(int), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_prune_words.p, 0, kPruneWords * sizeof(unsigned long long), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_prune_in_seed.p, 0, (size_t)nq, e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_prune_state.p, 0, (size_t)n_chunks * kPruneChunk, e->stream));
  // from the first launch on, a failure returns with the stream drained
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  const PruneBlocks blocks = prune3_blocks_of(call, first_block);
  int* seed_q = e->d_prune_seed.p;
  int* seed_off = e->d_prune_seed.p + kSearchMaxK;
  int* surv_q = e->d_prune_surv.p;
  int* surv_off = e->d_prune_surv.p + (size_t)n_chunks * kPruneChunk;

  // 2. bounds, and the best kPruneSeed of them (the seed is as large as the bound list whatever k is, as in the planar
  // call)
  rc = prune3_bound_pass(e, call, (long long)first_block * headings, nq, kPruneSeed, &st.windows);
  if (rc != BPF_OK)
    return drained(rc);

  // 3. the seed: at most min(kPruneSeed, nq) block candidates of at most max_members members each
  hipLaunchKernelGGL(k_prune_seed_plan, dim3(1), dim3(1024), 0, e->stream, (const SearchEntry*)e->d_prune_best.p,
                     (const int*)e->d_prune_best_count.p, blocks, seed_q, seed_off, e->d_prune_in_seed.p,
                     e->d_prune_words.p);
  if (hipGetLastError() != hipSuccess)
    return drained(e->fail(BPF_ERR_HIP, "k_prune_seed_plan launch"));
  const long long seed_room = std::min(std::min<long long>(kPruneSeed, nq) * (long long)L.max_members, st.candidates);
  for (long long done = 0; done < seed_room; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(seed_room - done, kSearchWindow);
    hipLaunchKernelGGL(k_prune_expand_seed, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(),
                       e->d_prune_ids.p, n, done, (const int*)seed_q, (const int*)seed_off,
                       (const unsigned long long*)e->d_prune_words.p, blocks, call.S);
    if (hipGetLastError() != hipSuccess)
      return drained(e->fail(BPF_ERR_HIP, "k_prune_expand_seed launch"));
    rc = prune3_score_fold(e, call, n, k);
    if (rc != BPF_OK)
      return drained(rc);
    ++st.windows;
  }

  // 4. the survivors; the host sums the chunks' totals.  A sharded search first shares tau: from here on the ranks
  // prune against the largest K-th score any of them holds behind its seed
  const unsigned long long* floor_key = nullptr;
  if (sh)
  {
    rc = shard_search_share_floor(e, sh, k);
    if (rc != BPF_OK)
      return drained(rc);
    floor_key = sh->floor_key;
  }
  hipLaunchKernelGGL(k_prune_survivors, dim3(n_chunks), dim3(kPruneChunk), 0, e->stream,
                     (const double*)e->d_prune_bounds.p, (int)nq, (const uint8_t*)e->d_prune_in_seed.p,
                     (const SearchEntry*)e->d_search_best.p, (const int*)e->d_search_counts.p, k, floor_key, blocks,
                     surv_q, surv_off, e->d_prune_chunks.p);
  if (hipGetLastError() != hipSuccess)
    return drained(e->fail(BPF_ERR_HIP, "k_prune_survivors launch"));
  rc = pinned_down_sync(e, e->h_prune_chunks, 0, e->d_prune_chunks, 0, (size_t)n_chunks, e->stream);
  if (rc == BPF_OK && sh)
    rc = shard_search_floor_arrived(e, sh);  // (the floor's exchange rides on this wait)
  if (rc != BPF_OK)
    return drained(rc);
  long long survivors = 0, members = 0;
  for (int c = 0; c < n_chunks; ++c)
  {
    e->h_prune_chunk_off.p[c] = members;
    survivors += e->h_prune_chunks.p[c].x;
    members += e->h_prune_chunks.p[c].y;
  }
  e->h_prune_chunk_off.p[n_chunks] = members;
  rc = pinned_up(e, e->d_prune_chunk_off, 0, e->h_prune_chunk_off, 0, (size_t)n_chunks + 1, e->stream);
  if (rc != BPF_OK)
    return drained(rc);

  // 5. expansion, every window behind the one before
  for (long long done = 0; done < members; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(members - done, kSearchWindow);
    hipLaunchKernelGGL(k_prune_expand, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(),
                       e->d_prune_ids.p, n, done, (const double*)e->d_prune_bounds.p,
                       (const SearchEntry*)e->d_search_best.p, (const int*)e->d_search_counts.p, k, floor_key,
                       (const int*)surv_q, (const int*)surv_off, (const int2*)e->d_prune_chunks.p,
                       (const long long*)e->d_prune_chunk_off.p, n_chunks, e->d_prune_state.p, e->d_prune_words.p,
                       blocks, call.S);
    if (hipGetLastError() != hipSuccess)
      return drained(e->fail(BPF_ERR_HIP, "k_prune_expand launch"));
    rc = prune3_score_fold(e, call, n, k);
    if (rc != BPF_OK)
      return drained(rc);
    ++st.windows;
  }

  // 6. the rows, and the counters with them
  rc = pinned_down(e, e->h_prune_words, 0, e->d_prune_words, 0, kPruneWords, e->stream);
  if (rc != BPF_OK)
    return drained(rc);
  rc = sh ? shard_search_finish(e, sh, call.S, k, hits_out, n_hits_out)
          : search_finish(e, call.S, k, hits_out, n_hits_out);
  if (rc != BPF_OK)
    return drained(rc);
  const unsigned long long* w = e->h_prune_words.p;
  st.seed_candidates = (long long)w[0];
  st.expanded_block_candidates = (long long)w[3];
  st.pruned_block_candidates = (nq - (long long)w[0] - survivors) + (long long)w[2];
  st.scored_candidates = (long long)w[1] + (long long)w[4];
  if (stats_out)
    *stats_out = st;
  return BPF_OK;
}

int cloud_search_bounds(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride, int block,
                        long long first_q, long long count, double* bounds_out)
{
  if (!bounds_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search bounds: an output is needed");
  Prune3Call call;
  int rc = prune3_prepare(e, points_xyz, n_points, headings, cell_stride, block, &call);
  if (rc != BPF_OK)
    return rc;
  const long long total = (long long)call.list->n_blocks * headings;
  if (first_q < 0 || first_q > total || count < -1 || (count >= 0 && count > total - first_q))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search bounds: first_q / count outside the block candidates");
  if (count < 0)
    count = total - first_q;
  if (count > kPruneMaxBlockCandidates)
    return e->fail(BPF_ERR_CAPACITY, "pose search bounds: more than 2^24 block candidates in one call");
  if (count == 0)
    return BPF_OK;
  rc = prune3_stage(e, points_xyz, block, &call);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, e->d_prune_bounds.reserve((size_t)count));
  long long windows = 0;
  rc = prune3_bound_pass(e, call, first_q, count, 0, &windows);
  if (rc != BPF_OK)
  {
    (void)hipStreamSynchronize(e->stream);
    return rc;
  }
  return d2h_to_host(e, bounds_out, e->d_prune_bounds.p, (size_t)count * sizeof(double), e->stream);
}

// what the scoring launches reset describes the engine's last scoring call, not the candidates: saved here, put back
// by restore().  Profiling is off in between, so no event slot is taken.
struct CloudSearchStateGuard
{
  bpf_engine* e;
  WeightCaches caches;
  long long evals;
  int status, form;
  bool profiling;
  explicit CloudSearchStateGuard(bpf_engine* eng)
    : e(eng), caches(eng->wc), evals(eng->evals_last), status(eng->last_status), form(eng->last_cloud_form),
      profiling(eng->profiling)
  {
    e->profiling = false;
  }
  void restore()
  {
    e->profiling = profiling;
    e->wc = caches;
    e->evals_last = evals;
    e->last_status = status;
    e->last_cloud_form = form;
  }
};
}  // namespace

int bpf_cloud_search_poses_pruned(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                                  int block, int first_block, int block_count, int k, bpf_pose_hit* hits_out,
                                  int* n_hits_out, bpf_pose_search_stats* stats_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  CloudSearchStateGuard guard(e);
  const int rc = cloud_search_poses_pruned(e, points_xyz, n_points, headings, cell_stride, block, first_block,
                                           block_count, k, hits_out, n_hits_out, stats_out);
  guard.restore();
  return rc;
}

int bpf_cloud_search_blocks(bpf_engine* e, int cell_stride, int block, int* n_blocks_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  int rc = BPF_OK;
  SearchSpace S;
  long long total = 0;
  if (cell_stride < 1 || prune_slot_of(block) < 0 || !n_blocks_out)
    rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search blocks: cell_stride >= 1, block one of 2 .. 64, an output");
  else if ((rc = cloud_search_space_of(e, 1, cell_stride, &S, &total)) == BPF_OK)
  {
    (void)hipSetDevice(e->device);
    bpf_engine::PruneRect* L = nullptr;
    rc = ensure_block_rect(e, S, block, &L);
    if (rc == BPF_OK)
      *n_blocks_out = L->n_blocks;
  }
  e->last_status = status;
  return rc;
}

int bpf_cloud_search_pooled_lut(bpf_engine* e, int block, unsigned char* bytes_out, long long capacity,
                                long long* n_out, int* ntx_out, int* nty_out, int* planes_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  int rc = BPF_OK;
  if (prune_slot_of(block) < 0 || !n_out)
    rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pooled volume: block one of 2 .. 64 and an output are needed");
  else if (!e->have_map3d)
    rc = e->fail(BPF_ERR_NOT_CONFIGURED, "cloud pose search needs the 3-D map (bpf_map3d_set)");
  else if (e->map3.dense == nullptr || e->map3.border_code < 0)
    rc = e->fail(BPF_ERR_UNSUPPORTED, "pooled volume: needs the dense volume and two free distance ratios");
  else
  {
    const Map3dDev& M = e->map3;
    const int planes = M.max_c[2] - M.min_c[2] + 2;  // the map's and the zero plane
    const int ntx = (int)((M.dense_k + 1) / 8);
    const long long n = (long long)M.dense_plane * planes;
    *n_out = n;
    if (ntx_out)
      *ntx_out = ntx;
    if (nty_out)
      *nty_out = (int)(M.dense_plane / ((unsigned)ntx * 64u));
    if (planes_out)
      *planes_out = planes;
    if (bytes_out != nullptr && capacity < n)
      rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pooled volume: the output holds fewer bytes than the volume");
    else if (bytes_out != nullptr)
    {
      (void)hipSetDevice(e->device);
      const uint8_t* vol = nullptr;
      rc = ensure_pooled_volume(e, block, &vol);
      if (rc == BPF_OK)
        rc = d2h_to_host(e, bytes_out, vol, (size_t)n, e->stream);
    }
  }
  e->last_status = status;
  return rc;
}

int bpf_cloud_search_bounds(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                            int block, long long first_q, long long count, double* bounds_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  CloudSearchStateGuard guard(e);
  const int rc = cloud_search_bounds(e, points_xyz, n_points, headings, cell_stride, block, first_q, count, bounds_out);
  guard.restore();
  return rc;
}
