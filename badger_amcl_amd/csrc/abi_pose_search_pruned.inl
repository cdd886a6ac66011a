// C-ABI: pruned pose search (include/badger_pf.h, kernels_pose_search_pruned.hpp) -- the rows of
// bpf_planar_search_poses from fewer exact evaluations.  Bounds of all block candidates first (anchor poses scored by
// score_planar against the pooled image P_B, FieldRequest::bound_tiles), the seed expanded and scored exactly, then
// the block candidates whose bound is not below tau.  Everything is enqueued on the engine's stream; this thread
// waits for the number of survivors (it sizes the expansion's windows) and for the rows.
//
// Read-only for the filter, as the exhaustive search is: the entry points save and put back what the scoring calls
// reset.
namespace
{
static_assert(sizeof(bpf_pose_search_stats) == 7 * sizeof(long long), "bpf_pose_search_stats is seven long long");

// slot of a block size in the engine's per-B caches, or -1
int prune_slot_of(int block)
{
  for (int s = 0; s < 6; ++s)
    if (block == (2 << s))
      return s;
  return -1;
}

// P_B on the device for the current map, cached per (map version, B)
int ensure_pooled_lut(bpf_engine* e, int block, const uint16_t** tiles_out)
{
  bpf_engine::PrunePool& pool = e->prune_pool[prune_slot_of(block)];
  if (pool.map_version != e->map_version)
  {
    const MapDev& M = e->map;
    const int Wp = M.size_x + 2, Hp = M.size_y + 2;
    HIPCHK(e, pool.tiles.reserve((size_t)M.ltx * M.lty * 64));
    HIPCHK(e, e->d_prune_rows.reserve((size_t)Wp * Hp));
    const unsigned koff = (unsigned)M.n_levels * 8u;
    hipLaunchKernelGGL(k_pool_rows, dim3(blocks_for(Wp, 256), Hp), dim3(256), 0, e->stream, M, block, koff,
                       e->d_prune_rows.p);
    hipLaunchKernelGGL(k_pool_cols, dim3(blocks_for(M.ltx * 8, 64), blocks_for(M.lty * 8, 64)), dim3(256), 0,
                       e->stream, M, block, koff, (const uint16_t*)e->d_prune_rows.p, pool.tiles.p);
    if (hipGetLastError() != hipSuccess)
      return e->fail(BPF_ERR_HIP, "pooled LUT image launch");
    pool.map_version = e->map_version;
  }
  *tiles_out = pool.tiles.p;
  return BPF_OK;
}

// the block list of (stride, B) with its members in CSR over F_s, built on the host as ensure_free_list builds F_s
// (the same walk, the same test), cached per (map version, radius, stride, B)
int ensure_block_list(bpf_engine* e, int stride, int block, bpf_engine::PruneList** out)
{
  bpf_engine::PruneList& L = e->prune_list[prune_slot_of(block)];
  const double radius = e->pm.non_free_radius;
  *out = &L;
  if (L.map_version == e->map_version && L.radius == radius && L.stride == stride)
    return BPF_OK;
  const int sx = e->map.size_x, sy = e->map.size_y;
  const int nbj = (sy + block - 1) / block, nbi = (sx + block - 1) / block;
  std::vector<int> count((size_t)nbi * nbj + 1, 0);
  std::vector<int> key_of;  // block key of entry f of F_s
  for (int i = 0; i < sx; i += stride)
    for (int j = 0; j < sy; j += stride)
    {
      const size_t idx = i + (size_t)j * sx;
      if (e->h_cells8[idx] == -1 && (double)e->h_lut_f32[idx] > radius)
      {
        const int key = (i / block) * nbj + j / block;
        key_of.push_back(key);
        ++count[(size_t)key];
      }
    }
  // non-empty blocks in key order (bi outer, bj inner); index_of[key] = its place in the list
  std::vector<int> index_of((size_t)nbi * nbj, -1);
  std::vector<int2> anchor;
  L.h_start.assign(1, 0);
  L.max_members = 0;
  for (int key = 0; key < nbi * nbj; ++key)
    if (count[(size_t)key] > 0)
    {
      index_of[(size_t)key] = (int)anchor.size();
      anchor.push_back(make_int2((key / nbj) * block, (key % nbj) * block));
      L.h_start.push_back(L.h_start.back() + count[(size_t)key]);
      L.max_members = std::max(L.max_members, count[(size_t)key]);
    }
  std::vector<int> fill(L.h_start.begin(), L.h_start.end() - 1), member(key_of.size());
  for (size_t f = 0; f < key_of.size(); ++f)
    member[(size_t)fill[(size_t)index_of[(size_t)key_of[f]]]++] = (int)f;
  L.n_blocks = (int)anchor.size();
  HIPCHK(e, L.start.reserve(L.h_start.size()));
  HIPCHK(e, L.member.reserve(std::max<size_t>(member.size(), 1)));
  HIPCHK(e, L.anchor.reserve(std::max<size_t>(anchor.size(), 1)));
  H2D_OR_RETURN(h2d_from_host(e, L.start.p, L.h_start.data(), L.h_start.size() * sizeof(int), e->stream));
  H2D_OR_RETURN(h2d_from_host(e, L.member.p, member.data(), member.size() * sizeof(int), e->stream));
  H2D_OR_RETURN(h2d_from_host_sync(e, L.anchor.p, anchor.data(), anchor.size() * sizeof(int2)));
  L.map_version = e->map_version;
  L.radius = radius;
  L.stride = stride;
  return BPF_OK;
}

// what both entry points check alike, before anything is launched; fills the bound's form
int prune_model_check(bpf_engine* e, double range_max, PruneBoundForm* F)
{
  const PlanarModel& pm = e->pm;
  if (pm.model != BPF_MODEL_LIKELIHOOD_FIELD && pm.model != BPF_MODEL_LIKELIHOOD_FIELD_GOMPERTZ)
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned pose search: likelihood field and likelihood-field Gompertz only");
  const bool gompertz = pm.model == BPF_MODEL_LIKELIHOOD_FIELD_GOMPERTZ;
  if (gompertz && !(pm.g.a > 0.0 && pm.g.b > 0.0 && pm.g.c > 0.0 && pm.g.input_scale > 0.0))
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned pose search: Gompertz needs a, b, c and input_scale > 0");
  if (!(pm.off_map_factor >= 0.0 && pm.non_free_factor >= 0.0))
    return e->fail(BPF_ERR_UNSUPPORTED, "pruned pose search: map factors below zero or NaN");
  // the per-level terms as the kernel will read them (host copy of the same table)
  const int K = e->map.n_levels;
  std::vector<double> table((size_t)K + 1);
  fill_term_table(e, range_max, table.data());
  for (int k = 0; k <= K; ++k)
    if (!(table[(size_t)k] == table[(size_t)k]) || (k > 0 && !(table[(size_t)k] <= table[(size_t)k - 1])))
      return e->fail(BPF_ERR_UNSUPPORTED, "pruned pose search: the per-level terms are not non-increasing");
  F->f_max = std::max(1.0, std::max(pm.off_map_factor, pm.non_free_factor));
  F->f_min = std::min(1.0, std::min(pm.off_map_factor, pm.non_free_factor));
  // Gompertz: 16 ulp of (a + |p|), DESIGN.md section 5
  F->margin_abs = gompertz ? 16.0 * 2.220446049250313e-16 * pm.g.a : 0.0;
  F->margin_rel = gompertz ? 16.0 * 2.220446049250313e-16 : 0.0;
  return BPF_OK;
}

struct PruneCall
{
  SearchSpace S;
  bpf_engine::PruneList* list;
  const uint16_t* pool;
  PruneBoundForm form;
  int headings;
};

// argument checks, refusals and the caches, shared by the search and the bounds call
int prune_prepare(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                  int headings, int cell_stride, int block, PruneCall* call)
{
  if (!ranges || !angles || range_count <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pruned pose search: a scan is needed");
  if (headings < 1 || cell_stride < 1)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: headings >= 1 and cell_stride >= 1 are needed");
  if (prune_slot_of(block) < 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pruned pose search: block is one of 2, 4, 8, 16, 32, 64");
  if (!e->pm.configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the planar models: none is set");
  if (!e->have_map || !e->have_lut)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search needs the 2-D map and its distance LUT");
  int rc = prune_model_check(e, range_max, &call->form);
  if (rc != BPF_OK)
    return rc;
  long long total = 0;
  rc = search_space_of(e, headings, cell_stride, &call->S, &total);
  if (rc != BPF_OK)
    return rc;
  if (total > 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "pose search: more than 2^31 - 1 candidates (raise cell_stride or lower headings)");
  rc = ensure_block_list(e, cell_stride, block, &call->list);
  if (rc != BPF_OK)
    return rc;
  call->headings = headings;
  call->pool = nullptr;
  return BPF_OK;
}

PruneBlocks prune_blocks_of(const PruneCall& call, int first_block)
{
  return PruneBlocks{ call.list->start.p, call.list->member.p, call.list->anchor.p, first_block, call.headings };
}

// one exact window as it stands in e->cand (poses, scored) and e->d_prune_ids, folded into the exact list
int prune_fold(bpf_engine* e, int n, int k)
{
  int kp = 2;
  while (kp < k)
    kp <<= 1;
  const int tiles = blocks_for(n, kSearchTile);
  hipLaunchKernelGGL(k_prune_select, dim3(tiles), dim3(kSearchThreads), 0, e->stream, (const double*)e->cand.w.p, n,
                     (const long long*)e->d_prune_ids.p, k, (const SearchEntry*)e->d_search_best.p,
                     (const int*)e->d_search_counts.p, e->d_search_tiles.p, e->d_search_counts.p + 1);
  hipLaunchKernelGGL(k_search_merge, dim3(1), dim3(kSearchThreads), 0, e->stream, e->d_search_best.p,
                     e->d_search_counts.p, k, kp, (const SearchEntry*)e->d_search_tiles.p,
                     (const int*)(e->d_search_counts.p + 1), tiles);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "pruned pose search selection launch");
  return BPF_OK;
}

// one exact window as it stands in e->cand (poses) and e->d_prune_ids: scored, folded into the exact list
int prune_score_fold(bpf_engine* e, int n, int k, const double* ranges, const double* angles, int range_count,
                     double range_max)
{
  if (e->pm.max_beams >= 2)
  {
    bool forced_zero = false;
    const int rc = score_planar(e, e->cand.dev(), n, 0, ranges, angles, range_count, range_max, &forced_zero);
    if (rc != BPF_OK)
      return rc;
  }
  return prune_fold(e, n, k);
}

// bounds of the global block candidates q0 .. q0 + nq - 1 into e->d_prune_bounds[0 .. nq), window by window; k > 0:
// folded into the bound list (ids = index into the range) as they come
int prune_bound_pass(bpf_engine* e, const PruneCall& call, long long q0, long long nq, int k, const double* ranges,
                     const double* angles, int range_count, double range_max, long long* windows)
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
    if (e->pm.max_beams >= 2)
    {
      bool forced_zero = false;
      const int rc = score_planar(e, e->cand.dev(), n, 0, ranges, angles, range_count, range_max, &forced_zero, false,
                                  false, nullptr, call.pool);
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

int search_poses_pruned(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                        int headings, int cell_stride, int block, int first_block, int block_count, int k,
                        bpf_pose_hit* hits_out, int* n_hits_out, bpf_pose_search_stats* stats_out,
                        SearchShard* sh = nullptr)
{
  if (!hits_out || !n_hits_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: an output is needed");
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  PruneCall call;
  int rc = prune_prepare(e, ranges, angles, range_count, range_max, headings, cell_stride, block, &call);
  if (rc != BPF_OK)
    return rc;
  const bpf_engine::PruneList& L = *call.list;
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
  rc = ensure_pooled_lut(e, block, &call.pool);
  if (rc != BPF_OK)
    return rc;

  const int n_chunks = blocks_for((int)nq, kPruneChunk);
  HIPCHK(e, e->cand.reserve((size_t)kSearchWindow));
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
  const PruneBlocks blocks = prune_blocks_of(call, first_block);
  int* seed_q = e->d_prune_seed.p;
  int* seed_off = e->d_prune_seed.p + kSearchMaxK;
  int* surv_q = e->d_prune_surv.p;
  int* surv_off = e->d_prune_surv.p + (size_t)n_chunks * kPruneChunk;

  // 2. bounds, and the best kPruneSeed of them.  The seed is not min(k, nq) block candidates but as many as the bound
  // list can hold: a seed window costs the same launch whether 16 or 65 536 of its slots are filled, and with a small
  // k the tau of k rows' members is loose -- measured with k = 1 on the bench map, most block candidates then
  // survive step 4, are dropped only at their windows, and the call is slower than the exhaustive search
  // (profiles/pose_search_pruned.md)
  rc = prune_bound_pass(e, call, (long long)first_block * headings, nq, kPruneSeed, ranges, angles, range_count,
                        range_max, &st.windows);
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
    rc = prune_score_fold(e, n, k, ranges, angles, range_count, range_max);
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
    rc = prune_score_fold(e, n, k, ranges, angles, range_count, range_max);
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

int search_bounds(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                  int headings, int cell_stride, int block, long long first_q, long long count, double* bounds_out)
{
  if (!bounds_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search bounds: an output is needed");
  PruneCall call;
  int rc = prune_prepare(e, ranges, angles, range_count, range_max, headings, cell_stride, block, &call);
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
  rc = ensure_pooled_lut(e, block, &call.pool);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, e->cand.reserve((size_t)kSearchWindow));
  HIPCHK(e, e->d_prune_bounds.reserve((size_t)count));
  long long windows = 0;
  rc = prune_bound_pass(e, call, first_q, count, 0, ranges, angles, range_count, range_max, &windows);
  if (rc != BPF_OK)
  {
    (void)hipStreamSynchronize(e->stream);
    return rc;
  }
  return d2h_to_host(e, bounds_out, e->d_prune_bounds.p, (size_t)count * sizeof(double), e->stream);
}

// what the scoring calls reset describes the engine's set, not the candidates: saved here, put back by restore()
struct SearchStateGuard
{
  bpf_engine* e;
  WeightCaches caches;
  long long evals;
  int status, form;
  bool window_path;
  explicit SearchStateGuard(bpf_engine* eng)
    : e(eng), caches(eng->wc), evals(eng->evals_last), status(eng->last_status), form(eng->last_score_form),
      window_path(eng->last_used_window_path)
  {
  }
  void restore()
  {
    e->wc = caches;
    e->evals_last = evals;
    e->last_status = status;
    e->last_score_form = form;
    e->last_used_window_path = window_path;
  }
};
}  // namespace

int bpf_planar_search_poses_pruned(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                   double range_max, int headings, int cell_stride, int block, int first_block,
                                   int block_count, int k, bpf_pose_hit* hits_out, int* n_hits_out,
                                   bpf_pose_search_stats* stats_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchStateGuard guard(e);
  const int rc = search_poses_pruned(e, ranges, angles, range_count, range_max, headings, cell_stride, block,
                                     first_block, block_count, k, hits_out, n_hits_out, stats_out);
  guard.restore();
  return rc;
}

int bpf_planar_search_blocks(bpf_engine* e, int cell_stride, int block, int* n_blocks_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  int rc = BPF_OK;
  if (cell_stride < 1 || prune_slot_of(block) < 0 || !n_blocks_out)
    rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search blocks: cell_stride >= 1, block one of 2 .. 64, an output");
  else if (!e->have_map || !e->have_lut)
    rc = e->fail(BPF_ERR_NOT_CONFIGURED, "pose search needs the 2-D map and its distance LUT");
  else
  {
    (void)hipSetDevice(e->device);
    bpf_engine::PruneList* L = nullptr;
    rc = ensure_block_list(e, cell_stride, block, &L);
    if (rc == BPF_OK)
      *n_blocks_out = L->n_blocks;
  }
  e->last_status = status;
  return rc;
}

int bpf_planar_search_pooled_lut(bpf_engine* e, int block, unsigned short* tiles_out, long long capacity,
                                 long long* n_out, int* ltx_out, int* lty_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  int rc = BPF_OK;
  if (prune_slot_of(block) < 0 || !n_out)
    rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pooled LUT image: block one of 2 .. 64 and an output are needed");
  else if (!e->have_map || !e->have_lut)
    rc = e->fail(BPF_ERR_NOT_CONFIGURED, "pose search needs the 2-D map and its distance LUT");
  else
  {
    const long long n = (long long)e->map.ltx * e->map.lty * 64;
    *n_out = n;
    if (ltx_out)
      *ltx_out = e->map.ltx;
    if (lty_out)
      *lty_out = e->map.lty;
    if (tiles_out != nullptr && capacity < n)
      rc = e->fail(BPF_ERR_INVALID_ARGUMENT, "pooled LUT image: the output holds fewer entries than the image");
    else if (tiles_out != nullptr)
    {
      (void)hipSetDevice(e->device);
      const uint16_t* tiles = nullptr;
      rc = ensure_pooled_lut(e, block, &tiles);
      if (rc == BPF_OK)
        rc = d2h_to_host(e, tiles_out, tiles, (size_t)n * sizeof(uint16_t), e->stream);
    }
  }
  e->last_status = status;
  return rc;
}

int bpf_planar_search_bounds(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                             double range_max, int headings, int cell_stride, int block, long long first_q,
                             long long count, double* bounds_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  SearchStateGuard guard(e);
  const int rc = search_bounds(e, ranges, angles, range_count, range_max, headings, cell_stride, block, first_q, count,
                               bounds_out);
  guard.restore();
  return rc;
}
