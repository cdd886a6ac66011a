// Host half of normalisation and resampling: CDF, updateConverged, free-space list and draw chain (recovery),
// KLD stop rule (device tree and ordered host replay), multinomial and systematic resamplers.
// BPF_KLD_COUNT_BINS: the stop rule's k is the number of distinct histogram keys (bpf_pf_set_kld_count)
bool kld_bins(const bpf_engine* e)
{
  return e->kld_count_mode == BPF_KLD_COUNT_BINS;
}

// a new ordered replay (e->seen, and the histogram tree or the distinct-key count)
void kld_host_reset(bpf_engine* e, int expected)
{
  e->hist.clear();
  e->seen.reset((size_t)expected);
  e->kld_host_bins = 0;
}

// one key of an ordered replay: a first occurrence enters the histogram tree (LEAVES: e->seen is a cache in front of
// the tree, which folds repeats itself) or only the count (BINS: the set's answer must be exact)
bool kld_host_insert(bpf_engine* e, int x, int y, int t)
{
  if (kld_bins(e))
  {
    if (!e->seen.first_time_exact(x, y, t))
      return false;
    ++e->kld_host_bins;
    return true;
  }
  if (!e->seen.first_time(x, y, t))
    return false;
  e->hist.insert(x, y, t);
  return true;
}

// the stop rule's k for the keys the replay has seen
int kld_host_k(const bpf_engine* e)
{
  return kld_bins(e) ? e->kld_host_bins : e->hist.leaf_count();
}

int fetch_scalars(bpf_engine* e)
{
  H2D_OR_RETURN(pinned_down(e, e->h_scalars, 0, e->d_scalars, 0, 1, e->stream));
  H2D_OR_RETURN(pinned_down_sync(e, e->h_flags, 0, e->d_flags, 0, 8, e->stream));
  if (e->converged_pending)
  {
    // particle_filter.cpp:206-219, float arithmetic for the percentage
    const double pct = (float)e->h_flags.p[1] / (float)e->conv_n * 100;
    e->percent_converged = (float)pct;
    e->converged = pct >= e->conv_threshold;
    e->converged_pending = false;
  }
  return BPF_OK;
}

// k_resample_block stages every (1 << shift)-th CDF value in LDS: the smallest shift that fits kFusedCoarse brackets
int fused_coarse_shift(int n)
{
  int shift = 0;
  while ((((n - 1) >> shift) + 1) > kFusedCoarse)
    shift++;
  return shift;
}

int ensure_cdf_buffers(bpf_engine* e, int n)
{
  HIPCHK(e, e->d_cdf.reserve((size_t)n + 1 + 64));  // slack: k_resample_block reads whole 32-value brackets
  if (!e->d_cdf_guide.p)
  {
    HIPCHK(e, e->d_cdf_guide.reserve(kCdfGuide + 2));
    HIPCHK(e, hipMemsetAsync(e->d_cdf_guide.p, 0xFF, (kCdfGuide + 2) * sizeof(int), e->stream));  // "no entry"
  }
  return BPF_OK;
}

// ParticleFilter::updateSensor's normalisation and the CDF of the normalised weights in one launch (k_normalize_cdf);
// needs the scoring kernel's per-block partials (e->wc.fused_partials) and at most 256 tiles
int launch_normalize_cdf(bpf_engine* e, double* w, int n)
{
  const int nb = std::max(1, blocks_for(n, BPF_RED_TILE));
  int rc = ensure_cdf_buffers(e, n);
  if (rc != BPF_OK)
    return rc;
  if (e->d_tile_slots.cap < (size_t)2 * BPF_RED_BLOCK)
  {
    HIPCHK(e, e->d_tile_slots.reserve((size_t)2 * BPF_RED_BLOCK));
    HIPCHK(e, hipMemsetAsync(e->d_tile_slots.p, 0xFF, 2 * BPF_RED_BLOCK * sizeof(unsigned long long), e->stream));
    e->tile_generation = 0;
  }
  NormCdfArgs A{};
  A.w = w;
  A.n = n;
  A.block_partials = e->d_block_partials.p;
  A.n_partials = e->wc.fused_partials;
  A.sc = e->d_scalars.p;
  A.alpha_slow = e->alpha_slow;
  A.alpha_fast = e->alpha_fast;
  A.tile_slots = e->d_tile_slots.p;
  A.generation = ++e->tile_generation;  // (only its parity matters)
  A.cdf = e->d_cdf.p;
  A.coarse_shift = fused_coarse_shift(n);
  HIPCHK(e, e->d_cdf_coarse.reserve((size_t)kFusedCoarse + 2));
  A.coarse = e->d_cdf_coarse.p;
  // k_resample_block searches through the subsample; the guide table is for the general path's draw kernel, worth its
  // writes only when a long draw stream is expected (the previous resample ran to the end: a spread cloud)
  const bool want_guide = e->window_hint >= e->max_samples;
  if (debug_on())
    fprintf(stderr, "[normalize_cdf] n %d window_hint %d max %d guide %d\n", n, e->window_hint, e->max_samples, (int)want_guide);
  A.guide = want_guide ? e->d_cdf_guide.p : nullptr;
  A.zero_word = e->d_flags.p;
  ProfScope ps(e, BPF_K_NORMALIZE);
  hipLaunchKernelGGL(k_normalize_cdf, dim3(nb), dim3(BPF_RED_BLOCK), 0, e->stream, A);
  HIPCHK(e, hipGetLastError());
  e->wc.cdf_left(n, want_guide);
  return BPF_OK;
}

// zero_word2 / sum_out (optional): a second miss flag to clear and where to leave c[n], both written by the scan
// itself instead of by a memset and a copy behind it
int build_cdf(bpf_engine* e, const double* w, int n, int* zero_word2 = nullptr, double* sum_out = nullptr)
{
  if (e->wc.cdf_ready_n == n && w == e->sets[e->cur].w.p && !e->cdf_serial && zero_word2 == nullptr &&
      sum_out == nullptr)
    return BPF_OK;  // k_normalize_cdf left it behind
  int rcb = ensure_cdf_buffers(e, n);
  if (rcb != BPF_OK)
    return rcb;
  e->wc.cdf_scan_begins(!e->cdf_serial);
  ProfScope ps(e, BPF_K_CDF);
  if (e->cdf_serial)
  {
    hipLaunchKernelGGL(k_scan_serial, dim3(1), dim3(64), 0, e->stream, w, n, e->d_cdf.p);
    HIPCHK(e, hipMemsetAsync(e->d_flags.p, 0, sizeof(int), e->stream));
    if (zero_word2)
      HIPCHK(e, hipMemsetAsync(zero_word2, 0, sizeof(int), e->stream));
    if (sum_out)
      HIPCHK(e, copy_d2d(sum_out, (const double*)e->d_cdf.p + n, 1, e->stream));
  }
  else
  {
    const int nb = std::max(1, blocks_for(n, BPF_RED_TILE));
    double* tiles;
    if (e->wc.tile_sums_n == n && w == e->sets[e->cur].w.p)
    {
      tiles = e->d_tile_sums.p;  // left behind by k_normalize_fused; consumed (scanned in place) here
      e->wc.drop();
    }
    else
    {
      HIPCHK(e, e->d_partials.reserve((size_t)nb));
      tiles = e->d_partials.p;
      hipLaunchKernelGGL(k_sum_partials, dim3(nb), dim3(BPF_RED_BLOCK), 0, e->stream, w, n, tiles);
    }
    if (nb <= 256)
    {
      // few tiles: every block of the final pass forms its own offset (one launch less)
      hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(BPF_RED_BLOCK), 0, e->stream, w, n, tiles, 0, e->d_cdf.p,
                         e->d_flags.p, e->d_cdf_guide.p, zero_word2, sum_out);
    }
    else
    {
      hipLaunchKernelGGL(k_scan_tile_offsets, dim3(1), dim3(BPF_RED_BLOCK), 0, e->stream, tiles, nb, e->d_flags.p);
      hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(BPF_RED_BLOCK), 0, e->stream, w, n, tiles, 1, e->d_cdf.p,
                         nullptr, e->d_cdf_guide.p, zero_word2, sum_out);
    }
  }
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// updateConverged (particle_filter.cpp:170-220) on the current set, result fetched lazily
int launch_converged(bpf_engine* e)
{
  SampleSet& s = e->sets[e->cur];
  const int n = e->sample_count;
  const int nb = std::max(1, blocks_for(n, BPF_RED_TILE));
  HIPCHK(e, e->d_partials.reserve((size_t)2 * nb));
  const int grid = std::max(1, std::min(blocks_for(n, 256), 1024));
  ProfScope ps(e, BPF_K_FINALIZE);
  hipLaunchKernelGGL(k_sum_xy_partials, dim3(nb), dim3(BPF_RED_BLOCK), 0, e->stream, (const double*)s.x.p,
                     (const double*)s.y.p, n, e->d_partials.p, e->d_partials.p + nb, e->d_flags.p + 1);
  hipLaunchKernelGGL(k_converged_count, dim3(grid), dim3(BPF_RED_BLOCK), 0, e->stream, (const double*)s.x.p,
                     (const double*)s.y.p, n, (const double*)e->d_partials.p, (const double*)(e->d_partials.p + nb), nb,
                     e->d_scalars.p, e->dist_threshold, e->d_flags.p + 1);
  HIPCHK(e, hipGetLastError());
  e->converged_pending = true;
  e->conv_n = n;
  return BPF_OK;
}

bool pose_check_scored(const bpf_engine* e);

// The list of Node2D::updateFreeSpaceIndices (node_2d.cpp:317-337) on the device for the current 2-D map and
// non_free_space_radius: FREE cells whose LUT distance (compared in double) is > radius, i outer, j inner; with
// stride s > 1 the entries with i % s == 0 && j % s == 0, in the same order.  Built on the host once per (map version,
// radius[, stride]) -- stride 1 in d_free_ij / n_free, the last other stride in d_free_s / n_free_s.  The caller has
// checked have_map && have_lut; no generator mode is asked for (ensure_free_space keeps those checks).
int ensure_free_list(bpf_engine* e, int stride, const int2** cells_out, int* n_out)
{
  const double radius = e->pm.non_free_radius;
  const bool unit = stride == 1;
  DevBuf<int2>& buf = unit ? e->d_free_ij : e->d_free_s;
  int& n = unit ? e->n_free : e->n_free_s;
  const bool cached = unit ? (e->free_map_version == e->map_version && e->free_radius == radius)
                           : (e->free_s_map_version == e->map_version && e->free_s_radius == radius &&
                              e->free_s_stride == stride);
  if (!cached)
  {
    const int sx = e->map.size_x, sy = e->map.size_y;
    std::vector<int2> ij;
    ij.reserve(((size_t)sx / stride + 1) * ((size_t)sy / stride + 1) / 2);
    for (int i = 0; i < sx; i += stride)
      for (int j = 0; j < sy; j += stride)
      {
        const size_t idx = i + (size_t)j * sx;
        if (e->h_cells8[idx] == -1 && (double)e->h_lut_f32[idx] > radius)
          ij.push_back(make_int2(i, j));
      }
    n = (int)ij.size();
    HIPCHK(e, buf.reserve(std::max<size_t>(ij.size(), 1)));
    if (!ij.empty())
      H2D_OR_RETURN(h2d_from_host_sync(e, buf.p, ij.data(), ij.size() * sizeof(int2)));
    if (unit)
    {
      e->free_map_version = e->map_version;
      e->free_radius = radius;
    }
    else
    {
      e->free_s_map_version = e->map_version;
      e->free_s_radius = radius;
      e->free_s_stride = stride;
    }
  }
  if (cells_out)
    *cells_out = buf.p;
  if (n_out)
    *n_out = n;
  return BPF_OK;
}

// Node2D::updateFreeSpaceIndices (node_2d.cpp:317-337) for the current map and non_free_space_radius, cached; or
// Node3D::updateFreeSpaceIndices (node_3d.cpp:306-318) over the 3-D map's cell bounds.  out->retries = the trials
// every call of Node::uniformPoseGenerator rejects (bpf_pf_set_uniform_pose_check).
int ensure_free_space(bpf_engine* e, FreeSpaceDev* out)
{
  if (e->random_pose_mode != BPF_RANDOM_POSE_FREE_SPACE_2D && e->random_pose_mode != BPF_RANDOM_POSE_FREE_SPACE_3D)
    return e->fail(BPF_ERR_UNSUPPORTED,
                   "w_diff > 0: random pose injection needs a pose generator (bpf_pf_set_random_pose_generator); "
                   "the node's random_pose_fn_ callback (particle_filter.cpp:385-388) cannot be called from here");
  if (e->pose_check_scoring == BPF_POSE_CHECK_SENSOR_MODEL && e->cloud_configured && e->pose_check_g0 > 0.0 &&
      e->pose_check_m < 1.0 && e->pose_check_m >= 0.0)
    return e->fail(BPF_ERR_UNSUPPORTED, "BPF_POSE_CHECK_SENSOR_MODEL scores with the planar models only");
  if (e->pose_retries < 0 && !pose_check_scored(e))
    return e->fail(BPF_ERR_CAPACITY, "the uniform pose check's threshold table does not reach the score within "
                                     "2^30 trials");
  *out = FreeSpaceDev{};
  out->retries = pose_check_scored(e) ? 0 : e->pose_retries;
  if (e->random_pose_mode == BPF_RANDOM_POSE_FREE_SPACE_3D)
  {
    if (!e->have_map3d)
      return e->fail(BPF_ERR_NOT_CONFIGURED, "random 3-D free-space poses need the 3-D map (bpf_map3d_set)");
    const Map3dDev& M = e->map3;
    const long long w = (long long)M.max_c[0] - M.min_c[0], h = (long long)M.max_c[1] - M.min_c[1];
    if (w <= 0 || h <= 0)
      return e->fail(BPF_ERR_NOT_CONFIGURED, "the 3-D map's cell bounds hold no column to draw random poses from");
    out->ij = nullptr;
    out->n = (int)(w * h);  // < (w + 1)(h + 1) = n_pose_indices < 2^30 (bpf_map3d_set)
    out->min_i = M.min_c[0];
    out->min_j = M.min_c[1];
    out->rect_h = (int)h;
    out->resolution = M.resolution;
    return BPF_OK;
  }
  if (!e->have_map || !e->have_lut)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "random free-space poses need the 2-D map and its distance LUT");
  int rcl = ensure_free_list(e, 1, nullptr, nullptr);
  if (rcl != BPF_OK)
    return rcl;
  if (e->n_free <= 0)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "the map has no free cell to draw random poses from");
  out->ij = e->d_free_ij.p;
  out->n = e->n_free;
  out->size_x = e->map.size_x;
  out->size_y = e->map.size_y;
  out->origin_x = e->map.origin_x;
  out->origin_y = e->map.origin_y;
  out->resolution = e->map.resolution;
  return BPF_OK;
}

// ---- BPF_POSE_CHECK_SENSOR_MODEL: Node::uniformPoseGenerator with the score its parameter documents -- the weight of
// the one-sample set {pose, 1.0} after applyModelToSampleSet with set->converged = 0 against the last planar scan.
// The trial poses are scored on the device in windows (k_candidate_poses, then the planar scoring kernels on the
// engine's candidate set); this thread runs the reference's loop over those scores, with good_weight *= m as the
// loop forms it, and the tests of the multinomial chain from the drand48 recurrence.  Every loop here is bounded by
// the 31-bit stream positions.
bool pose_check_scored(const bpf_engine* e)
{
  const double g0 = e->pose_check_g0, m = e->pose_check_m;
  return e->pose_check_scoring == BPF_POSE_CHECK_SENSOR_MODEL && e->have_scan && g0 > 0.0 && m < 1.0 && m >= 0.0;
}

constexpr unsigned kPosLimit = 0x7ffffff0u;  // stream positions a resolution may reach
constexpr int kScoreWindow = 16384;          // trial poses per scoring launch

struct TrialScores
{
  bpf_engine* e;
  FreeSpaceDev F;
  uint64_t rng0;
  unsigned stride;
  unsigned lo = 0, hi = 0;  // positions lo, lo + stride, ... < hi are scored

  // the score of the trial whose pose takes stream elements pos, pos + 1
  int score(unsigned pos, double* out)
  {
    if (pos < lo || pos >= hi)
    {
      long long cnt = ((long long)kPosLimit - pos) / stride;
      if (cnt <= 0)
        return e->fail(BPF_ERR_CAPACITY, "random pose calls would pass 31-bit stream positions");
      const int n = (int)std::min<long long>(cnt, kScoreWindow);
      HIPCHK(e, e->cand.reserve((size_t)n));
      hipLaunchKernelGGL(k_candidate_poses, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(), n, pos,
                         stride, rng0, e->jump, F);
      HIPCHK(e, hipGetLastError());
      // the scoring call resets the engine's per-set caches (partials, CDF hand-over); the candidate set is not the
      // engine's set, so they are put back
      const WeightCaches caches = e->wc;
      const long long ev = e->evals_last;
      bool forced_zero = false;
      int rc = score_planar(e, e->cand.dev(), n, 0, e->scan_ranges.data(), e->scan_angles.data(),
                            (int)e->scan_ranges.size(), e->scan_range_max, &forced_zero);
      e->wc = caches;
      e->evals_last = ev;
      if (rc != BPF_OK)
        return rc;
      e->h_cand_scores.resize((size_t)n);
      H2D_OR_RETURN(d2h_to_host(e, e->h_cand_scores.data(), e->cand.w.p, (size_t)n * sizeof(double), e->stream));
      lo = pos;
      hi = pos + (unsigned)n * stride;
    }
    *out = e->h_cand_scores[(pos - lo) / stride];
    return BPF_OK;
  }

  // one call of Node::uniformPoseGenerator (node.cpp:847-868) that starts at element p: *accepted = its pose's element
  int call(unsigned p, unsigned* accepted)
  {
    double good = e->pose_check_g0;
    const double m = e->pose_check_m;
    unsigned t = p;
    double sc = 0.0;
    int rc = score(t, &sc);
    while (rc == BPF_OK && sc < good)
    {
      t += 2;
      rc = score(t, &sc);
      good *= m;
    }
    *accepted = t;
    return rc;
  }
};

// n back-to-back calls from element `first`: e->h_accept[i] = call i's accepted element, *end = the element after the
// last call
int resolve_scored_calls(bpf_engine* e, const FreeSpaceDev& F, uint64_t rng0, unsigned first, int n, unsigned* end)
{
  if (e->cloud_configured)
    return e->fail(BPF_ERR_UNSUPPORTED, "BPF_POSE_CHECK_SENSOR_MODEL scores with the planar models only");
  TrialScores T{ e, F, rng0, 2 };
  e->h_accept.resize((size_t)std::max(n, 1));
  unsigned p = first;
  for (int i = 0; i < n; ++i)
  {
    int rc = T.call(p, &e->h_accept[i]);
    if (rc != BPF_OK)
      return rc;
    p = e->h_accept[i] + 2;
  }
  HIPCHK(e, e->d_accept.reserve((size_t)std::max(n, 1)));
  if (n > 0)
    H2D_OR_RETURN(h2d_from_host_sync(e, e->d_accept.p, e->h_accept.data(), (size_t)n * sizeof(unsigned)));
  *end = p;
  return BPF_OK;
}

// the multinomial draw chain (kernels_recovery.hpp's convention) for draws 0 .. max_draws - 1 with scored calls
int resolve_scored_chain(bpf_engine* e, const FreeSpaceDev& F, double w_diff, int max_draws)
{
  if (e->cloud_configured)
    return e->fail(BPF_ERR_UNSUPPORTED, "BPF_POSE_CHECK_SENSOR_MODEL scores with the planar models only");
  TrialScores T{ e, F, e->rng, 1 };
  e->h_chain.assign((size_t)max_draws + 1, 0);
  unsigned q = 1;                                    // the current test
  unsigned at = 1;                                   // x = element `at`
  uint64_t x = lcg_skip_host(e->rng, 1, e->jump);
  for (int m = 0; m < max_draws; ++m)
  {
    if (q >= kPosLimit)
      return e->fail(BPF_ERR_CAPACITY, "draw chain would pass 31-bit stream positions");
    if (q - at < 64)
      for (; at < q; ++at)
        x = (0x5DEECE66Dull * x + 0xBull) & ((1ull << 48) - 1);
    else
      x = lcg_skip_host(x, q - at, e->jump);
    at = q;
    if (std::ldexp((double)x, -48) < w_diff)
    {
      unsigned t = 0;
      int rc = T.call(q + 1, &t);
      if (rc != BPF_OK)
        return rc;
      e->h_chain[m] = (int)(t | 0x80000000u);
      q = t + 2;
    }
    else
    {
      e->h_chain[m] = (int)(q + 1);
      q += 2;
    }
  }
  HIPCHK(e, e->d_chain.reserve((size_t)max_draws + 1));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_chain.p, e->h_chain.data(), ((size_t)max_draws + 1) * sizeof(int)));
  return BPF_OK;
}

// Where every candidate draw 0 .. max_draws finds its stream elements when w_diff > 0 (kernels_recovery.hpp);
// `retries` = FreeSpaceDev::retries
int build_draw_chain(bpf_engine* e, double w_diff, int max_draws, int retries)
{
  const long long positions = (2ll * retries + 3) * ((long long)max_draws + 1) + 3;
  if (retries < 0 || positions >= 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "draw chain would pass 31-bit stream positions");
  if (retries > 0)
  {
    HIPCHK(e, e->d_chain.reserve((size_t)max_draws + 1));
    ChainArgs C{};
    C.rng_state = e->rng;
    C.w_diff = w_diff;
    C.max_draws = max_draws;
    C.chain = e->d_chain.p;
    C.retries = retries;
    C.jump = e->jump;
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_chain_chase, dim3(1), dim3(64), 0, e->stream, C);
    HIPCHK(e, hipGetLastError());
    return BPF_OK;
  }
  const int n_seg = (int)((positions + kChainSeg - 1) / kChainSeg);
  HIPCHK(e, e->d_chain_bits.reserve((size_t)2 * n_seg));
  HIPCHK(e, e->d_chain_cnt.reserve((size_t)3 * n_seg));
  HIPCHK(e, e->d_chain_exit.reserve((size_t)3 * n_seg));
  HIPCHK(e, e->d_chain_entry.reserve((size_t)n_seg));
  HIPCHK(e, e->d_chain_base.reserve((size_t)n_seg));
  HIPCHK(e, e->d_chain.reserve((size_t)max_draws + 1));
  ChainArgs C{};
  C.rng_state = e->rng;
  C.w_diff = w_diff;
  C.n_seg = n_seg;
  C.max_draws = max_draws;
  C.seg_bits = e->d_chain_bits.p;
  C.seg_cnt = e->d_chain_cnt.p;
  C.seg_exit = e->d_chain_exit.p;
  C.seg_entry = e->d_chain_entry.p;
  C.seg_base = e->d_chain_base.p;
  C.chain = e->d_chain.p;
  C.jump = e->jump;
  ProfScope ps(e, BPF_K_DRAW);
  hipLaunchKernelGGL(k_chain_segments, dim3(blocks_for(n_seg, 256)), dim3(256), 0, e->stream, C);
  hipLaunchKernelGGL(k_chain_scan, dim3(1), dim3(1024), 0, e->stream, C);
  hipLaunchKernelGGL(k_chain_emit, dim3(blocks_for(n_seg, 256)), dim3(256), 0, e->stream, C);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// resampleLimit per leaf count 0 .. upto on the device, cached per parameter set (host libm, as the reference
// evaluates it)
int ensure_limit_table(bpf_engine* e, int upto)
{
  if (e->kld_limit_key[0] != e->pop_err || e->kld_limit_key[1] != e->pop_z || e->kld_limit_key[2] != e->min_samples ||
      e->kld_limit_key[3] != e->max_samples || (int)e->kld_limit_host.size() < upto + 1)
  {
    const int n = std::max(upto, (int)e->kld_limit_host.size() - 1);
    e->kld_limit_host.resize((size_t)n + 1);
    for (int k = 0; k <= n; ++k)
      e->kld_limit_host[k] = resample_limit(k, e->min_samples, e->max_samples, e->pop_err, e->pop_z);
    HIPCHK(e, e->d_kld_limit.reserve((size_t)n + 1));
    H2D_OR_RETURN(h2d_from_host_sync(e, e->d_kld_limit.p, e->kld_limit_host.data(), ((size_t)n + 1) * sizeof(int)));
    e->kld_limit_key[0] = e->pop_err;
    e->kld_limit_key[1] = e->pop_z;
    e->kld_limit_key[2] = e->min_samples;
    e->kld_limit_key[3] = e->max_samples;
  }
  return BPF_OK;
}

// draw m takes stream element 2 m + 2: the composed LCG step for that distance, per draw of a window kernel
int ensure_fused_jump(bpf_engine* e)
{
  if (e->d_fused_jump.p)
    return BPF_OK;
  std::vector<FusedJump> jt(kFusedWindow);
  const uint64_t mask = (1ull << 48) - 1;
  for (int m = 0; m < kFusedWindow; ++m)
  {
    uint64_t a = 1, c = 0, k = 2ull * (uint64_t)m + 2ull;
    for (int j = 0; k != 0 && j < 48; ++j, k >>= 1)
      if (k & 1)
      {
        a = (a * e->jump.A[j]) & mask;
        c = (c * e->jump.A[j] + e->jump.C[j]) & mask;
      }
    jt[m].a = a;
    jt[m].c = c;
  }
  HIPCHK(e, e->d_fused_jump.reserve(kFusedWindow));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_fused_jump.p, jt.data(), jt.size() * sizeof(FusedJump)));
  HIPCHK(e, e->d_fused_keys.reserve(kFusedWindow));
  HIPCHK(e, e->d_fused_counter.reserve(1));
  // on the engine's stream: a plain hipMemset may still be in flight when the first launch counts its blocks
  HIPCHK(e, hipMemsetAsync(e->d_fused_counter.p, 0, sizeof(unsigned), e->stream));
  return BPF_OK;
}

// What the window kernels (k_resample_block, k_shard_stop_block and their kin) need ahead of the launch, in `A`: the
// limit table, the pinned result block, the kernel's LDS limit, a new generation and the debug flag
template <class Args, class Kernel>
int fused_block_arm(bpf_engine* e, Kernel* kernel, int window, bool systematic, Args* A)
{
  if (!systematic)
    H2D_OR_RETURN(ensure_limit_table(e, window));
  HIPCHK(e, e->h_fused.reserve(32));
  H2D_OR_RETURN(ensure_dynamic_lds(e, kernel, kFusedLds));
  A->limit = e->d_kld_limit.p;
  A->result_host = e->h_fused.p;
  e->fused_generation = next_generation(e->fused_generation);
  A->generation = e->fused_generation;
  A->debug = debug_on();
  A->lds_tree = e->fused_lds_tree ? 1 : 0;
  return BPF_OK;
}

// Waits for a window kernel's three result words (fused_publish in kernels_fused.hpp) of `generation` in e->h_fused
// (a ~25 us kernel); res[0..4] = M, leaf count, bin count, status, levels
int fused_result_wait(bpf_engine* e, int generation, const char* kernel_name, int res[5])
{
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(e->h_fused.p);
  int low[3] = { 0, 0, 0 };
  H2D_OR_RETURN(await_published(
      e, [&] { return tagged_words(w, 0, 3, (unsigned)generation, low); }, 50, kernel_name));
  res[0] = low[0];
  res[1] = (low[1] >> 16) & 0xFFFF;
  res[2] = low[1] & 0xFFFF;
  res[3] = (low[2] >> 8) & 0xFF;
  res[4] = low[2] & 0xFF;
  return BPF_OK;
}

// ---- what a resample made, whichever driver and regime ran.  The regimes fill it; bpf_pf_update_resample and
// bpf_shard_mailbox_update_resample commit it, and nothing else writes the engine's record of the last resample.
enum ResampleCountedBy  // (the values of bpf_pf_state::kld_on_device)
{
  COUNTED_BY_HOST_TREE = 0,    // the ordered replay into e->hist (or its distinct-key count in BINS mode)
  COUNTED_BY_DEVICE_TREE = 1,  // kld_tree_on_device
  COUNTED_BY_BLOCK = 2,        // a one-block kernel, which also wrote the weights and counted the converged particles
};

struct ResampleOutcome
{
  int M = 0, leaf = 0, bins = 0, windows = 0;
  ResampleCountedBy counted_by = COUNTED_BY_HOST_TREE;

  void counted(ResampleCountedBy by, int leaf_, int bins_)
  {
    counted_by = by;
    leaf = leaf_;
    bins = bins_;
  }
};

// the counts of the host's replay, as the stop rule's count mode reads them
void counted_by_host_tree(const bpf_engine* e, ResampleOutcome* out)
{
  out->counted(COUNTED_BY_HOST_TREE, kld_host_k(e), kld_bins(e) ? e->kld_host_bins : e->hist.bin_count());
}

// The whole resample for a candidate stream of at most kFusedWindow draws as one single-block launch
// (k_resample_block): draws, histogram tree and KLD stop, weights 1/M, updateConverged.  *handled = false when the
// stop lies beyond the window, a key does not fit the packing or the tree is too deep: the caller runs the general path.
int resample_block(bpf_engine* e, int window, bool systematic, const double* targets, ResampleOutcome* out,
                   bool* handled)
{
  *handled = false;
  SampleSet& a = e->sets[e->cur];
  SampleSet& b = e->sets[e->cur ^ 1];
  const auto kernel = kld_bins(e) ? k_resample_block_bins : k_resample_block;
  ResampleBlockArgs A{};
  H2D_OR_RETURN(fused_block_arm(e, kernel, window, systematic, &A));
  H2D_OR_RETURN(ensure_fused_jump(e));
  A.src = a.dev();
  A.n_src = e->sample_count;
  A.cdf = e->d_cdf.p;
  A.coarse_shift = fused_coarse_shift(A.n_src);
  A.coarse = (e->wc.cdf_coarse_n == A.n_src) ? e->d_cdf_coarse.p : nullptr;
  A.dst = b.dev();
  A.window = window;
  A.max_samples = e->max_samples;
  A.systematic = systematic ? 1 : 0;
  A.targets = targets;
  A.rng_state = e->rng;
  A.jump = e->d_fused_jump.p;
  A.keys = e->d_fused_keys.p;
  A.counter = e->d_fused_counter.p;
  A.miss_flag = e->d_flags.p;
  A.thr = e->dist_threshold;
  A.sc = e->d_scalars.p;
  A.conv_count = e->d_flags.p + 1;
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(window, kFusedDrawsPerBlock)), dim3(1024), kFusedLds, e->stream, A);
  }
  HIPCHK(e, hipGetLastError());
  int r5[5] = { 0, 0, 0, 0, 0 };
  H2D_OR_RETURN(fused_result_wait(e, A.generation, "k_resample_block", r5));
  const int* res = e->h_fused.p;  // (the debug stamps, [6] and [8 ..])
  if (debug_on())
  {
    fprintf(stderr, "[resample block] window %d M %d leaf %d bins %d status %d levels %d; last block (10 ns ticks): load %d "
            "dedup %d tree %d scan %d tail %d = %d shader clocks\n", window, r5[0], r5[1], r5[2], r5[3], r5[4],
            res[11] - res[9], res[12] - res[11], res[13] - res[12], res[14] - res[13], res[15] - res[14], res[6]);
    fprintf(stderr, "   block 0 draw phase (if it was not the last block): stage %d search %d gather+key %d fence %d\n",
            res[28] - res[20], res[29] - res[28], res[30] - res[29], res[31] - res[30]);
  }
  if (r5[3] != BPF_FUSED_OK)
    return BPF_OK;
  out->M = r5[0];
  out->counted(COUNTED_BY_BLOCK, kld_bins(e) ? r5[2] : r5[1], r5[2]);  // BINS mode: the leaf count IS the bin count
  out->windows = 1;
  *handled = true;
  return BPF_OK;
}

// ---- the KLD stop rule for a whole candidate stream [0, n) on the device, keys in e->d_keys (AoS).
// stop = the stop count (-1: no stop), leaf / bins at the final count; handled = false when the device declined (a key
// that does not fit the 64-bit packing, a tree deeper than the level budget): the caller replays on the host.
struct KldOutcome
{
  bool handled = false;
  int stop = -1, leaf = 0, bins = 0;

  void set(int stop_, int leaf_, int bins_)
  {
    handled = true;
    stop = stop_;
    leaf = leaf_;
    bins = bins_;
  }
};

// what one form of the device tree made of the stream
enum KldForm
{
  KLD_HANDLED,    // the outcome is filled in
  KLD_DECLINED,   // to the host replay
  KLD_NEXT_FORM,  // nothing decided: the driver goes on down its chain
};

constexpr int kKldMaxLevels = 256;  // the level budget; e->d_kld_flags and the pinned e->h_kld hold 4 + kKldMaxLevels flag words
// behind them in e->h_kld: the eight 64-bit result words of the pieces form, or the bins form's (never both in a call)
constexpr int kKldResultAt = 4 + kKldMaxLevels;
static_assert(kKldResultAt % 2 == 0, "the result words are 8-byte aligned");

// the buffers of a build over n keys and the arguments every kernel of it takes (`tree`: with the node arrays, which
// the bins form does without)
int kld_prepare(bpf_engine* e, int n, unsigned table, bool tree, KldArgs* K)
{
  HIPCHK(e, e->d_kld_hkey.reserve(table));
  HIPCHK(e, e->d_kld_htmin.reserve(table));
  HIPCHK(e, e->d_kld_slot.reserve((size_t)n));
  HIPCHK(e, e->d_kld_counts.reserve((size_t)n));
  HIPCHK(e, e->d_kld_flags.reserve(tree ? 4 + kKldMaxLevels : 4));
  HIPCHK(e, e->h_kld.reserve(kKldResultAt + 16));
  *K = KldArgs{};
  if (tree)
  {
    HIPCHK(e, e->d_kld_cur.reserve((size_t)n));
    HIPCHK(e, e->d_kld_first.reserve((size_t)n));
    HIPCHK(e, e->d_kld_child.reserve((size_t)2 * n));
    HIPCHK(e, e->d_kld_delta.reserve((size_t)n));
    HIPCHK(e, e->d_kld_tiles.reserve((size_t)blocks_for(n, kKldTile)));
    K->cur = e->d_kld_cur.p;
    K->first = e->d_kld_first.p;
    K->child = e->d_kld_child.p;
    K->delta = e->d_kld_delta.p;
  }
  K->keys = e->d_keys.p;
  K->n = n;
  K->h_key = e->d_kld_hkey.p;
  K->h_tmin = e->d_kld_htmin.p;
  K->h_mask = table - 1;
  K->slot = e->d_kld_slot.p;
  K->flags = e->d_kld_flags.p;
  K->limit = e->d_kld_limit.p;
  return BPF_OK;
}

// the look-back slots of the one-launch prefix scans (k_kld2_scan, k_kld_bins_scan), tagged with the generation:
// reserved and zeroed once
int kld_scan_slots(bpf_engine* e, int tiles)
{
  if (e->d_kld2_slots.cap < (size_t)tiles)
  {
    HIPCHK(e, e->d_kld2_slots.reserve((size_t)std::max(tiles, 1024)));
    HIPCHK(e, hipMemsetAsync(e->d_kld2_slots.p, 0, e->d_kld2_slots.cap * sizeof(unsigned long long), e->stream));
  }
  return BPF_OK;
}

// the tagged result words at e->h_kld + kKldResultAt: res[k] = word k for k = 1 .. count
int kld_result_wait(bpf_engine* e, int generation, int count, int* res, const char* kernel_name)
{
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(e->h_kld.p + kKldResultAt);
  return await_published(
      e, [&] { return tagged_words(words, 1, count, (unsigned)generation, res + 1); }, 100, kernel_name);
}

// BINS mode: the stop rule over the whole stream [0, n) with k = distinct keys so far (kernels_kld_bins.hpp): the key
// hash, then one look-back prefix count of the first occurrences with the stop test, and the result in pinned memory.
// leaf = bins in the outcome.
int kld_bins_on_device(bpf_engine* e, int n, bool whole_stream, KldOutcome* out)
{
  const unsigned table = hash_table_size(n);
  const int tiles = blocks_for(n, kKldTile);
  KldArgs K{};
  H2D_OR_RETURN(kld_prepare(e, n, table, false, &K));
  H2D_OR_RETURN(kld_scan_slots(e, tiles));
  int* counts = reinterpret_cast<int*>(e->d_kld_counts.p);
  e->kld_clean_table = 0;  // (the pieces form's start state is gone)
  e->kld_last_form = 4;
  e->kld_generation = next_generation(e->kld_generation);
  const int generation = e->kld_generation;
  ProfScope ps(e, BPF_K_DRAW);
  hipLaunchKernelGGL(k_kld_clear, dim3(std::min(1024, blocks_for((int)table, 256))), dim3(256), 0, e->stream, K, table,
                     4, 0);
  hipLaunchKernelGGL(k_kld_hash, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, K);
  hipLaunchKernelGGL(k_kld_bins_scan, dim3(tiles), dim3(256), 0, e->stream, K, e->d_kld2_slots.p, (unsigned)generation,
                     counts, K.flags + 3);
  hipLaunchKernelGGL(k_kld_bins_result, dim3(1), dim3(64), 0, e->stream, K, (const int*)counts,
                     (const int*)(K.flags + 3), whole_stream ? 1 : 0, e->h_kld.p + kKldResultAt, generation);
  HIPCHK(e, hipGetLastError());
  int res[5] = { 0, 0, 0, 0, 0 };
  H2D_OR_RETURN(kld_result_wait(e, generation, 4, res, "k_kld_bins_result"));
  if (debug_on())
    fprintf(stderr, "[kld bins] n %d key range %d stop %d bins %d status %d\n", n, res[1], res[2], res[3], res[4]);
  if (res[1] != 0 || res[4] != 0)
    return BPF_OK;  // a key outside the packing range, or a look-back that timed out: not handled (host replay)
  out->set(res[2], res[3], res[3]);
  return BPF_OK;
}

// One start of the tree forms' chain: the hash tables in their start state (the pieces form clears them behind its
// result while the host is turning around: `clean` then, and nothing to launch) and every key hashed
int kld_tree_begin(bpf_engine* e, const KldArgs& K, unsigned table, bool local)
{
  const bool clean = local && e->kld_clean_table == table && e->kld_clean_key == e->d_kld_hkey.p &&
                     e->kld_clean_tmin == e->d_kld_htmin.p && e->kld_clean_cap == e->d_kld_hkey.cap;
  e->kld_clean_table = 0;
  const dim3 clear_grid(std::min(1024, blocks_for((int)std::max<unsigned>(table, 2u * (unsigned)K.n), 256)));
  if (!clean)
    hipLaunchKernelGGL(k_kld_clear, clear_grid, dim3(256), 0, e->stream, K, table, 4 + kKldMaxLevels, local ? 0 : 1);
  hipLaunchKernelGGL(k_kld_hash, dim3(blocks_for(K.n, 256)), dim3(256), 0, e->stream, K);
  return BPF_OK;
}

// The whole stream in one resident round of 1024-thread blocks: the level loop, the prefix sums and the stop test run
// in ONE launch with grid barriers between the levels (k_kld_tree_persistent).  KLD_NEXT_FORM: the grid does not fit
// the device, or (e->kld_persistent cleared for the rest of the engine's life, and the stream drained) it did not
// become resident as a whole because the GPU is shared with another process.
int kld_tree_persistent(bpf_engine* e, const KldArgs& K, bool whole_stream, KldOutcome* out, KldForm* form)
{
  *form = KLD_NEXT_FORM;
  e->kld_last_form = 3;
  const int n = K.n, pgrid = blocks_for(n, kKldBlock);
  if (e->kld_persist_blocks_per_cu < 0)
  {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_kld_tree_persistent),
                                                     kKldBlock, 0) != hipSuccess)
      nb = 0;
    e->kld_persist_blocks_per_cu = nb;
  }
  if (pgrid > e->kld_persist_blocks_per_cu * e->n_cu)
    return BPF_OK;
  HIPCHK(e, e->d_kld_bar.reserve(4));
  HIPCHK(e, e->d_kld_tiles.reserve((size_t)std::max(pgrid, blocks_for(n, kKldTile))));
  HIPCHK(e, hipMemsetAsync(e->d_kld_bar.p, 0, 4 * sizeof(unsigned), e->stream));
  KldPersistArgs P{};
  P.K = K;
  P.bar = e->d_kld_bar.p;
  P.level_waiting = e->d_kld_flags.p + 4;
  P.tile_sums = e->d_kld_tiles.p;
  P.max_levels = kKldMaxLevels;
  P.whole_stream = whole_stream ? 1 : 0;
  P.timeout_ticks = 2000000ll;  // 20 ms per barrier: a resident grid passes one in microseconds
  P.result_host = e->h_kld.p;
  e->kld_generation = next_generation(e->kld_generation);
  P.generation = e->kld_generation;
  e->h_kld.p[0] = 0;  // (the level-per-launch form copies its flag words here)
  hipLaunchKernelGGL(k_kld_tree_persistent, dim3(pgrid), dim3(kKldBlock), 0, e->stream, P);
  HIPCHK(e, hipGetLastError());
  H2D_OR_RETURN(await_published(
      e, [&] { return __atomic_load_n(e->h_kld.p, __ATOMIC_ACQUIRE) == P.generation; }, 200, "k_kld_tree_persistent"));
  const int* res = e->h_kld.p;
  if (debug_on())
    fprintf(stderr, "[kld persistent] n %d blocks %d stop %d leaf %d bins %d status %d levels %d\n", n, pgrid, res[1],
            res[2], res[3], res[4], res[5]);
  if (res[4] == BPF_KLD_PERSIST_OK)
  {
    out->set(res[1], res[2], res[3]);
    *form = KLD_HANDLED;
  }
  else if (res[4] != BPF_KLD_PERSIST_TIMEOUT)
    *form = KLD_DECLINED;  // a key outside the packing, or deeper than the level budget
  else
  {
    // let the launch drain and leave this form alone from now on
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->kld_persistent = false;
  }
  return BPF_OK;
}

// The tree in LDS-sized pieces (kernels_kld2.hpp): no level loop, no host round trip until the result.
// KLD_NEXT_FORM: a bucket that does not fit a block, or a piece deeper than its budget.
int kld_tree_pieces(bpf_engine* e, const KldArgs& K, unsigned table, bool whole_stream, KldOutcome* out, KldForm* form)
{
  *form = KLD_DECLINED;
  e->kld_last_form = 2;
  const int n = K.n;
  const size_t nn = (size_t)n;
  const int n_tiles = blocks_for(n, 256), tiles = blocks_for(n, kKldTile);
  HIPCHK(e, e->d_kld2_int.reserve(5 * nn + 3 * (size_t)kKld2Nodes + 8 + (size_t)n_tiles));
  HIPCHK(e, e->d_kld2_top.reserve((size_t)kKld2Nodes));
  H2D_OR_RETURN(ensure_dynamic_lds(e, &k_kld2_top, kKld2LdsBytes));
  H2D_OR_RETURN(ensure_dynamic_lds(e, &k_kld2_subtrees, kKld2LdsBytes));
  Kld2Args L{};
  L.K = K;
  L.pk = reinterpret_cast<unsigned long long*>(e->d_kld2_int.p);  // first: 8-byte aligned
  int* base = e->d_kld2_int.p + 2 * nn;
  L.tkeys = base;
  L.bucket = base + nn;
  L.bk = base + 2 * nn;
  L.cnt = base + 3 * nn;
  L.off = L.cnt + kKld2Nodes;
  L.fill = L.off + kKld2Nodes + 1;
  L.n_tkeys = L.fill + kKld2Nodes;
  L.n_top = L.n_tkeys + 1;
  L.status = L.n_top + 1;
  int* tile_first = L.status + 4;
  L.tile_first = tile_first;
  L.n_tiles = n_tiles;
  L.top = e->d_kld2_top.p;
  L.counts = e->d_kld_counts.p;
  L.whole_stream = whole_stream ? 1 : 0;
  e->kld_generation = next_generation(e->kld_generation);
  L.generation = e->kld_generation;
  L.result_host = e->h_kld.p + kKldResultAt;
  hipLaunchKernelGGL(k_kld2_init, dim3(n_tiles), dim3(256), 0, e->stream, K, tile_first);
  hipLaunchKernelGGL(k_kld2_compact, dim3(n_tiles), dim3(256), 0, e->stream, L);
  hipLaunchKernelGGL(k_kld2_top, dim3(1), dim3(kKld2Block), kKld2LdsBytes, e->stream, L);
  hipLaunchKernelGGL(k_kld2_route, dim3(blocks_for(n, kKld2Block)), dim3(kKld2Block), 0, e->stream, L);
  hipLaunchKernelGGL(k_kld2_offsets, dim3(1), dim3(1024), 0, e->stream, L);
  hipLaunchKernelGGL(k_kld2_scatter, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, L);
  hipLaunchKernelGGL(k_kld2_subtrees, dim3(blocks_for(n, kKld2Span) + 1), dim3(kKld2Block), kKld2LdsBytes, e->stream,
                     L);
  // prefix sums + stop test in one launch
  H2D_OR_RETURN(kld_scan_slots(e, tiles));
  hipLaunchKernelGGL(k_kld2_scan, dim3(tiles), dim3(256), 0, e->stream, K, e->d_kld2_slots.p,
                     (unsigned)L.generation, e->d_kld_counts.p, L.status);
  hipLaunchKernelGGL(k_kld2_result, dim3(1), dim3(64), 0, e->stream, L);
  // the next build's start state now, behind the result: the GPU does it while this thread turns around
  hipLaunchKernelGGL(k_kld_clear, dim3(std::min(1024, blocks_for((int)table, 256))), dim3(256), 0, e->stream, K, table,
                     4 + kKldMaxLevels, 0);
  HIPCHK(e, hipGetLastError());
  // the result block in pinned memory, every word tagged with the generation: one poll instead of three copies
  // with a stream synchronisation each
  int res[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  H2D_OR_RETURN(kld_result_wait(e, L.generation, 7, res, "k_kld2_result"));
  if (debug_on())
    fprintf(stderr, "[kld pieces] n %d tree keys %d status %d largest bucket %d stop %d leaf %d bins %d\n", n, res[6],
            res[5], res[7], res[2], res[3], res[4]);
  e->kld_clean_table = table;
  e->kld_clean_key = e->d_kld_hkey.p;
  e->kld_clean_tmin = e->d_kld_htmin.p;
  e->kld_clean_cap = e->d_kld_hkey.cap;
  if (res[1] != 0)
    return BPF_OK;  // a key outside the packing range
  if (res[5] != BPF_KLD2_OK)
  {
    *form = KLD_NEXT_FORM;
    return BPF_OK;
  }
  out->set(res[2], res[3], res[4]);
  *form = KLD_HANDLED;
  return BPF_OK;
}

// The tree grown level by level, a launch pair per level and a look at the flag words per batch of levels, then the
// scan of the leaf count.  The last form of the chain: the outcome stays unhandled when a key does not fit the packing
// or the tree is deeper than the level budget.
int kld_tree_levels(bpf_engine* e, const KldArgs& K, bool whole_stream, KldOutcome* out)
{
  e->kld_last_form = 1;
  const int n = K.n, tiles = blocks_for(n, kKldTile);
  hipLaunchKernelGGL(k_kld_init, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, K);
  hipLaunchKernelGGL(k_kld_root_first, dim3(1), dim3(1024), 0, e->stream, K);
  int level = 0;
  bool done = false;
  int batch = std::min(24, (int)std::ceil(1.3 * std::log2((double)n + 1.0)) + 1);  // (see below)
  while (!done && level < kKldMaxLevels)
  {
    for (int q = 0; q < batch && level < kKldMaxLevels; ++q, ++level)
    {
      hipLaunchKernelGGL(k_kld_children, dim3(blocks_for(n, kKldBlock)), dim3(kKldBlock), 0, e->stream, K);
      hipLaunchKernelGGL(k_kld_descend, dim3(blocks_for(n, kKldBlock)), dim3(kKldBlock), 0, e->stream, K,
                         e->d_kld_flags.p + 4 + level);
    }
    HIPCHK(e, hipGetLastError());
    H2D_OR_RETURN(pinned_down_sync(e, e->h_kld, 0, e->d_kld_flags, 0, 4 + kKldMaxLevels, e->stream));
    if (e->h_kld.p[0] != 0)
      return BPF_OK;  // a key outside the packing range: not handled
    const int waiting = e->h_kld.p[4 + level - 1];  // keys that are not nodes yet
    done = waiting == 0;
    if (done)
      break;
    // A random-order tree of K keys is ~2.5 log2 K levels deep and the count of waiting keys falls faster and faster
    // near the end: ~1.3 log2(waiting) more levels finish it (measured on 59 k and 97 k keys).  (One block taking over
    // the last few thousand keys was tried: a level is ~6 dependent round trips to first[] / child[] either way, 8 us
    // in one block against 14 us as a launch pair, and the switch costs what it saves.)
    batch = std::min(24, (int)std::ceil(1.3 * std::log2((double)waiting + 1.0)) + 1);
  }
  if (debug_on())
  {
    fprintf(stderr, "[kld device] n %d levels %d done %d; keys waiting after each level:", n, level, (int)done);
    for (int l = 0; l < level; ++l)
      fprintf(stderr, " %d", e->h_kld.p[4 + l]);
    fprintf(stderr, "\n");
  }
  if (!done)
    return BPF_OK;  // deeper than the level budget: not handled
  hipLaunchKernelGGL(k_kld_scan_tiles, dim3(tiles), dim3(256), 0, e->stream, (const int2*)e->d_kld_delta.p, n,
                     e->d_kld_tiles.p);
  hipLaunchKernelGGL(k_kld_scan_offsets, dim3(1), dim3(1024), 0, e->stream, e->d_kld_tiles.p, tiles);
  hipLaunchKernelGGL(k_kld_scan_final, dim3(tiles), dim3(256), 0, e->stream, K, (const int2*)e->d_kld_tiles.p,
                     e->d_kld_counts.p);
  HIPCHK(e, hipGetLastError());
  H2D_OR_RETURN(pinned_down_sync(e, e->h_kld, 0, e->d_kld_flags, 0, 4, e->stream));
  const int stop = whole_stream ? -1 : e->h_kld.p[2];  // whole_stream: the tree of all n keys, no stop rule
  const int M = (stop >= 1 && stop <= n) ? stop : n;
  int2 c;
  H2D_OR_RETURN(small_down_sync(e, &c, (const int2*)e->d_kld_counts.p + (M - 1), 1, e->stream));
  out->set((stop >= 1 && stop <= n) ? stop : -1, c.x, c.y);
  return BPF_OK;
}

// The driver.  BINS mode has one form.  Otherwise the chain is: the persistent form (BPF_OPT_KLD_PERSISTENT), the
// pieces (BPF_OPT_KLD_LOCAL), the level loop; a form that hands on leaves the tables used, so the chain starts again
// with them (kld_tree_begin), in a ProfScope of its own inside the one before it.
int kld_tree_on_device(bpf_engine* e, int n, KldOutcome* out, bool whole_stream = false)
{
  *out = KldOutcome{};
  if (n >= (1 << 30))
    return BPF_OK;  // element indices 2v + side are folded as 32-bit tags
  H2D_OR_RETURN(ensure_limit_table(e, n));
  if (kld_bins(e))
    return kld_bins_on_device(e, n, whole_stream, out);
  const unsigned table = hash_table_size(n);
  KldArgs K{};
  H2D_OR_RETURN(kld_prepare(e, n, table, true, &K));
  KldForm form = KLD_NEXT_FORM;
  bool local = e->kld_local && !e->kld_persistent;
  ProfScope ps(e, BPF_K_DRAW);
  std::optional<ProfScope> ps_again, ps_levels;
  H2D_OR_RETURN(kld_tree_begin(e, K, table, local));
  if (e->kld_persistent)
  {
    H2D_OR_RETURN(kld_tree_persistent(e, K, whole_stream, out, &form));
    if (form != KLD_NEXT_FORM)
      return BPF_OK;
    if (!e->kld_persistent)
    {
      // it timed out and is out of the way for good: from the top without it.  (A grid that merely does not fit goes
      // on to the level loop: the option is still set, and it keeps the pieces out.)
      local = e->kld_local;
      ps_again.emplace(e, BPF_K_DRAW);
      H2D_OR_RETURN(kld_tree_begin(e, K, table, local));
    }
  }
  if (local)
  {
    H2D_OR_RETURN(kld_tree_pieces(e, K, table, whole_stream, out, &form));
    if (form != KLD_NEXT_FORM)
      return BPF_OK;
    ps_levels.emplace(e, BPF_K_DRAW);
    H2D_OR_RETURN(kld_tree_begin(e, K, table, false));
  }
  return kld_tree_levels(e, K, whole_stream, out);
}

// the whole candidate stream [0, maxs) again with the keys on the device only, then the tree
int kld_on_device(bpf_engine* e, DrawArgs A, int maxs, KldOutcome* out)
{
  A.m0 = 0;
  A.m1 = maxs;
  A.host_keys = nullptr;
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_draw_select, dim3(blocks_for(maxs, 256)), dim3(256), 0, e->stream, A);
  }
  return kld_tree_on_device(e, maxs, out);
}

// Spin on the generation word a kernel publishes in pinned host memory (kernels of ~10 us); false if it
// takes implausibly long, and the caller falls back to a copy or a stream synchronisation.
bool wait_generation(bpf_engine* e, unsigned generation)
{
  return spin_until([&] { return __atomic_load_n(e->h_done.p, __ATOMIC_ACQUIRE) == generation; }, 20);
}

// ---- the resamplers' keys on their way to the ordered host replay
// Zero-copy hand-off (DrawArgs, SystematicArgs): the kernel writes the keys of its n draws straight into pinned host
// memory as three rows and its last block publishes a generation number there (wait_generation), so that the host
// polls a word instead of paying for a copy plus a stream synchronisation.
template <class Args>
void arm_key_handoff(bpf_engine* e, int n, Args* A)
{
  A->host_keys = e->h_keys.p;
  A->host_stride = n;
  A->done_counter = reinterpret_cast<unsigned*>(e->d_flags.p + 4);
  A->host_done = reinterpret_cast<volatile unsigned*>(e->h_done.p);
  A->generation = ++e->done_generation;
}

// the keys of n draws in e->h_keys: three rows of `stride` (the zero-copy hand-off), or AoS triples (stride 0)
struct KeyView
{
  const int* keys;
  int stride;

  int key(int o, int d) const
  {
    return stride ? keys[(size_t)d * stride + o] : keys[3 * (size_t)o + d];
  }
};

// the AoS triples the kernel left in e->d_keys, copied
int copy_key_triples(bpf_engine* e, int n, KeyView* view)
{
  H2D_OR_RETURN(pinned_down_sync(e, e->h_keys, 0, e->d_keys, 0, (size_t)n * 3, e->stream));
  *view = KeyView{ e->h_keys.p, 0 };
  return BPF_OK;
}

// The ordered replay's stop test (particle_filter.cpp:409-417): the bound follows the stop rule's k, recomputed when k
// changes
struct KldReplay
{
  int leaf = -1, limit = 0;

  // the key of draw number `count` (1-based); true when the set is complete with it
  bool feed(bpf_engine* e, int x, int y, int t, int count)
  {
    if (kld_host_insert(e, x, y, t) || leaf < 0)
    {
      const int lc = kld_host_k(e);
      if (lc != leaf)
      {
        leaf = lc;
        limit = resample_limit(lc, e->min_samples, e->max_samples, e->pop_err, e->pop_z);
      }
    }
    return count > limit;  // particle_filter.cpp:416
  }
};

// ---- the drand48 stream behind a resample that kept M samples (resample_plan.hpp: stream_consumed), with the one
// read-back of the draw chain's word: *state48_out = state0 advanced by what the resample consumed
int stream_after_resample(bpf_engine* e, uint64_t state0, const StreamUse& use, int M, uint64_t* state48_out)
{
  int chain_word = 0;
  if (use.regime == STREAM_MULTINOMIAL_CHAIN)
  {
    HIPCHK(e, e->h_chain_word.reserve(1));
    H2D_OR_RETURN(pinned_down_sync(e, e->h_chain_word, 0, e->d_chain, (size_t)(M - 1), 1, e->stream));
    chain_word = e->h_chain_word.p[0];
  }
  *state48_out = lcg_skip_host(state0, stream_consumed(use, M, chain_word), e->jump);
  return BPF_OK;
}

// ---- the multinomial resampler (particle_filter.cpp:357-420)
// w_diff > 0 (:383-388): every draw first tests a uniform against w_diff; where each draw finds its stream elements
// is resolved up front for all candidate draws, into e->d_chain
struct RecoveryDraws
{
  FreeSpaceDev free_space{};
  const int* chain = nullptr;
};

int multinomial_recovery_chain(bpf_engine* e, double w_diff, RecoveryDraws* R)
{
  int rc = ensure_free_space(e, &R->free_space);
  if (rc != BPF_OK)
    return rc;
  rc = pose_check_scored(e) ? resolve_scored_chain(e, R->free_space, w_diff, e->max_samples)
                            : build_draw_chain(e, w_diff, e->max_samples, R->free_space.retries);
  if (rc != BPF_OK)
    return rc;
  R->chain = e->d_chain.p;
  return BPF_OK;
}

// The single engine's tracking predicate: the previous cycle's stop (+ 25 %) fits one block's window (*w0, the first
// window BEFORE the schedule's cap at 4096), no recovery draws are due and no long stream is expected.  (The sharded
// driver's differs: shard_tracking in abi_mailbox_step.inl.)
bool multinomial_tracking(const bpf_engine* e, double w_diff, int* w0)
{
  const int maxs = e->max_samples;
  *w0 = std::min(std::max(1024, std::min(e->window_hint, maxs)), maxs);
  const bool long_stream0 = e->window_hint >= maxs && maxs >= e->kld_device_min;
  return e->fused_resample && w_diff == 0.0 && *w0 <= kFusedWindow && !long_stream0;
}

// the arguments of a draw window, all but the window itself
DrawArgs multinomial_draw_args(bpf_engine* e, const RecoveryDraws& R)
{
  DrawArgs A{};
  A.src = e->sets[e->cur].dev();
  A.n_src = e->sample_count;
  A.cdf = e->d_cdf.p;
  A.dst = e->sets[e->cur ^ 1].dev();
  A.rng_state = e->rng;
  A.jump = e->jump;
  A.keys = e->d_keys.p;
  A.src_index = e->d_src_index.p;
  A.miss_flag = e->d_flags.p;
  A.sharded = 0;
  A.chain = R.chain;
  A.free_space = R.free_space;
  A.guide = e->wc.cdf_guide_valid ? e->d_cdf_guide.p : nullptr;
  return A;
}

// No stop so far and a long stream ahead (a spread cloud): the ordered replay moves to the device for the whole
// stream.  *handled = false: key range or depth outside what the device tree takes, host replay as before.
int multinomial_device_stream(bpf_engine* e, const DrawArgs& A, ResampleOutcome* out, int* stop, bool* handled)
{
  KldOutcome dev;
  int rc = kld_on_device(e, A, e->max_samples, &dev);
  if (rc != BPF_OK)
    return rc;
  *handled = dev.handled;
  if (dev.handled)
  {
    out->windows++;
    *stop = dev.stop;
    out->counted(COUNTED_BY_DEVICE_TREE, dev.leaf, dev.bins);
  }
  return BPF_OK;
}

// One window [m0, m1) replayed on the host: the draws, their keys through the zero-copy hand-off or a copy, and the
// ordered insertion with the stop test; *stop = the stop count when the window held it
int multinomial_host_window(bpf_engine* e, DrawArgs A, int m0, int m1, KldReplay* replay, int* stop)
{
  A.m0 = m0;
  A.m1 = m1;
  const int wn = m1 - m0;
  const bool zero_copy = e->zero_copy_keys && wn <= (1 << 20);
  if (zero_copy)
    arm_key_handoff(e, wn, &A);
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_draw_select, dim3(blocks_for(wn, 256)), dim3(256), 0, e->stream, A);
  }
  HIPCHK(e, hipGetLastError());
  KeyView keys{ e->h_keys.p, wn };
  if (!(zero_copy && wait_generation(e, A.generation)))
    H2D_OR_RETURN(copy_key_triples(e, wn, &keys));  // (the kernel writes e->d_keys either way)
  for (int m = m0; m < m1 && *stop < 0; ++m)
    if (replay->feed(e, keys.key(m - m0, 0), keys.key(m - m0, 1), keys.key(m - m0, 2), m + 1))
      *stop = m + 1;
  return BPF_OK;
}

// The general path: windows of candidate draws by the schedule of resample_plan.hpp, replayed on the host in order
// until the stop rule ends the stream, or the whole stream handed to the device tree
int multinomial_windows(bpf_engine* e, const RecoveryDraws& R, ResampleOutcome* out)
{
  const int maxs = e->max_samples;
  HIPCHK(e, e->d_keys.reserve((size_t)maxs * 3));
  HIPCHK(e, e->d_src_index.reserve((size_t)maxs));
  HIPCHK(e, e->h_keys.reserve((size_t)maxs * 3));
  kld_host_reset(e, std::min(maxs, 1 << 20));
  const DrawArgs A = multinomial_draw_args(e, R);
  // whole_stream_at_start: a previous cycle that ran to the end sends this one to the device tree at once
  WindowSchedule s = window_schedule(e->window_hint, maxs, e->kld_device_min, true);
  KldReplay replay;
  int stop = -1;
  bool on_device = false;
  out->windows = 0;
  while (s.m0 < maxs && stop < 0 && !on_device)
  {
    if (s.whole_stream_due(replay.limit))
    {
      H2D_OR_RETURN(multinomial_device_stream(e, A, out, &stop, &on_device));
      if (on_device)
        break;
      s.device_declined = true;
    }
    H2D_OR_RETURN(multinomial_host_window(e, A, s.m0, s.m1(), &replay, &stop));
    out->windows++;
    s.next(replay.limit);
  }
  out->M = (stop > 0) ? stop : maxs;
  // the window that found the stop also inserted nothing past it: hist is exactly set b's tree
  if (!on_device)
    counted_by_host_tree(e, out);
  return BPF_OK;
}

int resample_multinomial(bpf_engine* e, double w_diff, ResampleOutcome* out)
{
  const uint64_t rng0 = e->rng;
  RecoveryDraws recovery;
  StreamUse stream;
  if (w_diff > 0.0)
  {
    H2D_OR_RETURN(multinomial_recovery_chain(e, w_diff, &recovery));
    stream.regime = STREAM_MULTINOMIAL_CHAIN;
  }
  int w0 = 0;
  bool tracked = false;
  if (multinomial_tracking(e, w_diff, &w0))
    H2D_OR_RETURN(resample_block(e, w0, false, nullptr, out, &tracked));
  if (!tracked)
    H2D_OR_RETURN(multinomial_windows(e, recovery, out));
  e->window_hint = resample_window_for(out->M);
  return stream_after_resample(e, rng0, stream, out->M, &e->rng);
}

// ---- the systematic resampler (particle_filter.cpp:269-355)
// The targets in e->h_targets: the serial chain of resample_plan.hpp from the stream state behind the systematic
// start.  A CPU core runs that dependency chain several times faster than a GPU lane, with the same IEEE arithmetic,
// so the host forms the targets and the kernel reads them from pinned memory.  A window kernel of the sharded filter
// may still be reading the previous ones (systematic_targets_in_use; no event on an engine that never ran sharded).
int systematic_targets(bpf_engine* e, uint64_t start_state48, int count, int num_systematic)
{
  HIPCHK(e, e->h_targets.reserve((size_t)std::max(count, e->max_samples)));
  if (e->targets_read)
    HIPCHK(e, hipEventSynchronize(e->targets_read));
  systematic_target_chain(std::ldexp((double)start_state48, -48), num_systematic, e->h_targets.p);
  return BPF_OK;
}

// The sample budget for a set of `leaf_count` leaves (resample_plan.hpp), with the free-space list when random pose
// calls are due; calls that are not resolved by score must fit 31-bit stream positions
int systematic_budget_for(bpf_engine* e, int leaf_count, double w_diff, SystematicBudget* B, FreeSpaceDev* free_space)
{
  *B = systematic_budget(resample_limit(leaf_count, e->min_samples, e->max_samples, e->pop_err, e->pop_z), w_diff,
                         e->max_samples);
  if (B->n_random <= 0)
    return BPF_OK;
  int rc = ensure_free_space(e, free_space);
  if (rc != BPF_OK)
    return rc;
  if (!pose_check_scored(e) && !random_calls_fit(free_space->retries, B->n_random))
    return e->fail(BPF_ERR_CAPACITY, "random pose calls would pass 31-bit stream positions");
  return BPF_OK;
}

struct SystematicPlan
{
  SystematicBudget budget;
  SystematicArgs A{};  // all but the targets and the key hand-off
  StreamUse stream;
};

// budget, random pose calls, buffers, targets and the kernel arguments; e->rng stands behind the systematic start
int systematic_plan(bpf_engine* e, double w_diff, SystematicPlan* P)
{
  FreeSpaceDev free_space{};
  P->stream.regime = STREAM_SYSTEMATIC;
  H2D_OR_RETURN(systematic_budget_for(e, e->tree.leaf_count, w_diff, &P->budget, &free_space));
  const int count = P->budget.count, num_random = P->budget.n_random;
  P->stream.retries = free_space.retries;
  P->stream.n_random = num_random;
  if (num_random > 0 && pose_check_scored(e))
  {
    H2D_OR_RETURN(resolve_scored_calls(e, free_space, e->rng, 2, num_random, &P->stream.scored_end));
    free_space.accept = e->d_accept.p;
    P->stream.regime = STREAM_SYSTEMATIC_SCORED;
  }
  const uint64_t rng_before = e->rng;
  e->rng = lcg_skip_host(e->rng, 1, e->jump);
  HIPCHK(e, e->d_keys.reserve((size_t)e->max_samples * 3));
  HIPCHK(e, e->d_src_index.reserve((size_t)e->max_samples));
  HIPCHK(e, e->h_keys.reserve((size_t)e->max_samples * 3));
  SystematicArgs& A = P->A;
  A.src = e->sets[e->cur].dev();
  A.n_src = e->sample_count;
  A.cdf = e->d_cdf.p;
  A.dst = e->sets[e->cur ^ 1].dev();
  A.count = count;
  A.n_random = num_random;
  A.rng_state = rng_before;
  A.jump = e->jump;
  A.free_space = free_space;
  A.keys = e->d_keys.p;
  A.src_index = e->d_src_index.p;
  A.miss_flag = e->d_flags.p;
  return systematic_targets(e, e->rng, count, count - num_random);
}

// The general path: the kernel reads the targets straight from the pinned buffer (28 KB for 3.5 k samples) and, like
// the multinomial draw kernel, leaves the keys in pinned memory behind a generation word -- or, for a large set in
// BINS mode, in e->d_keys, where the device counts the new set's distinct keys (the key hash and one scan)
int systematic_select_and_count(bpf_engine* e, SystematicArgs A, ResampleOutcome* out)
{
  const int count = A.count;
  A.targets = e->h_targets.p;
  const bool device_count = kld_bins(e) && count >= 8192;
  const bool zero_copy = e->zero_copy_keys && count <= (1 << 20) && !device_count;
  if (zero_copy)
    arm_key_handoff(e, count, &A);
  {
    ProfScope ps(e, BPF_K_DRAW);
    hipLaunchKernelGGL(k_systematic_select, dim3(blocks_for(count, 256)), dim3(256), 0, e->stream, A);
  }
  HIPCHK(e, hipGetLastError());
  KldOutcome dev;
  if (device_count)
    H2D_OR_RETURN(kld_tree_on_device(e, count, &dev, true));
  if (dev.handled)
    out->counted(COUNTED_BY_DEVICE_TREE, dev.bins, dev.bins);
  else
  {
    KeyView keys{ e->h_keys.p, count };
    if (!zero_copy)
      H2D_OR_RETURN(copy_key_triples(e, count, &keys));
    else if (!wait_generation(e, A.generation))
      HIPCHK(e, hipStreamSynchronize(e->stream));  // the kernel wrote only the host rows; wait for it the slow way
    kld_host_reset(e, std::min(count, 1 << 20));
    for (int m = 0; m < count; ++m)
      kld_host_insert(e, keys.key(m, 0), keys.key(m, 1), keys.key(m, 2));
    counted_by_host_tree(e, out);
  }
  out->M = count;
  out->windows = 1;
  return BPF_OK;
}

int resample_systematic(bpf_engine* e, double w_diff, ResampleOutcome* out)
{
  SystematicPlan P;
  H2D_OR_RETURN(systematic_plan(e, w_diff, &P));
  bool handled = false;
  // the whole resample as one launch (k_resample_block): selection, the new set's histogram tree, weights,
  // updateConverged; the targets are read straight from the pinned buffer
  if (e->fused_resample && P.budget.n_random == 0 && P.budget.count <= kFusedWindow)
    H2D_OR_RETURN(resample_block(e, P.budget.count, true, e->h_targets.p, out, &handled));
  if (!handled)
    H2D_OR_RETURN(systematic_select_and_count(e, P.A, out));
  // :316-324: the random pose calls took their uniforms right after the systematic start
  return stream_after_resample(e, P.A.rng_state, P.stream, out->M, &e->rng);
}

int upload_samples(bpf_engine* e, const double* aos, int n, SampleSet& dst)
{
  HIPCHK(e, e->d_aos.reserve((size_t)n));
  HIPCHK(e, dst.reserve((size_t)n));
  // the caller's buffer goes up the way h2d_from_host decides: through the engine's pinned bounce buffer, piece by
  // piece, unless it is registered or BPF_OPT_HOST_DIRECT_PAGEABLE hands pageable memory to the runtime as it is
  H2D_OR_RETURN(h2d_from_host(e, e->d_aos.p, aos, (size_t)n * sizeof(double4), e->stream));
  hipLaunchKernelGGL(k_aos_to_soa, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->d_aos.p, dst.dev(), n);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}

// the weights of a device-side set back into the caller's AoS records (only the weight of a record changes in a
// sensor update): 8 bytes per particle over PCIe instead of 32, no re-interleaving launch
int download_weights(bpf_engine* e, const SampleSet& src, int n, double* aos)
{
  HIPCHK(e, e->h_aos.reserve((size_t)n));
  const double* hw = reinterpret_cast<const double*>(e->h_aos.p);  // the staging buffer lent out as n doubles
  H2D_OR_RETURN(pinned_down(e, e->h_aos, 0, src.w, 0, (size_t)n, e->stream));
  H2D_OR_RETURN(pinned_down_sync(e, e->h_scalars, 0, e->d_scalars, 0, 1, e->stream));
  for (int i = 0; i < n; ++i)
    aos[4 * (size_t)i + 3] = hw[i];
  return BPF_OK;
}
