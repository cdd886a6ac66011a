// C-ABI: exhaustive pose search with the 3-D map and the cloud scanner (include/badger_pf.h) -- every column of the
// map's rectangle (Node3D::updateFreeSpaceIndices) x heading scored against one cloud on the device, the best k kept.
// The columns are rectangle arithmetic (SearchSpace's rectangle form), never a list.  The cloud and the term table are
// staged ONCE (stage_cloud, abi_cloud3d.inl: the one stream wait of the call before its launches); every window is then
// k_search_candidates, launch_cloud on the engine's candidate set -- so a score is by construction what
// bpf_cloud_apply_model_to_sample_set gives the sample {pose, 1.0} --, k_search_select and k_search_merge, enqueued
// behind the window before.  All scratch is reserved for the first (largest) window, so no window reallocates; this
// thread waits a second time for the k rows and never per window.
//
// Read-only for the filter: what the scoring launches write that describes the engine's last scoring call
// (evals_last, last_cloud_form, the profiling slots) and last_status are put back on every path.
namespace
{
// ceil(a / s) * s for s >= 1 and a of either sign (the division truncates towards zero: a ceiling for a <= 0 already)
long long first_multiple_at_or_above(long long a, long long s)
{
  return (a / s + (a % s > 0 ? 1 : 0)) * s;
}

// arguments every entry point checks alike
int cloud_search_space_of(bpf_engine* e, int headings, int cell_stride, SearchSpace* S, long long* total)
{
  if (headings < 1 || cell_stride < 1)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: headings >= 1 and cell_stride >= 1 are needed");
  if (!e->have_map3d)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "cloud pose search needs the 3-D map (bpf_map3d_set)");
  const Map3dDev& M = e->map3;
  const long long s = cell_stride;
  // the columns min <= c < max of either axis (node_3d.cpp:306-318) that the stride divides
  const long long i0 = first_multiple_at_or_above(M.min_c[0], s), j0 = first_multiple_at_or_above(M.min_c[1], s);
  const long long n_i = i0 < M.max_c[0] ? (M.max_c[0] - 1 - i0) / s + 1 : 0;
  const long long n_j = j0 < M.max_c[1] ? (M.max_c[1] - 1 - j0) / s + 1 : 0;
  *S = SearchSpace{};
  S->cells = nullptr;
  S->n_cells = (int)(n_i * n_j);  // <= n_pose_indices < 2^30 (bpf_map3d_set)
  S->headings = headings;
  S->resolution = M.resolution;
  S->i0 = (int)i0;
  S->j0 = (int)j0;
  S->n_j = (int)n_j;
  S->stride = cell_stride;
  *total = n_i * n_j * (long long)headings;
  return BPF_OK;
}

int cloud_search_poses(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                       long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out,
                       SearchShard* sh = nullptr)
{
  if (!hits_out || !n_hits_out || !points_xyz || n_points <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: a cloud and an output are needed");
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  SearchSpace S;
  long long total = 0;
  int rc = cloud_search_space_of(e, headings, cell_stride, &S, &total);
  if (rc != BPF_OK)
    return rc;
  if (!e->cloud_configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the point-cloud model: none is set");
  if (total > 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "pose search: more than 2^31 - 1 candidates (raise cell_stride or lower headings)");
  if (first < 0 || first > total || count < -1 || (count >= 0 && count > total - first))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: first / count outside the candidate space");
  if (count < 0)
    count = total - first;
  *n_hits_out = 0;
  if (sh)  // (an empty share scores nothing and contributes an empty list)
    shard_search_share(sh->rank, sh->world, first, count, &first, &count);
  else if (count == 0)
    return BPF_OK;
  HIPCHK(e, hipSetDevice(e->device));

  const bool scored = e->cloud_max_beams >= 2;  // (below that applyModelToSampleSet leaves the weight 1.0, :109-110)
  const int n_max = (int)std::max<long long>(1, std::min<long long>(count, kSearchWindow));
  if (scored)
  {
    rc = stage_cloud(e, points_xyz, n_points);  // (waits for the stream: nothing below frees a buffer in use)
    if (rc != BPF_OK)
      return rc;
    HIPCHK(e, e->d_affine.reserve((size_t)n_max * 12));
    HIPCHK(e, e->d_cloud_partials.reserve((size_t)blocks_for(n_points, kCloudChunk) * n_max));
  }
  HIPCHK(e, e->cand.reserve((size_t)n_max));
  rc = search_begin(e);
  if (rc != BPF_OK)
    return rc;
  // from the first launch on, a failure returns with the stream drained
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  for (long long done = 0; done < count; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(count - done, kSearchWindow);
    const long long c0 = first + done;
    hipLaunchKernelGGL(k_search_candidates, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(), n, c0, S);
    if (hipGetLastError() != hipSuccess)
      return drained(e->fail(BPF_ERR_HIP, "k_search_candidates launch"));
    if (scored)
    {
      rc = launch_cloud(e, e->cand.dev(), n, n_points);
      if (rc != BPF_OK)
        return drained(rc);
    }
    rc = search_fold_window(e, n, c0, k);
    if (rc != BPF_OK)
      return drained(rc);
  }
  rc = sh ? shard_search_finish(e, sh, S, k, hits_out, n_hits_out) : search_finish(e, S, k, hits_out, n_hits_out);
  return rc == BPF_OK ? rc : drained(rc);
}
}  // namespace

int bpf_cloud_search_space(bpf_engine* e, int headings, int cell_stride, long long* candidates_out, int* columns_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  SearchSpace S;
  long long total = 0;
  const int rc = cloud_search_space_of(e, headings, cell_stride, &S, &total);
  e->last_status = status;
  if (rc != BPF_OK)
    return rc;
  if (candidates_out)
    *candidates_out = total;
  if (columns_out)
    *columns_out = S.n_cells;
  return BPF_OK;
}

int bpf_cloud_search_poses(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                           long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // what the scoring launches reset describes the engine's last scoring call, not the candidates: put back, whatever
  // the outcome.  Profiling is off for the call, so no event slot is taken and the stride of timed launches stays.
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_cloud_form;
  const bool profiling = e->profiling;
  e->profiling = false;
  const int rc = cloud_search_poses(e, points_xyz, n_points, headings, cell_stride, first, count, k, hits_out,
                                    n_hits_out);
  e->profiling = profiling;
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_cloud_form = form;
  return rc;
}
