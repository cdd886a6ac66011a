// C-ABI: joint pose search (include/badger_pf.h) -- every candidate of the exhaustive search scored against S scans,
// scan s taken at the candidate's base pose composed with the rigid offset D_s, the weight carried from scan to scan as
// the filter carries it; the best k kept.  Built on abi_pose_search.inl and abi_pose_search_cloud.inl: the space, the
// numbering, the selection (search_begin / search_fold_window / search_finish) and the scoring paths are theirs.  Per
// window this file enqueues, for s = 0 .. S - 1, k_search_compose (kernels_pose_search_joint.hpp: the pose of scan s
// into e->cand, w = 1.0 with the first scan and untouched after it) and the unchanged scoring path, which multiplies w
// in place; then search_fold_window once.  So a score is "leave w, rewrite the pose, score again": the un-normalised
// weight a noise-free particle started at the candidate carries after the S sensor updates, not a product of S
// separately rounded scores.
//
// Planar: score_planar stages the scan per call, so a window stages S scans against a ring of four slots; with S >= 4
// the host waits at the ring for the window before (profiles/pose_search_joint.md says what that costs).
// Cloud: stage_cloud is single-slot and waits for the stream, so it runs once, for the term table (which depends on
// the model only); the S clouds go up once into a buffer of this file's own in the float SoA layout of d_points, and
// launch_cloud is pointed at scan s's part of it.
//
// Read-only for the filter, exactly as the single-scan searches: the same fields are saved and put back on every path.
namespace
{
// theta_h as search_pose_of forms it (kernels_pose_search.hpp), evaluated on the host: a product, a division and a
// difference, none of which a compiler may fuse
double search_heading_of(int h, int headings)
{
  return (2.0 * 3.14159265358979323846 * (double)h) / (double)headings - 3.14159265358979323846;
}

void search_heading_table(int headings, double* cos_out, double* sin_out)
{
  for (int h = 0; h < headings; ++h)
  {
    const double th = search_heading_of(h, headings);
    cos_out[h] = std::cos(th);
    sin_out[h] = std::sin(th);
  }
}

// the arguments the four joint entry points check alike, before anything about the engine
int joint_offsets_ok(bpf_engine* e, int n_scans, const double* offsets)
{
  if (n_scans < 1 || n_scans > kSearchJointMaxScans)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "joint pose search: 1 <= n_scans <= 16");
  if (!offsets)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "joint pose search: offsets [n_scans][3] are needed");
  for (int q = 0; q < 3 * n_scans; ++q)
    if (!std::isfinite(offsets[q]))
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "joint pose search: an offset is not finite");
  return BPF_OK;
}

// C_h, S_h of the call's H headings on the device: d_joint_table[0 .. H) and [H .. 2 H).  Enqueues only.  The pinned
// side is single-slot: every joint call returns with the stream drained once it has come here.
int joint_table_up(bpf_engine* e, int headings)
{
  HIPCHK(e, e->h_joint_table.reserve(2 * (size_t)headings));
  HIPCHK(e, e->d_joint_table.reserve(2 * (size_t)headings));
  search_heading_table(headings, e->h_joint_table.p, e->h_joint_table.p + headings);
  H2D_OR_RETURN(pinned_up(e, e->d_joint_table, 0, e->h_joint_table, 0, 2 * (size_t)headings, e->stream));
  return BPF_OK;
}

int joint_compose(bpf_engine* e, int n, long long c0, const long long* ids, const SearchSpace& S, const double* D,
                  int first_scan)
{
  hipLaunchKernelGGL(k_search_compose, dim3(blocks_for(n, 256)), dim3(256), 0, e->stream, e->cand.dev(), n, c0, ids, S,
                     (const double*)e->d_joint_table.p, (const double*)(e->d_joint_table.p + S.headings), D[0], D[1],
                     D[2], first_scan);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_search_compose launch");
  return BPF_OK;
}

// the range checks of the single-scan searches, and the joint form's limit on the heading table
int joint_range_ok(bpf_engine* e, int headings, long long total, long long first, long long* count)
{
  if (total > 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "pose search: more than 2^31 - 1 candidates (raise cell_stride or lower headings)");
  if (headings > kSearchJointMaxHeadings)
    return e->fail(BPF_ERR_CAPACITY, "joint pose search: more than 65536 headings");
  if (first < 0 || first > total || *count < -1 || (*count >= 0 && *count > total - first))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: first / count outside the candidate space");
  if (*count < 0)
    *count = total - first;
  return BPF_OK;
}

int search_poses_joint(bpf_engine* e, int n_scans, const double* const* ranges, const double* const* angles,
                       const int* range_counts, const double* range_maxes, const double* offsets, int headings,
                       int cell_stride, long long first, long long count, int k, bpf_pose_hit* hits_out,
                       int* n_hits_out)
{
  int rc = joint_offsets_ok(e, n_scans, offsets);
  if (rc != BPF_OK)
    return rc;
  if (!hits_out || !n_hits_out || !ranges || !angles || !range_counts || !range_maxes)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: the scans and an output are needed");
  for (int s = 0; s < n_scans; ++s)
    if (!ranges[s] || !angles[s] || range_counts[s] <= 0)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: a scan and an output are needed");
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  if (headings < 1 || cell_stride < 1)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: headings >= 1 and cell_stride >= 1 are needed");
  if (!e->pm.configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the planar models: none is set");
  SearchSpace S;
  long long total = 0;
  rc = search_space_of(e, headings, cell_stride, &S, &total);
  if (rc != BPF_OK)
    return rc;
  rc = joint_range_ok(e, headings, total, first, &count);
  if (rc != BPF_OK)
    return rc;
  *n_hits_out = 0;
  if (count == 0)
    return BPF_OK;

  HIPCHK(e, e->cand.reserve((size_t)std::min<long long>(count, kSearchWindow)));
  rc = search_begin(e);
  if (rc != BPF_OK)
    return rc;
  // from the first enqueued copy on, a failure returns with the stream drained
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  rc = joint_table_up(e, headings);
  if (rc != BPF_OK)
    return drained(rc);
  const bool scored = e->pm.max_beams >= 2;  // (below that applyModelToSampleSet leaves the weight 1.0)
  for (long long done = 0; done < count; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(count - done, kSearchWindow);
    const long long c0 = first + done;
    for (int s = 0; s < (scored ? n_scans : 1); ++s)
    {
      rc = joint_compose(e, n, c0, nullptr, S, offsets + 3 * s, s == 0);
      if (rc != BPF_OK)
        return drained(rc);
      if (scored)
      {
        bool forced_zero = false;
        rc = score_planar(e, e->cand.dev(), n, 0, ranges[s], angles[s], range_counts[s], range_maxes[s], &forced_zero);
        if (rc != BPF_OK)
          return drained(rc);
      }
    }
    rc = search_fold_window(e, n, c0, k);
    if (rc != BPF_OK)
      return drained(rc);
  }
  rc = search_finish(e, S, k, hits_out, n_hits_out);
  return rc == BPF_OK ? rc : drained(rc);
}

int cloud_search_poses_joint(bpf_engine* e, int n_scans, const float* const* points_xyz, const int* n_points,
                             const double* offsets, int headings, int cell_stride, long long first, long long count,
                             int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  int rc = joint_offsets_ok(e, n_scans, offsets);
  if (rc != BPF_OK)
    return rc;
  if (!hits_out || !n_hits_out || !points_xyz || !n_points)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: the clouds and an output are needed");
  size_t all_points = 0;
  int most_points = 0;
  for (int s = 0; s < n_scans; ++s)
  {
    if (!points_xyz[s] || n_points[s] <= 0)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: a cloud and an output are needed");
    all_points += (size_t)n_points[s];
    most_points = std::max(most_points, n_points[s]);
  }
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  SearchSpace S;
  long long total = 0;
  rc = cloud_search_space_of(e, headings, cell_stride, &S, &total);
  if (rc != BPF_OK)
    return rc;
  if (!e->cloud_configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the point-cloud model: none is set");
  rc = joint_range_ok(e, headings, total, first, &count);
  if (rc != BPF_OK)
    return rc;
  *n_hits_out = 0;
  if (count == 0)
    return BPF_OK;
  HIPCHK(e, hipSetDevice(e->device));

  const bool scored = e->cloud_max_beams >= 2;  // (below that applyModelToSampleSet leaves the weight 1.0, :109-110)
  const int n_max = (int)std::min<long long>(count, kSearchWindow);
  // from the first enqueued copy on, a failure returns with the stream drained
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  // every buffer before the first copy is enqueued; the scoring scratch for the largest window and the largest cloud,
  // so that no launch_cloud reallocates behind a launch
  HIPCHK(e, e->cand.reserve((size_t)n_max));
  if (scored)
  {
    HIPCHK(e, e->h_joint_points.reserve(all_points * 3));
    HIPCHK(e, e->d_joint_points.reserve(all_points * 3));
    HIPCHK(e, e->d_affine.reserve((size_t)n_max * 12));
    HIPCHK(e, e->d_cloud_partials.reserve((size_t)blocks_for(most_points, kCloudChunk) * n_max));
  }
  rc = search_begin(e);
  if (rc != BPF_OK)
    return drained(rc);
  std::vector<size_t> at((size_t)n_scans, 0);  // where scan s's x row starts in d_joint_points
  if (scored)
  {
    // the term table, and the one wait for the stream that the single-slot staging buffers need (it stages the first
    // cloud into d_points as well, which nothing below reads)
    rc = stage_cloud(e, points_xyz[0], n_points[0]);
    if (rc != BPF_OK)
      return drained(rc);
    size_t off = 0;
    for (int s = 0; s < n_scans; ++s)
    {
      const size_t np = (size_t)n_points[s];
      float* dst = e->h_joint_points.p + off;
      for (size_t q = 0; q < np; ++q)
      {
        dst[q] = points_xyz[s][3 * q];
        dst[np + q] = points_xyz[s][3 * q + 1];
        dst[2 * np + q] = points_xyz[s][3 * q + 2];
      }
      at[(size_t)s] = off;
      off += 3 * np;
    }
    rc = pinned_up(e, e->d_joint_points, 0, e->h_joint_points, 0, all_points * 3, e->stream);
    if (rc != BPF_OK)
      return drained(rc);
  }
  rc = joint_table_up(e, headings);
  if (rc != BPF_OK)
    return drained(rc);
  for (long long done = 0; done < count; done += kSearchWindow)
  {
    const int n = (int)std::min<long long>(count - done, kSearchWindow);
    const long long c0 = first + done;
    for (int s = 0; s < (scored ? n_scans : 1); ++s)
    {
      rc = joint_compose(e, n, c0, nullptr, S, offsets + 3 * s, s == 0);
      if (rc != BPF_OK)
        return drained(rc);
      if (scored)
      {
        rc = launch_cloud(e, e->cand.dev(), n, n_points[s], nullptr, e->d_joint_points.p + at[(size_t)s]);
        if (rc != BPF_OK)
          return drained(rc);
      }
    }
    rc = search_fold_window(e, n, c0, k);
    if (rc != BPF_OK)
      return drained(rc);
  }
  rc = search_finish(e, S, k, hits_out, n_hits_out);
  return rc == BPF_OK ? rc : drained(rc);
}

// the diagnostic of both scanners: the composed poses of the candidates given, from k_search_compose itself
int search_joint_poses(bpf_engine* e, const SearchSpace& S, long long total, const double* offsets, int n_scans,
                       const long long* candidates, int n, double* poses_out)
{
  if (total > 0x7fffffffll)
    return e->fail(BPF_ERR_CAPACITY, "pose search: more than 2^31 - 1 candidates (raise cell_stride or lower headings)");
  if (S.headings > kSearchJointMaxHeadings)
    return e->fail(BPF_ERR_CAPACITY, "joint pose search: more than 65536 headings");
  for (int t = 0; t < n; ++t)
    if (candidates[t] < 0 || candidates[t] >= total)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "joint pose search: a candidate outside the space");
  if (n == 0)
    return BPF_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const int n_max = std::min(n, kSearchWindow);
  HIPCHK(e, e->cand.reserve((size_t)n_max));
  HIPCHK(e, e->d_joint_ids.reserve((size_t)n_max));
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  int rc = joint_table_up(e, S.headings);
  if (rc != BPF_OK)
    return drained(rc);
  std::vector<double> row((size_t)n_max);
  for (int done = 0; done < n; done += kSearchWindow)
  {
    const int m = std::min(n - done, kSearchWindow);
    rc = h2d_from_host(e, e->d_joint_ids.p, candidates + done, (size_t)m * sizeof(long long), e->stream);
    if (rc != BPF_OK)
      return drained(rc);
    for (int s = 0; s < n_scans; ++s)
    {
      rc = joint_compose(e, m, 0, e->d_joint_ids.p, S, offsets + 3 * s, s == 0);
      if (rc != BPF_OK)
        return drained(rc);
      const double* parts[3] = { e->cand.x.p, e->cand.y.p, e->cand.th.p };
      for (int a = 0; a < 3; ++a)
      {
        rc = d2h_to_host(e, row.data(), parts[a], (size_t)m * sizeof(double), e->stream);  // (waits)
        if (rc != BPF_OK)
          return drained(rc);
        for (int t = 0; t < m; ++t)
          poses_out[((size_t)(done + t) * (size_t)n_scans + (size_t)s) * 3 + (size_t)a] = row[(size_t)t];
      }
    }
  }
  return BPF_OK;
}

int search_joint_poses_checked(bpf_engine* e, bool cloud, int headings, int cell_stride, const double* offsets,
                               int n_scans, const long long* candidates, int n, double* poses_out)
{
  int rc = joint_offsets_ok(e, n_scans, offsets);
  if (rc != BPF_OK)
    return rc;
  if (n < 0 || (n > 0 && (!candidates || !poses_out)))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "joint pose search: candidates and an output are needed");
  SearchSpace S;
  long long total = 0;
  rc = cloud ? cloud_search_space_of(e, headings, cell_stride, &S, &total)
             : search_space_of(e, headings, cell_stride, &S, &total);
  if (rc != BPF_OK)
    return rc;
  return search_joint_poses(e, S, total, offsets, n_scans, candidates, n, poses_out);
}
}  // namespace

int bpf_pose_search_heading_table(int headings, double* cos_out, double* sin_out)
{
  if (headings < 1 || !cos_out || !sin_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (headings > kSearchJointMaxHeadings)
    return BPF_ERR_CAPACITY;
  search_heading_table(headings, cos_out, sin_out);
  return BPF_OK;
}

int bpf_planar_search_poses_joint(bpf_engine* e, int n_scans, const double* const* ranges, const double* const* angles,
                                  const int* range_counts, const double* range_maxes, const double* offsets,
                                  int headings, int cell_stride, long long first, long long count, int k,
                                  bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // what the scoring calls reset describes the engine's set, not the candidates: put back, whatever the outcome
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_score_form;
  const bool window_path = e->last_used_window_path;
  const int rc = search_poses_joint(e, n_scans, ranges, angles, range_counts, range_maxes, offsets, headings,
                                    cell_stride, first, count, k, hits_out, n_hits_out);
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_score_form = form;
  e->last_used_window_path = window_path;
  return rc;
}

int bpf_cloud_search_poses_joint(bpf_engine* e, int n_scans, const float* const* points_xyz, const int* n_points,
                                 const double* offsets, int headings, int cell_stride, long long first,
                                 long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // as bpf_cloud_search_poses: what describes the engine's last scoring call is put back, and profiling is off for
  // the call, so no event slot is taken
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_cloud_form;
  const bool profiling = e->profiling;
  e->profiling = false;
  const int rc = cloud_search_poses_joint(e, n_scans, points_xyz, n_points, offsets, headings, cell_stride, first,
                                          count, k, hits_out, n_hits_out);
  e->profiling = profiling;
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_cloud_form = form;
  return rc;
}

int bpf_planar_search_joint_poses(bpf_engine* e, int headings, int cell_stride, const double* offsets, int n_scans,
                                  const long long* candidates, int n, double* poses_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  const int rc = search_joint_poses_checked(e, false, headings, cell_stride, offsets, n_scans, candidates, n, poses_out);
  e->last_status = status;
  return rc;
}

int bpf_cloud_search_joint_poses(bpf_engine* e, int headings, int cell_stride, const double* offsets, int n_scans,
                                 const long long* candidates, int n, double* poses_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  const int rc = search_joint_poses_checked(e, true, headings, cell_stride, offsets, n_scans, candidates, n, poses_out);
  e->last_status = status;
  return rc;
}
