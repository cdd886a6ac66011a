// C-ABI: pose moments (include/badger_pf.h) -- per pose the score-weighted first and second moments of one lattice of
// the refinement (level 0: the steps as given), and bpf_pose_mixture_apply_moments, the host step from those moments
// to the rotation / sigma of mixture components.  The driver is shaped like refine_run (abi_pose_refine.inl): the
// poses go up once, groups of max(1, window / M) poses, per group k_refine_candidates, the scoring path of the
// searches, then k_pose_moments, everything enqueued back to back; this thread waits once, for the rows (the cloud
// form a second time, in its staging).  With scores_out a group's scores leave e->cand.w on the stream before the
// next group overwrites them.
//
// Read-only for the filter: what the refinement saves and puts back is saved and put back here.
namespace
{
static_assert(sizeof(bpf_pose_moments) == 96, "bpf_pose_moments is 96 bytes in every binding");

// arguments both forms check alike; the lattice (steps included) on success
int moments_arguments(bpf_engine* e, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                      int theta_radius, double theta_step, double baseline, const bpf_pose_moments* out,
                      RefineLattice* G)
{
  if (!poses_xyt || !out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: poses and an output are needed");
  if (n_poses < 1 || n_poses > kRefineMaxPoses)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: 1 <= n_poses <= 1024");
  if (!refine_lattice_of(xy_radius, theta_radius, G))
    return e->fail(BPF_ERR_INVALID_ARGUMENT,
                   "pose moments: radii >= 0 and 2 <= (2 xy_radius + 1)^2 (2 theta_radius + 1) <= 2048");
  if (xy_radius > 0 && !(std::isfinite(xy_step) && xy_step > 0.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: xy_step must be finite and > 0");
  if (theta_radius > 0 && !(std::isfinite(theta_step) && theta_step > 0.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: theta_step must be finite and > 0");
  if (!(std::isfinite(baseline) && baseline >= 0.0 && baseline < 1.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: 0 <= baseline < 1");
  for (int v = 0; v < 3 * n_poses; ++v)
    if (!std::isfinite(poses_xyt[v]))
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: every input pose must be finite");
  G->xy_step = xy_radius > 0 ? xy_step : 0.0;
  G->theta_step = theta_radius > 0 ? theta_step : 0.0;
  return BPF_OK;
}

// `score(n)` enqueues the scoring of e->cand[0 .. n) and returns its status; it is not called where the scanner
// leaves every weight 1.0 (max_beams < 2).
int moments_run(bpf_engine* e, const double* poses_xyt, int n_poses, const RefineLattice& G, double baseline,
                bool scored, const std::function<int(int)>& score, bpf_pose_moments* out, double* scores_out)
{
  const int M = G.M;
  const int group = std::max(1, kSearchWindow / M);
  const size_t n = (size_t)n_poses;
  HIPCHK(e, e->cand.reserve((size_t)std::min(n_poses, group) * M));
  HIPCHK(e, e->d_refine_centres.reserve(3 * n));
  HIPCHK(e, e->d_moments_rows.reserve(n));
  HIPCHK(e, e->h_refine_in.reserve(3 * n));
  HIPCHK(e, e->h_moments_rows.reserve(n));
  if (scores_out)
    HIPCHK(e, e->h_moments_scores.reserve(n * M));
  // (h_refine_in is free: every call that filled it has waited for its rows since)
  std::memcpy(e->h_refine_in.p, poses_xyt, 3 * n * sizeof(double));
  H2D_OR_RETURN(pinned_up(e, e->d_refine_centres, 0, e->h_refine_in, 0, 3 * n, e->stream));
  // from the first launch on, a failure returns with the stream drained
  auto drained = [&](int code) {
    (void)hipStreamSynchronize(e->stream);
    return code;
  };
  for (int r0 = 0; r0 < n_poses; r0 += group)
  {
    const int ng = std::min(group, n_poses - r0);
    const int nc = ng * M;
    hipLaunchKernelGGL(k_refine_candidates, dim3(blocks_for(nc, 256)), dim3(256), 0, e->stream, e->cand.dev(), ng, r0,
                       (const double*)e->d_refine_centres.p, G);
    if (hipGetLastError() != hipSuccess)
      return drained(e->fail(BPF_ERR_HIP, "k_refine_candidates launch"));
    if (scored)
    {
      const int rc = score(nc);
      if (rc != BPF_OK)
        return drained(rc);
    }
    hipLaunchKernelGGL(k_pose_moments, dim3(ng), dim3(kMomentsThreads), 0, e->stream, (const double*)e->cand.w.p, r0,
                       G, baseline, (const double*)e->d_refine_centres.p, e->d_moments_rows.p);
    if (hipGetLastError() != hipSuccess)
      return drained(e->fail(BPF_ERR_HIP, "k_pose_moments launch"));
    if (scores_out)
    {
      const int rc = pinned_down(e, e->h_moments_scores, (size_t)r0 * M, e->cand.w, 0, (size_t)nc, e->stream);
      if (rc != BPF_OK)
        return drained(rc);
    }
  }
  const int rc = pinned_down_sync(e, e->h_moments_rows, 0, e->d_moments_rows, 0, n, e->stream);
  if (rc != BPF_OK)
    return drained(rc);
  std::memcpy(out, e->h_moments_rows.p, n * sizeof(bpf_pose_moments));
  if (scores_out)
    std::memcpy(scores_out, e->h_moments_scores.p, n * M * sizeof(double));
  return BPF_OK;
}

int planar_pose_moments(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                        const double* poses_xyt, int n_poses, int xy_radius, double xy_step, int theta_radius,
                        double theta_step, double baseline, bpf_pose_moments* out, double* scores_out)
{
  if (!ranges || !angles || range_count <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: a scan is needed");
  RefineLattice G;
  const int rc =
      moments_arguments(e, poses_xyt, n_poses, xy_radius, xy_step, theta_radius, theta_step, baseline, out, &G);
  if (rc != BPF_OK)
    return rc;
  if (!e->pm.configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose moments score with the planar models: none is set");
  if (!e->have_map || !e->have_lut)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose moments need the 2-D map and its distance LUT");
  HIPCHK(e, hipSetDevice(e->device));
  return moments_run(
      e, poses_xyt, n_poses, G, baseline, e->pm.max_beams >= 2,
      [&](int n) {
        bool forced_zero = false;
        return score_planar(e, e->cand.dev(), n, 0, ranges, angles, range_count, range_max, &forced_zero);
      },
      out, scores_out);
}

int cloud_pose_moments(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                       int xy_radius, double xy_step, int theta_radius, double theta_step, double baseline,
                       bpf_pose_moments* out, double* scores_out)
{
  if (!points_xyz || n_points <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose moments: a cloud is needed");
  RefineLattice G;
  int rc = moments_arguments(e, poses_xyt, n_poses, xy_radius, xy_step, theta_radius, theta_step, baseline, out, &G);
  if (rc != BPF_OK)
    return rc;
  if (!e->have_map3d)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "cloud pose moments need the 3-D map (bpf_map3d_set)");
  if (!e->cloud_configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose moments score with the point-cloud model: none is set");
  HIPCHK(e, hipSetDevice(e->device));
  const bool scored = e->cloud_max_beams >= 2;
  if (scored)
  {
    rc = stage_cloud(e, points_xyz, n_points);  // (waits for the stream: nothing below frees a buffer in use)
    if (rc != BPF_OK)
      return rc;
    // all scratch for the largest launch, so that no group reallocates
    const size_t n_max = (size_t)std::min(n_poses, std::max(1, kSearchWindow / G.M)) * G.M;
    HIPCHK(e, e->d_affine.reserve(n_max * 12));
    HIPCHK(e, e->d_cloud_partials.reserve((size_t)blocks_for(n_points, kCloudChunk) * n_max));
  }
  return moments_run(
      e, poses_xyt, n_poses, G, baseline, scored, [&](int n) { return launch_cloud(e, e->cand.dev(), n, n_points); },
      out, scores_out);
}

// ---------------------------------------------------------------------- moments to components
// cyclic Jacobi on the symmetric a[3][3] (both triangles kept); v receives the eigenvectors as columns
void moments_jacobi(double a[3][3], double v[3][3])
{
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      v[i][j] = i == j ? 1.0 : 0.0;
  static const int pairs[3][2] = { { 0, 1 }, { 0, 2 }, { 1, 2 } };
  for (int sweep = 0; sweep < 8; ++sweep)
  {
    if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0)
      break;
    for (const auto& pq : pairs)
    {
      const int p = pq[0], q = pq[1], r = 3 - p - q;
      const double apq = a[p][q];
      if (apq == 0.0)
        continue;
      const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double at = tau < 0.0 ? -tau : tau;
      const double mag = 1.0 / (at + std::sqrt(tau * tau + 1.0));
      const double t = tau < 0.0 ? -mag : mag;
      const double c = 1.0 / std::sqrt(t * t + 1.0);
      const double s = t * c;
      const double app = a[p][p], aqq = a[q][q], arp = a[r][p], arq = a[r][q];
      a[p][p] = app - t * apq;
      a[q][q] = aqq + t * apq;
      a[p][q] = a[q][p] = 0.0;
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int k = 0; k < 3; ++k)
      {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
    }
  }
}
}  // namespace

int bpf_planar_pose_moments(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                            int theta_radius, double theta_step, double baseline, bpf_pose_moments* out,
                            double* scores_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // as bpf_planar_refine_poses: what the scoring calls reset describes the engine's set, not the lattice
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_score_form;
  const bool window_path = e->last_used_window_path;
  const int rc = planar_pose_moments(e, ranges, angles, range_count, range_max, poses_xyt, n_poses, xy_radius, xy_step,
                                     theta_radius, theta_step, baseline, out, scores_out);
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_score_form = form;
  e->last_used_window_path = window_path;
  return rc;
}

int bpf_cloud_pose_moments(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                           int xy_radius, double xy_step, int theta_radius, double theta_step, double baseline,
                           bpf_pose_moments* out, double* scores_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // as bpf_cloud_refine_poses: profiling is off for the call, so no event slot is taken
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_cloud_form;
  const bool profiling = e->profiling;
  e->profiling = false;
  const int rc = cloud_pose_moments(e, points_xyz, n_points, poses_xyt, n_poses, xy_radius, xy_step, theta_radius,
                                    theta_step, baseline, out, scores_out);
  e->profiling = profiling;
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_cloud_form = form;
  return rc;
}

int bpf_pose_mixture_apply_moments(bpf_mixture_component* comps, int n_components, const int* source_row,
                                   const bpf_pose_moments* rows, int n_rows, const double sigma_floor[3],
                                   const double sigma_cap[3], int take_mean)
{
#pragma clang fp contract(off)
  if (!comps || !source_row || !rows || !sigma_floor || !sigma_cap)
    return BPF_ERR_INVALID_ARGUMENT;
  if (n_components < 1 || n_components > kMixtureMax || n_rows < 1 || n_rows > kMixtureMax)
    return BPF_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n_components; ++k)
    if (source_row[k] < 0 || source_row[k] >= n_rows)
      return BPF_ERR_INVALID_ARGUMENT;
  for (int q = 0; q < 3; ++q)
    if (!(std::isfinite(sigma_floor[q]) && sigma_floor[q] >= 0.0 && std::isfinite(sigma_cap[q]) &&
          sigma_cap[q] >= sigma_floor[q]))
      return BPF_ERR_INVALID_ARGUMENT;
  for (int r = 0; r < n_rows; ++r)
    if (rows[r].flags & BPF_MOMENTS_VALID)
      for (int q = 0; q < 6; ++q)
        if (!std::isfinite(rows[r].cov[q]))
          return BPF_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n_components; ++k)
  {
    const bpf_pose_moments& row = rows[source_row[k]];
    if (!(row.flags & BPF_MOMENTS_VALID))
      continue;
    double a[3][3] = { { row.cov[0], row.cov[1], row.cov[2] },
                       { row.cov[1], row.cov[3], row.cov[4] },
                       { row.cov[2], row.cov[4], row.cov[5] } };
    double v[3][3];
    moments_jacobi(a, v);
    bpf_mixture_component& c = comps[k];
    for (int i = 0; i < 3; ++i)
    {
      int axis = 0;
      for (int j = 1; j < 3; ++j)
        if (std::fabs(v[j][i]) > std::fabs(v[axis][i]))
          axis = j;
      const double lo = sigma_floor[axis] * sigma_floor[axis], hi = sigma_cap[axis] * sigma_cap[axis];
      double lambda = a[i][i];
      if (!(lambda >= lo))
        lambda = lo;
      if (lambda > hi)
        lambda = hi;
      c.sigma[i] = std::sqrt(lambda);
      for (int j = 0; j < 3; ++j)
        c.rotation[3 * j + i] = v[j][i];
    }
    if (take_mean)
    {
      c.mean[0] = row.mean[0];
      c.mean[1] = row.mean[1];
      c.mean[2] = mixture_normalize_angle(row.mean[2]);
    }
  }
  return BPF_OK;
}
