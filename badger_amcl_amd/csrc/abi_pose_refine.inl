// C-ABI: pose refinement (include/badger_pf.h) -- a coarse-to-fine lattice descent around up to 1024 poses, all of it
// on the device.  The poses go up once; they are processed in groups of max(1, window / M) poses so that a launch
// scores at most bpf_pose_search_window() candidates; per group and level k_refine_candidates writes the lattice into
// the engine's candidate set, the scoring path of the searches scores it (score_planar with set->converged = 0;
// launch_cloud against what stage_cloud staged once), and k_refine_select moves every centre to its best point.  A
// pose's descent reads only its own M scores, so the grouping does not show in the result.  Every level of every
// group is enqueued behind the one before; this thread waits once, for the rows (the cloud form a second time, before
// its first launch, for the staging buffers).  score_planar stages the scan per launch, as it does for the search: a
// slot of its ring is reused after kRing launches, so the host may wait there for the launch four back.
//
// Read-only for the filter: what the searches save and put back is saved and put back here.
namespace
{
static_assert(sizeof(bpf_pose_refined) == 48, "bpf_pose_refined is 48 bytes in every binding");

// the lattice of (xy_radius, theta_radius), or false where the limits of the call refuse it
bool refine_lattice_of(int xy_radius, int theta_radius, RefineLattice* G)
{
  if (xy_radius < 0 || theta_radius < 0 || xy_radius > kRefineMaxPoints || theta_radius > kRefineMaxPoints)
    return false;
  const long long side = 2ll * xy_radius + 1, turns = 2ll * theta_radius + 1;
  const long long M = side * side * turns;
  if (M < 2 || M > kRefineMaxPoints)
    return false;
  *G = RefineLattice{};
  G->R = xy_radius;
  G->A = theta_radius;
  G->M = (int)M;
  G->centre = (int)((xy_radius * side + xy_radius) * turns + theta_radius);
  return true;
}

// arguments both forms check alike; the lattice on success
int refine_arguments(bpf_engine* e, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                     int theta_radius, double theta_step, int levels, const bpf_pose_refined* out, RefineLattice* G)
{
  if (!poses_xyt || !out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: poses and an output are needed");
  if (n_poses < 1 || n_poses > kRefineMaxPoses)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: 1 <= n_poses <= 1024");
  if (levels < 1 || levels > kRefineMaxLevels)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: 1 <= levels <= 16");
  if (!refine_lattice_of(xy_radius, theta_radius, G))
    return e->fail(BPF_ERR_INVALID_ARGUMENT,
                   "pose refinement: radii >= 0 and 2 <= (2 xy_radius + 1)^2 (2 theta_radius + 1) <= 2048");
  if (xy_radius > 0 && !(std::isfinite(xy_step) && xy_step > 0.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: xy_step must be finite and > 0");
  if (theta_radius > 0 && !(std::isfinite(theta_step) && theta_step > 0.0))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: theta_step must be finite and > 0");
  for (int v = 0; v < 3 * n_poses; ++v)
    if (!std::isfinite(poses_xyt[v]))
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: every input pose must be finite");
  return BPF_OK;
}

// The descent.  `score(n)` enqueues the scoring of e->cand[0 .. n) and returns its status; it is not called where the
// scanner leaves every weight 1.0 (max_beams < 2).
int refine_run(bpf_engine* e, const double* poses_xyt, int n_poses, const RefineLattice& lattice, double xy_step,
               double theta_step, int levels, bool scored, const std::function<int(int)>& score,
               bpf_pose_refined* out, int* trace_out)
{
  const int M = lattice.M;
  const int group = std::max(1, kSearchWindow / M);
  const size_t n = (size_t)n_poses;
  HIPCHK(e, e->cand.reserve((size_t)std::min(n_poses, group) * M));
  HIPCHK(e, e->d_refine_centres.reserve(3 * n));
  HIPCHK(e, e->d_refine_score.reserve(n));
  HIPCHK(e, e->d_refine_score_in.reserve(n));
  HIPCHK(e, e->d_refine_moved.reserve(n));
  HIPCHK(e, e->d_refine_trace.reserve(n * levels));
  HIPCHK(e, e->d_refine_rows.reserve(n));
  HIPCHK(e, e->h_refine_in.reserve(3 * n));
  HIPCHK(e, e->h_refine_rows.reserve(n));
  if (trace_out)
    HIPCHK(e, e->h_refine_trace.reserve(n * levels));
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
    for (int level = 0; level < levels; ++level)
    {
      RefineLattice G = lattice;
      G.xy_step = lattice.R > 0 ? std::ldexp(xy_step, -level) : 0.0;
      G.theta_step = lattice.A > 0 ? std::ldexp(theta_step, -level) : 0.0;
      hipLaunchKernelGGL(k_refine_candidates, dim3(blocks_for(nc, 256)), dim3(256), 0, e->stream, e->cand.dev(), ng,
                         r0, (const double*)e->d_refine_centres.p, G);
      if (hipGetLastError() != hipSuccess)
        return drained(e->fail(BPF_ERR_HIP, "k_refine_candidates launch"));
      if (scored)
      {
        const int rc = score(nc);
        if (rc != BPF_OK)
          return drained(rc);
      }
      hipLaunchKernelGGL(k_refine_select, dim3(ng), dim3(kRefineThreads), 0, e->stream, e->cand.dev(), r0, G, level,
                         levels, e->d_refine_centres.p, e->d_refine_score.p, e->d_refine_score_in.p,
                         e->d_refine_moved.p, e->d_refine_trace.p);
      if (hipGetLastError() != hipSuccess)
        return drained(e->fail(BPF_ERR_HIP, "k_refine_select launch"));
    }
  }
  hipLaunchKernelGGL(k_refine_rows, dim3(blocks_for(n_poses, 256)), dim3(256), 0, e->stream, n_poses,
                     (const double*)e->d_refine_centres.p, (const double*)e->d_refine_score.p,
                     (const double*)e->d_refine_score_in.p, (const int*)e->d_refine_moved.p, e->d_refine_rows.p);
  if (hipGetLastError() != hipSuccess)
    return drained(e->fail(BPF_ERR_HIP, "k_refine_rows launch"));
  int rc = BPF_OK;
  if (trace_out)
    rc = pinned_down(e, e->h_refine_trace, 0, e->d_refine_trace, 0, n * levels, e->stream);
  if (rc == BPF_OK)
    rc = pinned_down_sync(e, e->h_refine_rows, 0, e->d_refine_rows, 0, n, e->stream);
  if (rc != BPF_OK)
    return drained(rc);
  std::memcpy(out, e->h_refine_rows.p, n * sizeof(bpf_pose_refined));
  if (trace_out)
    std::memcpy(trace_out, e->h_refine_trace.p, n * levels * sizeof(int));
  return BPF_OK;
}

int planar_refine_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                        const double* poses_xyt, int n_poses, int xy_radius, double xy_step, int theta_radius,
                        double theta_step, int levels, bpf_pose_refined* out, int* trace_out)
{
  if (!ranges || !angles || range_count <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: a scan is needed");
  RefineLattice G;
  int rc = refine_arguments(e, poses_xyt, n_poses, xy_radius, xy_step, theta_radius, theta_step, levels, out, &G);
  if (rc != BPF_OK)
    return rc;
  if (!e->pm.configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose refinement scores with the planar models: none is set");
  if (!e->have_map || !e->have_lut)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose refinement needs the 2-D map and its distance LUT");
  HIPCHK(e, hipSetDevice(e->device));
  // (with max_beams < 2 applyModelToSampleSet leaves the weight 1.0, planar_scanner.cpp:144-145)
  return refine_run(
      e, poses_xyt, n_poses, G, xy_step, theta_step, levels, e->pm.max_beams >= 2,
      [&](int n) {
        bool forced_zero = false;
        return score_planar(e, e->cand.dev(), n, 0, ranges, angles, range_count, range_max, &forced_zero);
      },
      out, trace_out);
}

int cloud_refine_poses(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                       int xy_radius, double xy_step, int theta_radius, double theta_step, int levels,
                       bpf_pose_refined* out, int* trace_out)
{
  if (!points_xyz || n_points <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose refinement: a cloud is needed");
  RefineLattice G;
  int rc = refine_arguments(e, poses_xyt, n_poses, xy_radius, xy_step, theta_radius, theta_step, levels, out, &G);
  if (rc != BPF_OK)
    return rc;
  if (!e->have_map3d)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "cloud pose refinement needs the 3-D map (bpf_map3d_set)");
  if (!e->cloud_configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose refinement scores with the point-cloud model: none is set");
  HIPCHK(e, hipSetDevice(e->device));
  const bool scored = e->cloud_max_beams >= 2;  // (below that applyModelToSampleSet leaves the weight 1.0, :109-110)
  if (scored)
  {
    rc = stage_cloud(e, points_xyz, n_points);  // (waits for the stream: nothing below frees a buffer in use)
    if (rc != BPF_OK)
      return rc;
    // all scratch for the largest launch, so that no level reallocates
    const size_t n_max = (size_t)std::min(n_poses, std::max(1, kSearchWindow / G.M)) * G.M;
    HIPCHK(e, e->d_affine.reserve(n_max * 12));
    HIPCHK(e, e->d_cloud_partials.reserve((size_t)blocks_for(n_points, kCloudChunk) * n_max));
  }
  return refine_run(
      e, poses_xyt, n_poses, G, xy_step, theta_step, levels, scored,
      [&](int n) { return launch_cloud(e, e->cand.dev(), n, n_points); }, out, trace_out);
}
}  // namespace

int bpf_pose_refine_lattice(int xy_radius, int theta_radius, int* points_out, int* centre_out)
{
  RefineLattice G;
  if (!refine_lattice_of(xy_radius, theta_radius, &G))
    return BPF_ERR_INVALID_ARGUMENT;
  if (points_out)
    *points_out = G.M;
  if (centre_out)
    *centre_out = G.centre;
  return BPF_OK;
}

int bpf_planar_refine_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                            int theta_radius, double theta_step, int levels, bpf_pose_refined* out, int* trace_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // what the scoring calls reset describes the engine's set, not the lattice: put back, whatever the outcome
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_score_form;
  const bool window_path = e->last_used_window_path;
  const int rc = planar_refine_poses(e, ranges, angles, range_count, range_max, poses_xyt, n_poses, xy_radius, xy_step,
                                     theta_radius, theta_step, levels, out, trace_out);
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_score_form = form;
  e->last_used_window_path = window_path;
  return rc;
}

int bpf_cloud_refine_poses(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                           int xy_radius, double xy_step, int theta_radius, double theta_step, int levels,
                           bpf_pose_refined* out, int* trace_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // as bpf_cloud_search_poses: profiling is off for the call, so no event slot is taken
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_cloud_form;
  const bool profiling = e->profiling;
  e->profiling = false;
  const int rc = cloud_refine_poses(e, points_xyz, n_points, poses_xyt, n_poses, xy_radius, xy_step, theta_radius,
                                    theta_step, levels, out, trace_out);
  e->profiling = profiling;
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_cloud_form = form;
  return rc;
}
