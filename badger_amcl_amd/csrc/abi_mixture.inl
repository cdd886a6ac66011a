// C-ABI: the mixture initialiser's host side -- the checked component table on its way to the device
// (kernels_mixture.hpp; the init calls are next to their Gaussian forms in abi_motion.inl, abi_shard_init.inl and
// abi_shard_node.inl) and bpf_pose_mixture_from_hits, the step from hit rows to components.
// ---------------------------------------------------------------------- mixture initialiser
namespace
{
// the table as the device reads it: k rows of kMixtureRow doubles, then int32[k + 1], the exclusive prefix of the
// counts, in the doubles behind them -- one buffer, so one copy
struct MixtureTable
{
  std::vector<double> words;
  int k = 0;
  bool spread = false;  // more than one component has samples
};

// every refusal of bpf_pf_init_with_mixture that concerns the components; nothing of the engine changes
int mixture_table(bpf_engine* e, const bpf_mixture_component* comps, int n_components, long long total,
                  MixtureTable* T)
{
  if (n_components < 1 || n_components > kMixtureMax)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "mixture init: n_components outside [1, 1024]");
  long long sum = 0;
  int with_samples = 0;
  for (int c = 0; c < n_components; ++c)
  {
    if (comps[c].count < 0)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "mixture init: a negative count");
    sum += comps[c].count;
    if (comps[c].count == 0)
      continue;  // (its other fields are not read)
    ++with_samples;
    bool finite = true;
    for (int q = 0; q < 3; ++q)
      finite = finite && std::isfinite(comps[c].mean[q]) && std::isfinite(comps[c].sigma[q]);
    for (int q = 0; q < 9; ++q)
      finite = finite && std::isfinite(comps[c].rotation[q]);
    if (!finite)
      return e->fail(BPF_ERR_INVALID_ARGUMENT, "mixture init: a non-finite mean, rotation or sigma");
  }
  if (sum != total)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "mixture init: the counts must sum to max_samples");
  const size_t rows = (size_t)n_components * kMixtureRow;
  T->k = n_components;
  T->spread = with_samples > 1;
  T->words.assign(rows + ((size_t)n_components + 2) / 2, 0.0);
  std::vector<int> prefix((size_t)n_components + 1, 0);
  for (int c = 0; c < n_components; ++c)
  {
    prefix[(size_t)c + 1] = prefix[c] + comps[c].count;
    if (comps[c].count == 0)
      continue;
    double* row = &T->words[(size_t)c * kMixtureRow];
    std::memcpy(row, comps[c].mean, 3 * sizeof(double));
    std::memcpy(row + 3, comps[c].rotation, 9 * sizeof(double));
    std::memcpy(row + 12, comps[c].sigma, 3 * sizeof(double));
  }
  std::memcpy(&T->words[rows], prefix.data(), prefix.size() * sizeof(int));
  return BPF_OK;
}

int mixture_upload(bpf_engine* e, const MixtureTable& T, MixtureDev* X)
{
  HIPCHK(e, e->d_mixture.reserve(T.words.size()));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_mixture.p, T.words.data(), T.words.size() * sizeof(double)));
  X->rows = e->d_mixture.p;
  X->prefix = reinterpret_cast<const int*>(e->d_mixture.p + (size_t)T.k * kMixtureRow);
  X->k = T.k;
  return BPF_OK;
}

// angles::normalize_angle in its Noetic form (third party), as odom_angle_diff and normalize_angle_dev restate it
double mixture_normalize_angle(double a)
{
  const double r = std::fmod(a + M_PI, 2.0 * M_PI);
  return (r <= 0.0) ? r + M_PI : r - M_PI;
}
}  // namespace

int bpf_pose_mixture_from_hits(const double* poses_xyt, const double* scores, int n_rows, int total_count,
                               double xy_merge, double theta_merge, int max_components, const double sigma[3],
                               bpf_mixture_component* out, int* source_row_out, int* merged_out, int* n_components_out)
{
  if (!poses_xyt || !scores || !sigma || !out || !n_components_out)
    return BPF_ERR_INVALID_ARGUMENT;
  if (n_rows < 1 || n_rows > kMixtureMax || max_components < 1 || max_components > kMixtureMax || total_count < 1)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(xy_merge) && xy_merge >= 0.0 && std::isfinite(theta_merge) && theta_merge >= 0.0))
    return BPF_ERR_INVALID_ARGUMENT;
  for (int q = 0; q < 3; ++q)
    if (!(std::isfinite(sigma[q]) && sigma[q] >= 0.0))
      return BPF_ERR_INVALID_ARGUMENT;
  // 1. usable rows, by score descending, equal scores by row
  std::vector<int> order;
  for (int r = 0; r < n_rows; ++r)
  {
    const double* p = poses_xyt + 3 * (size_t)r;
    if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(scores[r]) &&
        scores[r] > 0.0)
      order.push_back(r);
  }
  if (order.empty())
    return BPF_ERR_INVALID_ARGUMENT;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a] > scores[b]; });
  // 2. suppression
  std::vector<int> kept, merged;
  for (int r : order)
  {
    const double* p = poses_xyt + 3 * (size_t)r;
    int by = -1;
    for (size_t c = 0; c < kept.size() && by < 0; ++c)
    {
      const double* q = poses_xyt + 3 * (size_t)kept[c];
      if (std::fabs(p[0] - q[0]) <= xy_merge && std::fabs(p[1] - q[1]) <= xy_merge &&
          std::fabs(mixture_normalize_angle(p[2] - q[2])) <= theta_merge)
        by = (int)c;
    }
    if (by >= 0)
      ++merged[by];
    else if ((int)kept.size() < max_components)
    {
      kept.push_back(r);
      merged.push_back(0);
    }
  }
  // 3. components, 4. counts by largest remainder
  const int K = (int)kept.size();
  double W = 0.0;
  for (int k = 0; k < K; ++k)
    W += scores[kept[k]];
  std::vector<double> rem((size_t)K);
  std::vector<int> count((size_t)K);
  long long given = 0;
  for (int k = 0; k < K; ++k)
  {
    const double t = ((double)total_count * scores[kept[k]]) / W;
    const double f = std::floor(t);
    count[k] = (int)f;
    rem[k] = t - f;
    given += count[k];
  }
  std::vector<int> by_rem((size_t)K);
  for (int k = 0; k < K; ++k)
    by_rem[k] = k;
  std::stable_sort(by_rem.begin(), by_rem.end(), [&](int a, int b) { return rem[a] > rem[b]; });
  for (size_t at = 0; given < total_count; at = (at + 1) % (size_t)K)
  {
    ++count[by_rem[at]];
    ++given;
  }
  for (size_t at = (size_t)K - 1; given > total_count; at = (at + (size_t)K - 1) % (size_t)K)
    if (count[by_rem[at]] > 0)
    {
      --count[by_rem[at]];
      --given;
    }
  for (int k = 0; k < K; ++k)
  {
    const double* p = poses_xyt + 3 * (size_t)kept[k];
    bpf_mixture_component& c = out[k];
    std::memset(&c, 0, sizeof(c));
    c.mean[0] = p[0];
    c.mean[1] = p[1];
    c.mean[2] = mixture_normalize_angle(p[2]);
    c.rotation[0] = c.rotation[4] = c.rotation[8] = 1.0;
    for (int q = 0; q < 3; ++q)
      c.sigma[q] = sigma[q];
    c.count = count[k];
    if (source_row_out)
      source_row_out[k] = kept[k];
    if (merged_out)
      merged_out[k] = merged[k];
  }
  *n_components_out = K;
  return BPF_OK;
}
