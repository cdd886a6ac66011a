// C-ABI: exhaustive pose search (include/badger_pf.h) -- every free cell x heading scored against one scan on the
// device, the best k kept.  Candidates are generated into the engine's candidate set window by window, scored by
// score_planar exactly as BPF_POSE_CHECK_SENSOR_MODEL scores its trial poses (set->converged = 0), and folded into a
// running best-k list by k_search_select / k_search_merge.  Every window is enqueued behind the one before; this
// thread waits once, for the k rows.  (score_planar stages the scan per call, so the scan is staged once per window:
// staging it once per search would mean taking the staging ring's slot handling out of score_planar, which every
// existing caller goes through.  A slot of the ring is reused after kRing windows, so the host may wait there for
// the window four back.)
//
// Read-only for the filter: the scoring call's bookkeeping (wc, evals_last, the diagnostics of the last launch) and
// last_status are saved and put back, as TrialScores::score does; nothing else it touches belongs to a set.
namespace
{
constexpr int kSearchWindow = 65536;  // candidates per window (bpf_pose_search_window)

static_assert(sizeof(bpf_pose_hit) == 56, "bpf_pose_hit is 56 bytes in every binding");
static_assert(kSearchWindow % kSearchTile == 0, "whole tiles per full window");

// ---- what a sharded search (abi_shard_search.inl) hands the four internal searches on its rank.  With it a search
// checks the whole range given, takes this rank's share of it, and hands its list -- left in d_search_best with its
// count -- to shard_search_finish instead of search_finish; the pruned forms share their tau behind the seed.  The
// single-engine entry points pass nullptr: finish, no hook.
struct SearchShard
{
  int rank = 0, world = 1;
  const unsigned long long* floor_key = nullptr;  // device word for prune_tau, set by shard_search_share_floor
};
// units [first + T r / W, first + T (r + 1) / W) of the T given: the convention of even_counts
void shard_search_share(int rank, int world, long long first, long long T, long long* my_first, long long* my_count)
{
  const long long lo = (T * rank) / world, hi = (T * (rank + 1)) / world;
  *my_first = first + lo;
  *my_count = hi - lo;
}
// abi_shard_search.inl: the ranks' K-th keys behind the seed into a floor on the device (enqueued, no wait) ...
int shard_search_share_floor(bpf_engine* e, SearchShard* sh, int k);
// ... whose exchange the host checks behind the wait for the survivor counts; and the ranks' lists gathered, folded
// on the device and fetched as rows
int shard_search_floor_arrived(bpf_engine* e, SearchShard* sh);
int shard_search_finish(bpf_engine* e, SearchShard* sh, const SearchSpace& S, int k, bpf_pose_hit* hits_out,
                        int* n_hits_out);

// arguments every entry point checks alike
int search_space_of(bpf_engine* e, int headings, int cell_stride, SearchSpace* S, long long* total)
{
  if (headings < 1 || cell_stride < 1)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: headings >= 1 and cell_stride >= 1 are needed");
  if (!e->have_map || !e->have_lut)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search needs the 2-D map and its distance LUT");
  HIPCHK(e, hipSetDevice(e->device));
  *S = SearchSpace{};
  int rc = ensure_free_list(e, cell_stride, &S->cells, &S->n_cells);
  if (rc != BPF_OK)
    return rc;
  S->headings = headings;
  S->size_x = e->map.size_x;
  S->size_y = e->map.size_y;
  S->origin_x = e->map.origin_x;
  S->origin_y = e->map.origin_y;
  S->resolution = e->map.resolution;
  *total = (long long)S->n_cells * (long long)headings;
  return BPF_OK;
}

// ---- the selection around the scoring, shared with the cloud search (abi_pose_search_cloud.inl)
// its buffers, for windows of up to kSearchWindow candidates, and the running best-k list emptied
int search_begin(bpf_engine* e)
{
  const int max_tiles = kSearchWindow / kSearchTile;
  HIPCHK(e, e->d_search_best.reserve(kSearchMaxK));
  HIPCHK(e, e->d_search_tiles.reserve((size_t)max_tiles * kSearchMaxK));
  HIPCHK(e, e->d_search_counts.reserve(1 + max_tiles));
  HIPCHK(e, e->d_search_hits.reserve(kSearchMaxK));
  HIPCHK(e, e->h_search_hits.reserve(kSearchMaxK));
  HIPCHK(e, e->h_search_count.reserve(1));
  HIPCHK(e, hipMemsetAsync(e->d_search_counts.p, 0, sizeof(int), e->stream));
  return BPF_OK;
}

// the scores of candidates c0 .. c0 + n - 1, as they stand in e->cand.w, folded into the running best-k list
int search_fold_window(bpf_engine* e, int n, long long c0, int k)
{
  int kp = 2;
  while (kp < k)
    kp <<= 1;
  const int tiles = blocks_for(n, kSearchTile);
  hipLaunchKernelGGL(k_search_select, dim3(tiles), dim3(kSearchThreads), 0, e->stream, (const double*)e->cand.w.p, n,
                     c0, k, (const SearchEntry*)e->d_search_best.p, (const int*)e->d_search_counts.p,
                     e->d_search_tiles.p, e->d_search_counts.p + 1);
  hipLaunchKernelGGL(k_search_merge, dim3(1), dim3(kSearchThreads), 0, e->stream, e->d_search_best.p,
                     e->d_search_counts.p, k, kp, (const SearchEntry*)e->d_search_tiles.p,
                     (const int*)(e->d_search_counts.p + 1), tiles);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "pose search selection launch");
  return BPF_OK;
}

// the list as rows for the caller: k_search_hits, the copy of the rows, and the call's wait for them
int search_finish(bpf_engine* e, const SearchSpace& S, int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  hipLaunchKernelGGL(k_search_hits, dim3(blocks_for(k, 256)), dim3(256), 0, e->stream,
                     (const SearchEntry*)e->d_search_best.p, (const int*)e->d_search_counts.p, S, e->d_search_hits.p);
  if (hipGetLastError() != hipSuccess)
    return e->fail(BPF_ERR_HIP, "k_search_hits launch");
  H2D_OR_RETURN(pinned_down(e, e->h_search_count, 0, e->d_search_counts, 0, 1, e->stream));
  H2D_OR_RETURN(pinned_down_sync(e, e->h_search_hits, 0, e->d_search_hits, 0, (size_t)k, e->stream));
  const int n_hits = std::max(0, std::min(e->h_search_count.p[0], k));
  std::memcpy(hits_out, e->h_search_hits.p, (size_t)n_hits * sizeof(bpf_pose_hit));
  *n_hits_out = n_hits;
  return BPF_OK;
}

int search_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count, double range_max,
                 int headings, int cell_stride, long long first, long long count, int k, bpf_pose_hit* hits_out,
                 int* n_hits_out, SearchShard* sh = nullptr)
{
  if (!hits_out || !n_hits_out || !ranges || !angles || range_count <= 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: a scan and an output are needed");
  if (k < 1 || k > kSearchMaxK)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: 1 <= k <= 1024");
  if (headings < 1 || cell_stride < 1)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose search: headings >= 1 and cell_stride >= 1 are needed");
  if (!e->pm.configured)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "pose search scores with the planar models: none is set");
  SearchSpace S;
  long long total = 0;
  int rc = search_space_of(e, headings, cell_stride, &S, &total);
  if (rc != BPF_OK)
    return rc;
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

  HIPCHK(e, e->cand.reserve((size_t)std::max<long long>(1, std::min<long long>(count, kSearchWindow))));
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
    if (e->pm.max_beams >= 2)  // (below that applyModelToSampleSet leaves the weight 1.0, planar_scanner.cpp:144-145)
    {
      bool forced_zero = false;
      rc = score_planar(e, e->cand.dev(), n, 0, ranges, angles, range_count, range_max, &forced_zero);
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

// the order of the result: score descending, equal scores by candidate, NaN behind every number
bool pose_hit_before(const bpf_pose_hit& a, const bpf_pose_hit& b)
{
  const bool a_nan = a.score != a.score, b_nan = b.score != b.score;
  if (a_nan != b_nan)
    return b_nan;
  if (!a_nan && a.score != b.score)
    return a.score > b.score;
  return a.candidate < b.candidate;
}
}  // namespace

int bpf_pose_search_window(void)
{
  return kSearchWindow;
}

int bpf_planar_search_space(bpf_engine* e, int headings, int cell_stride, long long* candidates_out,
                            int* free_cells_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  const int status = e->last_status;
  SearchSpace S;
  long long total = 0;
  const int rc = search_space_of(e, headings, cell_stride, &S, &total);
  e->last_status = status;
  if (rc != BPF_OK)
    return rc;
  if (candidates_out)
    *candidates_out = total;
  if (free_cells_out)
    *free_cells_out = S.n_cells;
  return BPF_OK;
}

int bpf_planar_search_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, int headings, int cell_stride, long long first, long long count,
                            int k, bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  // what the scoring calls reset describes the engine's set, not the candidates: put back, whatever the outcome
  const WeightCaches caches = e->wc;
  const long long evals = e->evals_last;
  const int status = e->last_status, form = e->last_score_form;
  const bool window_path = e->last_used_window_path;
  const int rc = search_poses(e, ranges, angles, range_count, range_max, headings, cell_stride, first, count, k,
                              hits_out, n_hits_out);
  e->wc = caches;
  e->evals_last = evals;
  e->last_status = status;
  e->last_score_form = form;
  e->last_used_window_path = window_path;
  return rc;
}

int bpf_pose_search_merge(const bpf_pose_hit* lists, const int* list_lengths, int n_lists, int k,
                          bpf_pose_hit* hits_out, int* n_hits_out)
{
  if (k < 1 || k > kSearchMaxK || n_lists < 0 || !hits_out || !n_hits_out || (n_lists > 0 && (!lists || !list_lengths)))
    return BPF_ERR_INVALID_ARGUMENT;
  size_t total = 0;
  for (int l = 0; l < n_lists; ++l)
  {
    if (list_lengths[l] < 0)
      return BPF_ERR_INVALID_ARGUMENT;
    total += (size_t)list_lengths[l];
  }
  std::vector<bpf_pose_hit> all(lists, lists + total);
  std::stable_sort(all.begin(), all.end(), pose_hit_before);
  const int n = (int)std::min<size_t>(total, (size_t)k);
  if (n > 0)
    std::memcpy(hits_out, all.data(), (size_t)n * sizeof(bpf_pose_hit));
  *n_hits_out = n;
  return BPF_OK;
}
