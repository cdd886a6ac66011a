// Engine state: device / pinned buffers, per-scan staging descriptors, the bpf_engine struct and the
// HIPCHK error macro.  Part of the one translation unit engine.hip.
#pragma once
#include "resample_plan.hpp"  // the resample drivers' shared arithmetic (host code, namespace bpf)

namespace
{

constexpr int kRing = 4;            // in-flight scan uploads
constexpr int kMaxBeams = 4096;     // beams staged in LDS per launch
// calc_range_skip forms j * 2 * dmin with a 24-bit multiply whose 32-bit result must not wrap: j <= c + 2,
// dmin <= c + 1 for a ray of c = range_max / resolution cells -> 2 (c + 2)(c + 1) < 2^31 <=> c <= 32 765
constexpr double kMaxRayCells = 32760.0;
constexpr int kTableLdsMax = 2048;  // table entries that still go to LDS
constexpr int kEventPool = 8192;
constexpr int kSeamMaxChunks = 8;
constexpr int kSeamMaxBlocks = 4096;
// the pinned scratch of small_down (host_copy.hpp): its largest caller fetches one weight sum per rank
constexpr size_t kSmallResultBytes = kMailboxMaxWorld * sizeof(double);

// Device / pinned buffers free themselves with the engine (bpf_destroy selects the device first).
template <typename T>
struct DevBuf
{
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n)
  {
    if (n <= cap)
      return hipSuccess;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t r = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (r == hipSuccess)
      cap = n;
    return r;
  }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

template <typename T>
struct PinnedBuf
{
  T* p = nullptr;
  size_t cap = 0;
  // fine-grained (hipHostMallocCoherent): a kernel's plain stores are written through to host memory.  The default
  // allocation is coarse-grained on this platform: plain stores may stay in the GPU's L2s until a system-scope
  // release -- the END of a kernel is not one when another kernel follows in the queue -- so data that the host reads
  // behind a flag word (and not behind a stream synchronisation) must not live in a default allocation.
  bool coherent = false;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  hipError_t reserve(size_t n)
  {
    if (n <= cap)
      return hipSuccess;
    if (p)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t r = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T),
                                 coherent ? hipHostMallocCoherent : hipHostMallocDefault);
    if (r == hipSuccess)
      cap = n;
    return r;
  }
  void release()
  {
    if (p)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct SampleSet
{
  DevBuf<double> x, y, th, w;
  ParticlesDev dev() { return ParticlesDev{ x.p, y.p, th.p, w.p }; }
  hipError_t reserve(size_t n)
  {
    hipError_t r;
    if ((r = x.reserve(n)) != hipSuccess) return r;
    if ((r = y.reserve(n)) != hipSuccess) return r;
    if ((r = th.reserve(n)) != hipSuccess) return r;
    return w.reserve(n);
  }
  void release()
  {
    x.release(); y.release(); th.release(); w.release();
  }
};

struct PlanarModel
{
  bool configured = false;
  int model = BPF_MODEL_LIKELIHOOD_FIELD;
  int max_beams = 0;
  double z_hit = 0, z_short = 0, z_max = 0, z_rand = 0, sigma_hit = 0, lambda_short = 0;
  GompertzDev g{ 0, 0, 0, 0, 0, 0 };
  int do_beamskip = 0;
  double beam_skip_distance = 0, beam_skip_threshold = 0, beam_skip_error_threshold = 0;
  double off_map_factor = 1.0, non_free_factor = 1.0, non_free_radius = 0.0;  // planar_scanner.cpp:42-44
  double pose[3] = { 0, 0, 0 };
  // the prob model's beam skipping (a counting pass, the mask, then the kept beams) runs only on a converged set
  bool beamskip_armed(bool converged) const
  {
    return model == BPF_MODEL_LIKELIHOOD_FIELD_PROB && do_beamskip && converged;
  }
};

struct ScanSlot
{
  PinnedBuf<unsigned char> host;
  DevBuf<unsigned char> dev;
  hipEvent_t done = nullptr;
  bool pending = false;
};

// host-side description of one staged scan (see stage_field_scan)
struct FieldScan
{
  int n_valid = 0;             // beams that pass the range_max / NaN tests
  int n_staged = 0;            // of those, the ones uploaded (all, or the kept ones of beam skipping)
  bool copy_pending = false;   // pinned staging not yet copied to the device slot
  bool ranges_staged = false;  // the pinned slot holds the decimated ranges (8 B per beam), not the end points: the
                               // prep launch forms them (copy_pending says whether that is still to come)
  int step = 1;                // decimation: staged beam k has bearing k * step
  int n_always_off = 0;        // valid beams too long / non-finite to stage: off the map for every pose
  double off_map_term = 0.0;   // table[K]
  int n_slots = 0;             // beam_ind range of the prob model
  std::vector<int> slot_of;    // staged beam -> beam_ind
  size_t beams_off = 0, bytes = 0;  // the beams in the slot (the term table is e->d_term_table)
  int table_len = 0;
};

// where a host-out scoring launch (the host-buffer seam, abi_planar.inl) leaves its results
struct FieldHostOut
{
  double4* rec;      // non-null: HOST_RECORDS -- the caller's records in registered host memory, read and written in place
  double* w_host;    // HOST_WEIGHTS: the weights go to this pinned array as well
  double* total_host;
  double* partials;  // >= blocks of the launch
  unsigned long long* flag;  // the done word and the value k_seam_done publishes in it
  unsigned long long value;
};

// what one launch_field call is asked for (host_scoring.inl); the defaults are the plain scoring of a resident set
struct FieldRequest
{
  int* obs_count = nullptr;    // non-null: the counting pass of beam skipping (per-beam counts, no weights) ...
  int skip_level = 0;          // ... of the end points in a LUT level below this one
  bool want_partials = false;  // leave per-block weight partials for the normalise launch (wc.fused_partials)
  const double4* aos = nullptr;  // non-null: the n particles are still 32-byte records there (device-visible memory);
                                 // the prep launch unpacks them into `p` as it goes (k_field_prep_aos)
  const FieldHostOut* host_out = nullptr;  // non-null: a host-out form of the scoring kernel
  const uint16_t* bound_tiles = nullptr;   // non-null: the bound pass of the pruned pose search -- the kernel gathers
                                           // from this image (the layout of lut_tiles) under neutral map factors
};

// What the last weight pass left behind for the passes that follow it.  Invariant: a field that is set describes the
// weights of the CURRENT set (sets[cur].w, sample_count of them) as they are now; whoever rewrites weights -- of any
// set, the buffers are shared -- drops them first (bpf_engine::weights_overwritten and the transitions on top of it),
// and only the launch that produced a buffer sets its field.  cdf_guide_valid is not dropped: it is read only behind
// a build_cdf that has either found cdf_ready_n set by the producer of both or rewritten it.  shard_cdf_valid goes
// with the CDF it describes: a single-filter update that leaves a CDF of its own for the same n must not be taken
// for the sharded one (its sum is not in scalars[7]).
struct WeightCaches
{
  int fused_partials = 0;        // > 0: the last scoring launch left that many per-block weight partials
  int tile_sums_n = -1;          // >= 0: d_tile_sums holds the 2048-tile sums of the current weights for that n
  int cdf_ready_n = -1;          // >= 0: d_cdf (and the guide) already hold the CDF of the current weights for that n
  int cdf_coarse_n = -1;         // >= 0: d_cdf_coarse holds the subsample of the CDF in d_cdf for that n
  bool cdf_guide_valid = false;  // d_cdf_guide holds head starts for the bisection of d_cdf
  bool shard_cdf_valid = false;  // k_normalize_gathered_cdf left the local CDF of the current weights behind
  void drop()
  {
    fused_partials = 0;
    tile_sums_n = cdf_ready_n = cdf_coarse_n = -1;
    shard_cdf_valid = false;
  }
  // k_normalize_cdf / k_normalize_gathered_cdf: the normalised weights' CDF and its subsample (the tile sums went
  // into them); `sharded`: it is the local CDF a bpf_shard_build_cdf may take
  void cdf_left(int n, bool guide, bool sharded = false)
  {
    tile_sums_n = -1;
    cdf_ready_n = cdf_coarse_n = n;
    cdf_guide_valid = guide;
    if (sharded)
      shard_cdf_valid = true;
  }
  // k_normalize_fused / k_normalize_gathered: the tile sums of the normalised weights, for build_cdf to scan
  void tile_sums_left(int n) { tile_sums_n = n; }
  // build_cdf's scan kernels are about to write d_cdf: they leave no subsample, and the guide unless they run serially
  void cdf_scan_begins(bool guide)
  {
    cdf_coarse_n = -1;
    cdf_guide_valid = guide;
  }
  // the local CDF was taken by bpf_shard_build_cdf, or this normalisation / this init leaves none
  void shard_cdf_dropped() { shard_cdf_valid = false; }
};

// Leaf and bin counts of the histogram tree of the current set (of the GLOBAL set on a sharded filter).  Invariant:
// tree_pending means the counts are -1 and ensure_set_tree builds them before anybody reads them; -1 without
// tree_pending means nobody has supplied them (a set adopted with a leaf count only, a sharded init before its
// bpf_shard_tree_* stage).  Otherwise they are the counts of the set that is current NOW.
struct TreeCounts
{
  int leaf_count = 0, bin_count = 0;
  int gt_route = 0;           // BPF_SHARD_TREE_ROUTE_* of the counts installed last (0: none since the last init)
  bool tree_pending = false;  // the current set's histogram tree (leaf / bin counts) has not been built yet
  TreeCounts counted(int leaf, int bins) const { return TreeCounts{ leaf, bins, gt_route, false }; }
  TreeCounts pending() const { return TreeCounts{ -1, -1, gt_route, true }; }
};

}  // namespace

#define HIPCHK(e, call)                          \
  do                                             \
  {                                              \
    hipError_t _r = (call);                      \
    if (_r != hipSuccess)                        \
      return (e)->fail_hip(_r, #call);           \
  } while (0)

struct bpf_engine
{
  int device = 0;
  int n_cu = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string last_error;

  // ---- 2-D map
  bool have_map = false, have_lut = false;
  MapDev map{};
  int map_version = 0;
  std::vector<int8_t> h_cells8;
  std::vector<float> h_levels;
  DevBuf<uint16_t> d_lut_tiles;
  DevBuf<uint32_t> d_cheb;
  DevBuf<int8_t> d_cells8;
  DevBuf<float> d_levels;
  DevBuf<float> d_lut_f32;
  DevBuf<int> d_edt_tmp;

  // ---- planar scanner
  PlanarModel pm;
  ScanSlot ring[kRing];
  int ring_next = 0;
  // host-side caches of scan staging: cos/sin of the bearings (a sensor's bearings are the same
  // arithmetic sequence scan after scan, node_2d.cpp:559) and the per-level term table (depends
  // only on the model parameters, range_max and the map)
  std::vector<double> trig_angles, trig_cos, trig_sin;
  std::vector<double> term_table;
  // their device copies: cos then sin, rc doubles each (for the prep launch that forms the end points itself), and the
  // term table every scoring launch reads; uploaded in stream order when the host cache changes
  DevBuf<double> d_trig, d_term_table;
  bool trig_on_device = false, term_on_device = false;
  bool stage_on_host = false;  // BPF_OPT_STAGE_ON_HOST: the end points always formed by the host
  struct TermKey
  {
    int model = -1, map_version = -1;
    double z_hit = 0, z_rand = 0, sigma = 0, range_max = 0;
    bool operator==(const TermKey& o) const
    {
      return model == o.model && map_version == o.map_version && z_hit == o.z_hit && z_rand == o.z_rand &&
             sigma == o.sigma && range_max == o.range_max;
    }
  } term_key;
  DevBuf<int> d_obs_count;
  FieldScan skip_fs;          // staging of the counting pass of beam skipping, kept for its second half
  bool skip_pending = false;
  // LDS-window scoring path
  DevBuf<double4> d_prep;
  DevBuf<double> d_prep_stats, d_chunk_partials;
  DevBuf<WindowPlan> d_plan;
  std::vector<const void*> dynamic_lds_set;  // kernels whose dynamic LDS limit has been raised (ensure_dynamic_lds)
  bool graded_shares = true;    // BPF_OPT_GRADED_SHARES
  DevBuf<int> d_beam_counter;   // work counter of k_score_beam
  bool window_enabled = false;  // measured: no gain on wide clouds; opt-in via BPF_OPT_WINDOW_PATH
  bool last_used_window_path = false;
  DevBuf<unsigned long long> d_cells_walked;

  // ---- 3-D map + point-cloud scanner
  bool have_map3d = false;
  Map3dDev map3{};
  double map3_max_dist = 0.0;
  int map3_version = 0;  // bumped by bpf_map3d_set: what is cached per 3-D map compares it
  DevBuf<uint32_t> d_pose_indices;
  DevBuf<uint8_t> d_ratios, d_dense3d;
  bool lut_host = false;      // BPF_OPT_LUT_HOST: the 3-D LUT builder on the host
  int lut3d_generations = 0;  // FIFO generations the device builder ran (0: host)
  bool cloud_dense = true;   // BPF_OPT_CLOUD_DENSE: use the dense tiled volume when there is one
  size_t n_pose_indices = 0, n_ratios = 0;
  bool cloud_configured = false;
  int cloud_max_beams = 0;
  double cloud_z_hit = 0, cloud_z_rand = 0, cloud_sigma = 0;
  CloudModelDev cm{};
  DevBuf<float> d_affine, d_points;
  DevBuf<double> d_cloud_partials, d_cloud_table;
  PinnedBuf<float> h_points;
  PinnedBuf<double> h_cloud_table;

  // ---- particle filter
  bool have_pf = false;
  int min_samples = 0, max_samples = 0;
  double alpha_slow = 0, alpha_fast = 0, conv_threshold = 0;
  double pop_err = 0.01, pop_z = 3, dist_threshold = 0.5;  // particle_filter.cpp:58-60
  int resample_model = BPF_RESAMPLE_MULTINOMIAL;
  uint64_t rng = 0;  // glibc's unseeded drand48 state
  LcgJump jump{};
  SampleSet sets[2];
  int cur = 0;
  int sample_count = 0;
  WeightCaches wc;
  TreeCounts tree;
  int converged = 0;
  float percent_converged = 0;
  bool converged_pending = false;
  int conv_n = 0;
  double w_diff_last = 0;
  int last_status = BPF_OK;
  // the last single-engine resample, as bpf_pf_get_state reports it (written by bpf_pf_update_resample alone)
  int resample_windows = 0;
  int resample_counted_by = 0;  // ResampleCountedBy: 0 host tree, 1 device tree, 2 one-block kernel
  int window_hint = 4096;
  long long evals_last = 0;
  bool cdf_serial = false;
  bool count_cells = false;
  KdHistogram hist;
  SeenKeys seen;
  DevBuf<int> d_cdf_guide;     // head start for the CDF bisection (k_scan_final / cdf_find_guided)
  DevBuf<double> d_cdf, d_partials, d_targets, d_block_partials, d_tile_sums;
  DevBuf<unsigned long long> d_tile_slots;  // k_normalize_cdf's look-back slots, [2][256]
  unsigned tile_generation = 0;
  bool fused_resample = true; // BPF_OPT_FUSED_RESAMPLE
  bool fused_lds_tree = false; // BPF_OPT_FUSED_LDS_TREE: the LDS form of the <= 64-key tree (tests)
  bool lut_exact_edt = false; // BPF_OPT_LUT_EXACT_EDT: implicit LUT builds take the device EDT instead of the reference's brushfire
  bool kld_persistent = false;         // BPF_OPT_KLD_PERSISTENT: the device tree in one launch when its grid is resident
  int kld_generation = 0;
  int kld_persist_blocks_per_cu = -1;  // occupancy of k_kld_tree_persistent (-1: not asked yet)
  DevBuf<unsigned> d_kld_bar;
  void* shard_cdf_flags = nullptr;     // the caller's miss flag that launch cleared (null: none)
  void* shard_flags_last = nullptr;    // flags_dev of the last bpf_shard_build_cdf
  int fused_generation = 0;
  PinnedBuf<int> h_fused;
  DevBuf<FusedJump> d_fused_jump;
  DevBuf<unsigned long long> d_fused_keys;
  DevBuf<unsigned> d_fused_counter;
  DevBuf<double> d_cdf_coarse;
  DevBuf<FilterScalars> d_scalars;
  DevBuf<int> d_keys, d_src_index, d_flags;  // d_flags[0] miss, [1] converged count
  DevBuf<double4> d_aos;
  PinnedBuf<int> h_keys;
  PinnedBuf<unsigned> h_done;
  unsigned done_generation = 0;
  bool zero_copy_keys = true;
  PinnedBuf<double> h_targets;
  hipEvent_t targets_read = nullptr;  // recorded after the sharded systematic window kernel
  PinnedBuf<int> h_flags;
  PinnedBuf<FilterScalars> h_scalars;
  PinnedBuf<double4> h_aos;
  SampleSet scratch;  // Seam A host-buffer path
  SampleSet snap;
  int snap_count = 0, snap_leaf = 0, snap_bins = 0;
  int snap_kld_mode = 0;  // the KLD count mode snap_leaf was counted in

  // ---- w_diff > 0: random free-space poses (Node::randomFreeSpacePose) and the draw chain
  int random_pose_mode = BPF_RANDOM_POSE_NONE;
  std::vector<float> h_lut_f32;     // the LUT as floats (free-space test: distance > non_free_space_radius)
  DevBuf<int2> d_free_ij;
  int n_free = 0;
  int free_map_version = -1;
  double free_radius = -1.0;
  double shard_w_diff = 0.0;        // of the sharded resample in progress (bpf_shard_begin_resample)
  bool shard_chain = false;         // its draw chain is in d_chain
  int shard_n_random = 0;           // systematic: random poses at the head of the new set
  int shard_retries = 0;            //   and the trials each of their calls rejected
  uint64_t shard_rng0 = 0;
  DevBuf<uint64_t> d_chain_bits;
  DevBuf<int> d_chain_cnt, d_chain_exit, d_chain_entry, d_chain_base, d_chain;
  PinnedBuf<int> h_chain_word;
  // Node::uniformPoseGenerator's score check (bpf_pf_set_uniform_pose_check): rejected trials per call, the same for
  // every call in BPF_POSE_CHECK_AS_REFERENCE; -1 = the threshold table does not reach 1.0 within 2^30 trials
  double pose_check_g0 = 0.0, pose_check_m = 0.0;
  int pose_check_scoring = BPF_POSE_CHECK_AS_REFERENCE;
  int pose_retries = 0;
  // BPF_POSE_CHECK_SENSOR_MODEL: the last scan given to bpf_pf_update_sensor_planar (cleared by bpf_map2d_set, as the
  // node clears latest_scan_data_, node_2d.cpp:217), the candidate set it scores and the resolved accept positions
  bool have_scan = false;
  std::vector<double> scan_ranges, scan_angles;
  double scan_range_max = 0.0;
  SampleSet cand;
  DevBuf<unsigned> d_accept;
  std::vector<unsigned> h_accept;
  std::vector<int> h_chain;
  std::vector<double> h_cand_scores;

  // ---- mailbox exchange of the sharded path (kernels_mailbox.hpp, abi_mailbox.inl)
  struct Mailbox
  {
    bool active = false;            // created AND connected
    int rank = 0, world = 0;
    long long max_window = 0;
    size_t bytes = 0;
    char* own = nullptr;            // this engine's mailbox (uncached device memory, exported by IPC handle)
    char* peer[kMailboxMaxWorld] = {};
    bool opened[kMailboxMaxWorld] = {};
    unsigned long long tot_gen = 0; // generation of the last totals post
    unsigned long long win_gen = 0; // generation of the window handed out last
    bool win_wait = false;          // that window's columns are in flight: its first consumer kernel has to wait
    unsigned long long hello = 0;
    int fold_deferred = 0;          // > 0: that many scoring partials wait to be folded and posted by the normalise launch
    unsigned long long gen_base = 0; // tot_gen + win_gen when the set-up ended (bpf_shard_exchange_count starts there)
  } mb;
  int shard_rank = 0, shard_world = 1;  // of the shard exchange in use (mailbox or collective)
  // ---- RCCL collectives (libbadger_pf_rccl.so, loaded by bpf_shard_bootstrap when the mailbox cannot be used)
  struct Collective
  {
    bool active = false;
    bool local = false;             // fn is the in-process table of abi_shard_local.inl, comm a seat of its world
    void* lib = nullptr;
    void* comm = nullptr;
    struct Fn
    {
      const char* (*last_error)() = nullptr;
      int (*unique_id_bytes)() = nullptr;
      int (*unique_id)(void*) = nullptr;
      int (*init)(void**, int, int, const void*) = nullptr;
      int (*destroy)(void*) = nullptr;
      int (*allgather_f64)(void*, const double*, double*, size_t, void*) = nullptr;
      int (*allreduce_sum_i64)(void*, long long*, size_t, void*) = nullptr;
      int (*allreduce_sum_i32)(void*, int*, size_t, void*) = nullptr;
      int (*allgather_i64)(void*, const long long*, long long*, size_t, void*) = nullptr;
    } fn;
    DevBuf<double> totals;
    DevBuf<long long> window[2];
    int window_turn = 0;
    DevBuf<long long> send, recv;       // a ragged all-gather, padded to the largest contribution
    unsigned long long exchanges = 0;   // collectives issued since the communicator was made
  } coll;
  // ---- the one-call sharded forms that do their own exchanges (abi_shard_node.inl)
  DevBuf<long long> d_x_words, d_x_gather;  // a few words (counts, flags) and their gathered form; gathered payloads
  PinnedBuf<long long> h_x_words;
  long long ss_global_epoch = -1;   // set_epoch for which bpf_shard_compute_cluster_stats installed the GLOBAL figures
  int ss_route = 0;                 //   and the route it took (BPF_SHARD_STATS_ROUTE_*)
  DevBuf<int> d_shard_flags;        // the CDF-miss flag word of the one-call sharded updates
  void* mb_totals = nullptr;        // bpf_shard_mailbox_update_sensor_planar: this update's totals (mailbox slots)
  bool mb_totals_valid = false;
  DevBuf<double> d_shard_out;       // [3][max_samples] poses of a resample that spans several windows
  PinnedBuf<unsigned> h_mb_error;
  DevBuf<unsigned> d_mb_error;
  int mb_timeout_ms = 5000;
  PinnedBuf<int> h_mb_result;
  DevBuf<unsigned> d_mb_counter;

  // ---- the particle-cloud message formed on the device (kernels_pose_array.hpp, abi_pose_array.inl): buffers of
  // their own, so that a query between two updates disturbs nothing another stage has left behind
  DevBuf<long long> d_pa_rows;      // int64[3][n_sel]: this slice's selected x / y / theta bits
  DevBuf<long long> d_pa_gather;    // int64[3][count]: every rank's rows in global order
  DevBuf<double> d_pa_out;          // double[count][7]: the formed poses on their way to the host

  // ---- exhaustive pose search (kernels_pose_search.hpp, abi_pose_search.inl): the strided free list F_s, cached per
  // (map version, radius, stride) like d_free_ij (stride 1 is d_free_ij itself), and the selection's buffers.  The
  // candidate poses live in `cand`; nothing here describes the particle set
  DevBuf<int2> d_free_s;
  int n_free_s = 0;
  int free_s_map_version = -1, free_s_stride = 0;
  double free_s_radius = -1.0;
  DevBuf<SearchEntry> d_search_best;   // [kSearchMaxK] the running best-K list, best first
  DevBuf<SearchEntry> d_search_tiles;  // [tiles of a window][k] what every block of k_search_select kept
  DevBuf<int> d_search_counts;         // [0] entries in d_search_best, [1 ...] per tile
  DevBuf<bpf_pose_hit> d_search_hits;  // [kSearchMaxK] the rows on their way to the host
  PinnedBuf<bpf_pose_hit> h_search_hits;
  PinnedBuf<int> h_search_count;
  // the sharded search (abi_shard_search.inl): a list travels as K + 1 entries, a header (count, 0) and K rows
  DevBuf<SearchEntry> d_shard_lists;         // [K + 1] this rank's packed list, then [world][K + 1] the gathered ones
  DevBuf<unsigned long long> d_shard_floor;  // [0] this rank's K-th key, [1] the floor, [2 ...] the W gathered keys

  // ---- joint pose search (kernels_pose_search_joint.hpp, abi_pose_search_joint.inl): cos / sin of the call's
  // headings, the S clouds of a cloud call as float SoA one behind the other, and the candidates of a diagnostic call
  DevBuf<double> d_joint_table;  // [2][H]: C_h, then S_h
  PinnedBuf<double> h_joint_table;
  DevBuf<float> d_joint_points;  // per scan [3][n_points_s]
  PinnedBuf<float> h_joint_points;
  DevBuf<long long> d_joint_ids;

  // ---- pruned pose search (kernels_pose_search_pruned.hpp, abi_pose_search_pruned.inl): one pooled image per
  // (map version, B) and one block list per (map version, radius, stride, B), a slot per allowed B (log2 B - 1), so
  // that calls with different B do not evict each other; then the working arrays of a call
  struct PrunePool
  {
    DevBuf<uint16_t> tiles;  // P_B in the layout of d_lut_tiles
    int map_version = -1;
  } prune_pool[6];
  DevBuf<uint16_t> d_prune_rows;  // the row pass of a pooled image under construction, padded row-major
  struct PruneList
  {
    DevBuf<int> start, member;  // CSR over F_s
    DevBuf<int2> anchor;
    std::vector<int> h_start;
    int n_blocks = 0, max_members = 0;
    int map_version = -1, stride = 0;
    double radius = -1.0;
  } prune_list[6];
  DevBuf<double> d_prune_bounds;        // [block candidates of the call]
  DevBuf<uint8_t> d_prune_in_seed;      // [block candidates of the call]
  DevBuf<SearchEntry> d_prune_best;     // [kSearchMaxK] the best bounds, ids = block candidates of the call
  DevBuf<int> d_prune_best_count;       // [1]
  DevBuf<int> d_prune_seed;             // [1024] seed_q, [1025] seed_off behind it
  DevBuf<long long> d_prune_ids;        // [window] candidate of every slot, -1 for an empty one
  DevBuf<int> d_prune_surv;             // [chunks * 1024] surv_q, then as many surv_off
  DevBuf<uint8_t> d_prune_state;        // [chunks * 1024] per survivor: 0 undecided, 1 dropped, 2 expanded
  DevBuf<int2> d_prune_chunks;          // [chunks] (survivors, their members)
  DevBuf<long long> d_prune_chunk_off;  // [chunks + 1] members before a chunk, from the host
  DevBuf<unsigned long long> d_prune_words;  // [kPruneWords]
  PinnedBuf<int2> h_prune_chunks;
  PinnedBuf<long long> h_prune_chunk_off;
  PinnedBuf<unsigned long long> h_prune_words;
  // the 3-D form (kernels_pose_search_cloud_pruned.hpp, abi_pose_search_cloud_pruned.inl): one pooled volume per
  // (3-D map version, B), as large as Map3dDev::dense and reserved on first use, and one block list per (3-D map
  // version, stride, B) -- per-axis arrays and per-block starts and anchors, never per column
  struct PrunePool3
  {
    DevBuf<uint8_t> vol;  // P_B in the layout of d_dense3d
    int map3_version = -1;
  } prune_pool3[6];
  DevBuf<uint8_t> d_prune_rows3;  // the row pass of some planes of a pooled volume under construction
  struct PruneRect
  {
    DevBuf<int> start, axis_i, axis_j;
    DevBuf<int2> anchor;
    std::vector<int> h_start;
    int n_blocks = 0, nbj = 0, max_members = 0;
    int map3_version = -1, stride = 0;
  } prune_rect[6];

  // ---- pose refinement (kernels_pose_refine.hpp, abi_pose_refine.inl): the centres of the descent and what
  // k_refine_select keeps per pose.  The lattice poses live in `cand`; nothing here describes the particle set
  DevBuf<double> d_refine_centres;  // [n_poses][3] x, y, theta: the input poses, then every level's choice
  DevBuf<double> d_refine_score;    // [n_poses] score of the centre, from the last level
  DevBuf<double> d_refine_score_in; // [n_poses] score of the input pose
  DevBuf<int> d_refine_moved;       // [n_poses]
  DevBuf<int> d_refine_trace;       // [n_poses][levels] the m chosen
  DevBuf<bpf_pose_refined> d_refine_rows;
  PinnedBuf<double> h_refine_in;    // the input poses on their way up
  PinnedBuf<bpf_pose_refined> h_refine_rows;
  PinnedBuf<int> h_refine_trace;

  // ---- pose moments (kernels_pose_moments.hpp, abi_pose_moments.inl): the poses go up through h_refine_in into
  // d_refine_centres, as a refinement's do
  DevBuf<bpf_pose_moments> d_moments_rows;
  PinnedBuf<bpf_pose_moments> h_moments_rows;
  PinnedBuf<double> h_moments_scores;  // [n_poses][M], only for a call with scores_out

  // ---- KLD stop rule on the device (long draw streams)
  int kld_device_min = 8192;  // draws left after the first window from which the device tree takes over
  int kld_count_mode = BPF_KLD_COUNT_LEAVES;  // bpf_pf_set_kld_count: what the stop rule's k counts
  int kld_host_bins = 0;  // BINS mode: distinct keys the host replay has seen (e->seen first occurrences)
  DevBuf<unsigned long long> d_kld_hkey;
  DevBuf<int> d_kld_htmin, d_kld_slot, d_kld_cur, d_kld_first, d_kld_child, d_kld_flags, d_kld_limit;
  DevBuf<int2> d_kld_delta, d_kld_tiles, d_kld_counts;
  // the tree in LDS-sized pieces (kernels_kld2.hpp)
  DevBuf<int> d_kld2_int;       // tkeys[n] bucket[n] bk[n] cnt[N] off[N + 1] fill[N] n_tkeys n_top status[2]
  DevBuf<Kld2Top> d_kld2_top;
  DevBuf<unsigned long long> d_kld2_slots;  // look-back slots of k_kld2_scan
  bool kld_local = true;        // BPF_OPT_KLD_LOCAL
  // the histogram tree's hash tables were left in their start state behind the last build (pieces form): table size,
  // buffers and capacities they were cleared at (0: not clean)
  unsigned kld_clean_table = 0;
  const void* kld_clean_key = nullptr;
  const void* kld_clean_tmin = nullptr;
  size_t kld_clean_cap = 0;
  int kld_last_form = 0;        // diagnostics: 2 = LDS pieces, 1 = level loop, 3 = persistent, 4 = bin count
  PinnedBuf<int> h_kld;
  std::vector<int> kld_limit_host;
  double kld_limit_key[4] = { -1, -1, -1, -1 };  // pop_err, pop_z, min_samples, max_samples of the cached table

  // ---- motion model
  int odom_model = BPF_ODOM_MODEL_DIFF;
  double odom_alpha[5] = { 0, 0, 0, 0, 0 };
  bool odom_configured = false;
  DevBuf<int> d_motion_counts;
  DevBuf<long long> d_motion_offsets, d_motion_result;
  DevBuf<double> d_gauss, d_init_rot;
  DevBuf<double> d_mixture;  // the mixture initialiser's component rows, then its count prefix (abi_mixture.inl)
  PinnedBuf<long long> h_motion_result;

  // ---- cluster statistics on the device (kernels_stats.hpp)
  bool stats_host = false;          // BPF_OPT_STATS_HOST: the bit-exact host evaluation instead
  bool stats_on_device = false;     // the current statistics came from the device
  bool stats_own_set = false;       // ... and describe this engine's own set (not a sharded filter's global one)
  bool stats_clusters_fetched = false;
  int stats_cluster_count = 0, stats_best = -1;
  double stats_best_weight = 0.0, stats_best_pose[3] = { 0, 0, 0 };
  DevBuf<int> d_stats_parent, d_stats_label, d_stats_root, d_stats_tiles, d_stats_flags;
  DevBuf<long long> d_stats_hi;
  DevBuf<unsigned long long> d_stats_lo;
  DevBuf<bpf_cluster> d_stats_clusters;
  DevBuf<StatsResult> d_stats_result;
  PinnedBuf<StatsResult> h_stats_result;
  PinnedBuf<int> h_stats_flags;
  PinnedBuf<int> h_stats_block;     // k_stats_block: [0] generation, [1] status, [4 ..] StatsResult
  int stats_generation = 0;

  // ---- cluster statistics of a sharded set (kernels_shard_stats.hpp, abi_shard_stats.inl)
  int ss_stage = 0;                 // 0 none, 1 local bins listed, 2 bins merged and labelled, 3 local sums exported
  bool ss_finish_installed = false; // the last bpf_shard_stats_finish_dev installed its result (the sums fitted)
  long long ss_epoch = -1;          // set_epoch the stages in progress belong to
  int ss_clusters = 0;              // global cluster count (stage 2)
  unsigned ss_gmask = 0;            // global bin table size - 1 (stage 2)
  DevBuf<long long> d_ss_bins, d_ss_limbs;
  DevBuf<unsigned long long> d_ss_gkey, d_ss_parent;
  DevBuf<int> d_ss_gtmin, d_ss_eslot, d_ss_eroot, d_ss_label, d_ss_binlabel;
  DevBuf<double> d_ss_w;

  // ---- the GLOBAL set's histogram tree from the ranks' bin lists (kernels_shard_init.hpp, abi_shard_init.inl)
  DevBuf<long long> d_gt_bins;      // [2][bins] this slice's list: packed keys, global first indices
  DevBuf<unsigned long long> d_gt_key;
  DevBuf<int> d_gt_tmin, d_gt_eslot, d_gt_tiles, d_gt_flags;
  PinnedBuf<int> h_gt_flags;

  // ---- the systematic resample of a sharded set in place (kernels_shard_inplace.hpp, abi_shard_inplace.inl)
  int shard_form = BPF_SHARD_RESAMPLE_WINDOW;       // bpf_shard_set_resample_form
  double shard_max_share = 2.0;                     //   and its imbalance cap
  int shard_form_used = BPF_SHARD_RESAMPLE_WINDOW;  // of the last resample
  long long slice_first = -1;       // global index of this slice's first sample as the last init / resample left it
  long long slice_global = 0;       //   (-1: nobody has told the engine) and the samples of the whole set
  int ip_stage = 0;                 // 0 none, 1 selected, 2 sums exported, 3 counted
  long long ip_epoch = -1;          // set_epoch the stages in progress belong to
  DevBuf<long long> d_ip_words;     // [kInplaceSumWords] limbs + flag, [16] the count, [24 .. 25] / [26 .. 27] / [28 .. 29] acc hi / top / lo
  int ip_counts[kMailboxMaxWorld] = { 0 };  // every rank's new count of the last one-call in-place resample

  // ---- the multinomial resample of a sharded set in place (kernels_shard_inplace_mn.hpp, abi_shard_inplace_mn.inl)
  int shard_mn_form = BPF_SHARD_RESAMPLE_WINDOW;    // bpf_shard_set_multinomial_form
  // ip_stage of its stage calls: -1 selected, -2 bin list formed; the stop stage commits and leaves ip_stage = 1
  struct MnStage
  {
    int rank = 0, world = 0;
    int n_kept = 0;                      // candidates this rank keeps (the stop rule truncates them)
    double edge[kMailboxMaxWorld + 1];   // the slices of the global CDF
    void* flags_dev = nullptr;           // the caller's miss flag
  } mn;
  DevBuf<int> d_mn_idx;             // [max] draw index of every kept candidate, ascending
  DevBuf<int> d_mn_mark;            // [max] list entry whose key first occurs at a draw
  DevBuf<int> d_mn_t;               // [bins] first draw index of the merged keys, ascending (beside d_keys)
  DevBuf<int> d_mn_tiles;           // [tiles] of the select and of the mark compaction
  DevBuf<int> d_mn_words;           // [0] first miss, [1] stop j, [2 .. 4] M / leaf / bins, [5] check, [8 .. 23] owner counts, [24] scratch

  // ---- rebalancing the slices of a sharded set (kernels_shard_rebalance.hpp, abi_shard_rebalance.inl)
  int shard_rebalance = BPF_SHARD_REBALANCE_OFF;    // bpf_shard_set_rebalance
  double shard_trigger_share = 1.5;                 //   a policy condition, not a measurement
  RebalancePlan rb_plan;            // bpf_shard_rebalance_plan's record
  int rb_rank = -1;                 //   for this rank (-1: none)
  long long rb_epoch = -1;          //   of the set with this set_epoch
  long long rb_last_moved = 0;      // T of the last rebalance that completed (bpf_shard_rebalance_last)
  bool resample_committed = false;  // the last one-call sharded resample made its new set current (even when the AUTO
                                    //   rebalance behind it then failed): bpf_shard_resample_committed
  DevBuf<long long> d_rb_rows;      // int64[4][out[rank]]: this rank's outgoing samples
  DevBuf<long long> d_rb_gather;    // int64[4][T]: every rank's, compact (the one-call form)

  // ---- cluster statistics (host, lazy)
  std::vector<bpf_cluster> clusters;
  double set_mean[3] = { 0, 0, 0 }, set_cov[5] = { 0, 0, 0, 0, 0 };
  long long stats_epoch = -1;   // value of set_epoch the statistics were computed for
  long long set_epoch = 0;      // bumped whenever the current set's poses / weights change
  bool hist_matches_set = false;

  // ---- host-buffer seam (abi_hostbuf.inl, abi_planar.inl): caller memory pinned with hipHostRegister, the copy
  // streams and events of the pipelined applyModelToSampleSet, the lazily built histogram tree of an adopted set
  struct HostReg
  {
    uintptr_t base;
    size_t bytes;
    bool automatic;  // made by BPF_OPT_HOST_AUTO_REGISTER, not by bpf_host_buffer_register
    uintptr_t dev_base;  // the range as a kernel addresses it (hipHostGetDevicePointer of base), 0: none
  };
  std::vector<HostReg> host_regs;
  bool host_auto_register = false;  // BPF_OPT_HOST_AUTO_REGISTER
  int seam_chunks = 0;              // BPF_OPT_SEAM_CHUNKS (0 = by size, 1 = the plain sequence)
  hipStream_t copy_up = nullptr;    // the uploads of the pipelined seam
  std::vector<hipEvent_t> seam_ev;  // [kSeamMaxChunks]: chunk uploaded
  DevBuf<double> d_seam_partials;   // [kSeamMaxChunks][kSeamMaxBlocks] block partials of the chunks' launches
  PinnedBuf<unsigned long long> h_seam_flags;  // [kSeamMaxChunks]: chunk c scored (the launch's generation)
  PinnedBuf<double> h_seam_totals;  // [kSeamMaxChunks]: weight total of chunk c
  unsigned long long seam_generation = 0;
  PinnedBuf<double> h_seam_w;       // [n] the chunked form's weights on their way back: FINE-grained (see PinnedBuf)
  int last_seam_chunks = 0;         // chunks the last applyModelToSampleSet used (0: the plain sequence)
  bool last_seam_registered = false;

  std::vector<double> stage_bx, stage_by;  // stage_field_scan's scratch: beam end points of every decimated beam

  // ---- tile-sorted scoring of a spread cloud (kernels_window.hpp, HOST_MODE 3 of k_score_field)
  bool tile_sort = true;            // BPF_OPT_TILE_SORT
  // Pageable host memory on its way up or down (h2d_from_host / d2h_to_host, host_copy.hpp): two pinned halves, one
  // in this thread's hands while the copy engine has the other
  PinnedBuf<unsigned char> h_bounce;
  PinnedBuf<unsigned char> h_small;  // [kSmallResultBytes] a few result words on their way into a local (small_down)
  hipEvent_t bounce_ev[2] = { nullptr, nullptr };
  bool bounce_busy[2] = { false, false };
  int bounce_next = 0;
  bool host_direct = false;         // BPF_OPT_HOST_DIRECT_PAGEABLE
  bool spread_init = false;         // the set was initialised with uniform random poses and not resampled since
  DevBuf<int> d_tile_int;           // hist[2][kTileBins] cursor[kTileBins] tile[n] perm[n]
  int tile_parity = 0;              // which half of hist the last tile-sorted update counted into
  DevBuf<double4> d_prep_sorted;
  int last_score_form = 0;          // diagnostics: 3 = the last scoring launch walked the particles in tile order
  int last_cloud_form = 0;          // diagnostics: 32 | the k_cloud_score instance of the last launch (badger_pf.h)

  // ---- profiling
  bool profiling = false;
  unsigned timed_launches = 0;  // scoring launches seen in profile mode 1 / 3 (every timed_stride-th is timed)
  unsigned timed_stride = 8;    // mode 1: kTimedLaunchStride, mode 3: 1
  bool profile_all = false;
  // the kernel classes the current profile mode times: the scoring kernels, or every class in mode 2
  bool times_class(int klass) const { return profile_all || klass == BPF_K_SCORE || klass == BPF_K_SCORE_WINDOW; }
  std::vector<hipEvent_t> ev_start, ev_stop;
  std::vector<int> ev_class;
  size_t ev_used = 0;
  bpf_profile prof{};

  int fail(int code, const std::string& msg)
  {
    last_error = msg;
    last_status = code;
    return code;
  }
  int fail_hip(hipError_t r, const char* what)
  {
    return fail(BPF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(r));
  }

  // ---- transitions: every change of the particle set goes through one of these, and wc, tree, set_epoch and
  // hist_matches_set are written here and in the two structs' own members, nowhere else.  Two
  // exceptions: wc.fused_partials is set by the scoring launch and cleared by the launch that folds the partials, and
  // TrialScores::score and shard_spare_tree put back a saved copy of wc / tree around work on a set that is not current

  // A scoring pass is about to overwrite the weights of a set that may not be the engine's (the candidate poses of
  // the uniform pose check, the host-buffer seam's scratch set: applyModelToSampleSet on a set of the caller's): the
  // buffers behind wc are its to use.  No epoch bump: the current set keeps its statistics.
  void weights_overwritten() { wc.drop(); }
  // The CURRENT set's weights changed (updateSensor's scoring and normalisation, a sharded stage of them): cached
  // statistics no longer describe it.  What the pass itself left in wc describes the new weights and stays; a site
  // that leaves nothing calls weights_overwritten as well.
  void weights_changed() { set_epoch++; }
  // Another set is current (updateResample's and updateAction's swap of current_set_, a set loaded or restored in
  // place): n samples, in the other buffer when `flip`; `t` are its tree counts (tree.counted / tree.pending /
  // tree itself when the poses' tree is the one already described).  converged_of > 0: updateConverged's count over
  // that many samples is on the device, for fetch_scalars to turn into `converged`.
  void new_set(int n, bool flip, const TreeCounts& t, int converged_of = 0)
  {
    if (flip)
      cur ^= 1;
    sample_count = n;
    wc.drop();
    set_epoch++;
    hist_matches_set = false;
    tree = t;
    if (converged_of > 0)
    {
      converged_pending = true;
      conv_n = converged_of;
    }
  }
  // A sharded set's slices went back to the even split (abi_shard_rebalance.inl): this rank's n samples from global
  // index `first` of `global` are in the other buffer, poses and weights copied bit for bit.  What describes the
  // GLOBAL set or the filter stays: tree (pending counts stay pending), converged and its pending count, d_scalars,
  // the drand48 state, spread_init, shard_form_used.  What described the old slice goes: the CDF and partials, the
  // statistics (epoch), the host histogram, and the W totals of the last sensor update, which belong to the old split.
  void slice_rebalanced(int n, long long first, long long global)
  {
    cur ^= 1;
    sample_count = n;
    slice_first = first;
    slice_global = global;
    wc.drop();
    set_epoch++;
    hist_matches_set = false;
    mb_totals_valid = false;
  }
  // initWithGaussian / initWithPoseFn / a set given by the caller (particle_filter.cpp:126-131,157-168): a new set,
  // w_slow = w_fast = 0, converged = false; `spread`: the poses are uniform over the free space
  int fresh_filter(int n, bool flip, const TreeCounts& t, bool spread)
  {
    new_set(n, flip, t);
    slice_first = -1;  // (a sharded init records its share behind this)
    spread_init = spread;
    HIPCHK(this, hipMemsetAsync(d_scalars.p, 0, sizeof(FilterScalars), stream));
    converged = 0;
    converged_pending = false;
    return BPF_OK;
  }
  // ParticleFilter's constructor (particle_filter.cpp:62-89): n samples at the origin in buffer 0, no tree yet
  // (counts 0).  A new_set like any other, so nothing an earlier filter on this engine left -- its CDF, statistics,
  // pending tree, host histogram, spread flag -- is served for this one
  void filter_created(int n)
  {
    new_set(n, cur != 0, TreeCounts{ 0, 0, 0, false });
    slice_first = -1;
    spread_init = false;
    converged = 0;
    converged_pending = false;
  }
  // updateResample has taken what it needs from the current set's tree and is about to draw: the resampler builds
  // the new set's tree from its draws, and its outcome says from here on whether the cloud is spread
  void resample_begins()
  {
    tree.tree_pending = false;
    spread_init = false;
  }
  // the current set's tree was built from its poses (PFKDTree of every sample, pf_kdtree.cpp:49-56) ...
  void tree_counted(int leaf, int bins) { tree = tree.counted(leaf, bins); }
  // ... or, for the global set of a sharded filter, from the ranks' bin lists or keys: e->hist, where that used it,
  // holds every distinct key ONCE and is not the set's histogram
  void tree_installed(int leaf, int bins, int route)
  {
    tree = TreeCounts{ leaf, bins, route, false };
    hist_matches_set = false;
  }
  // the counts were taken in the other KLD count mode: computed again when they are needed
  void tree_invalidated() { tree = tree.pending(); }
  // e->hist now holds every pose of the current set, inserted in index order
  void hist_built() { hist_matches_set = true; }
};

