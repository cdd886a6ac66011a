// A sharded filter as a C / C++ node runs it, with nothing but the library between the ranks: this program forks one
// process per rank (all on GPU 0) plus one that runs the same filter unsharded, every rank calls bpf_shard_bootstrap
// on 127.0.0.1:<port> and then drives update + resample cycles and the global statistics through the one-call forms --
// the planar update (prob model with beam skipping included), the 3-D cloud update, bpf_shard_compute_cluster_stats /
// bpf_shard_get_max_weight_pose -- either through the C calls (api 0) or through badger_amcl_amd::ShardedParticleFilter
// (api 1).  Every process dumps its set after each step and writes what it got into <dir>/rank<r>.txt (single.txt);
// tests/test_gpu_cpp_shard_node.py compares.
//
// usage: shard_node dir world port flags api        (dir holds cfg.txt and the binary inputs, and takes the dumps)
// cfg.txt: "key value ..." lines; kind 0 planar scanner, 1 cloud scanner, 2 none (statistics and their timing only)
#include <algorithm>
#include <chrono>

#include "shard_harness.hpp"

struct NodeInputs : Inputs
{
  std::vector<float> points;
  std::vector<uint32_t> pose_indices;
  std::vector<uint8_t> ratios;
  bool cloud() const { return i("kind") == 1; }
};

static int setup(bpf_engine* e, const NodeInputs& in, int rank)
{
  if (in.i("kind") == 2)
    ;  // no scanner: the statistics of the loaded set only
  else if (in.cloud())
  {
    const int mn[3] = { in.i("min_cells", 0), in.i("min_cells", 1), in.i("min_cells", 2) };
    const int mx[3] = { in.i("max_cells", 0), in.i("max_cells", 1), in.i("max_cells", 2) };
    CHECK(e, bpf_map3d_set(e, in.pose_indices.data(), in.pose_indices.size(), in.ratios.data(), in.ratios.size(), mn, mx,
                           in.v("res"), in.v("max_dist")));
    CHECK(e, bpf_cloud_init(e, in.i("max_beams")));
    CHECK(e, bpf_cloud_set_model(e, in.v("model_p", 0), in.v("model_p", 1), in.v("model_p", 2)));
    CHECK(e, bpf_cloud_set_map_factors(e, in.v("map_factors", 0), in.v("map_factors", 1), in.v("map_factors", 2)));
    const double xyz[3] = { in.v("tf_xyz", 0), in.v("tf_xyz", 1), in.v("tf_xyz", 2) };
    const double q[4] = { in.v("tf_quat", 0), in.v("tf_quat", 1), in.v("tf_quat", 2), in.v("tf_quat", 3) };
    CHECK(e, bpf_cloud_set_scanner_to_footprint_tf(e, xyz, q));
  }
  else
  {
    CHECK(e, bpf_map2d_set(e, in.cells.data(), in.lut.data(), in.i("size"), in.i("size"), (float)in.v("origin", 0),
                           (float)in.v("origin", 1), in.v("res"), in.v("max_dist")));
    CHECK(e, bpf_planar_init(e, in.i("max_beams")));
    if (in.i("model") == 1)
      CHECK(e, bpf_planar_set_model_likelihood_field_prob(e, in.v("model_p", 0), in.v("model_p", 1), in.v("model_p", 2),
                                                          in.v("max_dist"), in.i("beamskip", 0), in.v("beamskip", 1),
                                                          in.v("beamskip", 2), in.v("beamskip", 3)));
    else
      CHECK(e, bpf_planar_set_model_likelihood_field(e, in.v("model_p", 0), in.v("model_p", 1), in.v("model_p", 2),
                                                     in.v("max_dist")));
    CHECK(e, bpf_planar_set_map_factors(e, in.v("map_factors", 0), in.v("map_factors", 1), in.v("map_factors", 2)));
    const double pose[3] = { in.v("scanner_pose", 0), in.v("scanner_pose", 1), in.v("scanner_pose", 2) };
    CHECK(e, bpf_planar_set_scanner_pose(e, pose));
  }
  if (in.i("stats_host"))
    CHECK(e, bpf_set_option(e, BPF_OPT_STATS_HOST, 1));
  return 0;
}

static int dump_set(bpf_engine* e, const NodeInputs& in, int rank, const std::string& name)
{
  return dump_set(e, in.dir, in.i("max_samples"), rank, name);
}

// the sharded filter of one rank behind either binding
struct Node
{
  int api = 0, rank = 0;
  bpf_engine* e = nullptr;
  std::shared_ptr<amd::Engine> eng;
  std::shared_ptr<amd::ParticleFilter> pf;
  std::unique_ptr<amd::ShardedParticleFilter> sf;
  int global = 0, leaf = 1, bins = 0, windows = 0, hint = 4096, miss = 0;

  int update_sensor(const NodeInputs& in)
  {
    if (api == 1)
    {
      if (in.cloud())
        sf->updateSensorCloud(in.points.data(), (int)in.points.size() / 3);
      else
        sf->updateSensor(scan(in));
      return 0;
    }
    if (in.cloud())
      CHECK(e, bpf_shard_update_sensor_cloud(e, in.points.data(), (int)in.points.size() / 3, global));
    else
      CHECK(e, bpf_shard_update_sensor_planar(e, in.ranges.data(), in.angles.data(), (int)in.ranges.size(),
                                              in.v("range_max"), global));
    return 0;
  }
  int update_resample()
  {
    if (api == 1)
    {
      sf->updateResample();
      global = sf->globalSampleCount();
      leaf = sf->leafCount();
      bins = sf->binCount();
      windows = sf->windowsUsed();
      miss = sf->cdfMiss() ? 1 : 0;
      return 0;
    }
    CHECK(e, bpf_shard_update_resample(e, &global, &leaf, &bins, &windows, &hint, &miss));
    return 0;
  }
  int max_weight_pose(double* w, double pose[3])
  {
    if (api == 1)
    {
      std::array<double, 3> p{};
      sf->getMaxWeightPose(w, &p);
      pose[0] = p[0], pose[1] = p[1], pose[2] = p[2];
      return 0;
    }
    CHECK(e, bpf_shard_get_max_weight_pose(e, w, pose));
    return 0;
  }
};

// the global figures as one line of hex floats, and the laziness of a second query
static int print_stats(Node& nd, const char* tag, int cycle)
{
  bpf_engine* e = nd.e;
  const int rank = nd.rank;
  int n = 0, route = 0;
  double mean[3], cov[5], bw = 0, bp[3] = { 0, 0, 0 };
  CHECK(e, bpf_shard_compute_cluster_stats(e, &n, mean, cov, &route));
  if (int rc = nd.max_weight_pose(&bw, bp))
    return rc;
  std::string line;
  char buf[512];
  std::snprintf(buf, sizeof buf, "stats %s %d route %d n %d mean %a %a %a cov %a %a %a %a %a best %a %a %a %a clusters", tag,
                cycle, route, n, mean[0], mean[1], mean[2], cov[0], cov[1], cov[2], cov[3], cov[4], bw, bp[0], bp[1], bp[2]);
  line = buf;
  for (int k = 0; k < n; ++k)
  {
    bpf_cluster c;
    CHECK(e, bpf_pf_get_cluster(e, k, &c));
    std::snprintf(buf, sizeof buf, " %d %a %a %a %a %a %a %a %a %a", c.count, c.weight, c.mean[0], c.mean[1], c.mean[2],
                  c.cov[0], c.cov[1], c.cov[2], c.cov[3], c.cov[4]);
    line += buf;
  }
  bpf_cluster past;
  if (bpf_pf_get_cluster(e, n, &past) != BPF_ERR_INVALID_ARGUMENT)
    return 4;
  if (nd.api == 1)
  {
    // the class's own cluster getter returns the same global cluster
    double w = 0;
    std::array<double, 3> m{};
    bpf_cluster c0;
    CHECK(e, bpf_pf_get_cluster(e, 0, &c0));
    if (!nd.sf->getClusterStats(0, &w, &m) || w != c0.weight || m[0] != c0.mean[0] || nd.sf->statsRoute() != route)
      return 5;
  }
  std::printf("rank %d %s\n", rank, line.c_str());
  // nothing has changed: the same bits, and no exchange
  long long before = 0, after = 0;
  CHECK(e, bpf_shard_exchange_count(e, &before));
  double bw2 = 0, bp2[3] = { 0, 0, 0 };
  if (int rc = nd.max_weight_pose(&bw2, bp2))
    return rc;
  CHECK(e, bpf_shard_exchange_count(e, &after));
  const int same = std::memcmp(&bw, &bw2, sizeof bw) == 0 && std::memcmp(bp, bp2, sizeof bp) == 0;
  std::printf("rank %d lazy %s %d same %d exch %lld %lld\n", rank, tag, cycle, same, before, after);
  std::fflush(stdout);
  return 0;
}

static int run_rank_body(const NodeInputs& in, Node& nd, int world, int port, int flags)
{
  const int rank = nd.rank;
  const int n_global = (int)in.samples.size() / 4;
  const int api = nd.api;
  if (api == 1)
  {
    nd.eng = std::make_shared<amd::Engine>(0);
    nd.e = nd.eng->get();
  }
  else
    CHECK(nd.e, bpf_create(0, &nd.e));
  bpf_engine* e = nd.e;
  if (int rc = setup(e, in, rank))
    return rc;
  if (api == 1)  // the GLOBAL bounds on every rank
    nd.pf = std::make_shared<amd::ParticleFilter>(nd.eng, in.i("min_samples"), in.i("max_samples"), 0.0, 0.0, 85.0);
  else
    CHECK(e, bpf_pf_create(e, in.i("min_samples"), in.i("max_samples"), 0.0, 0.0, 85.0));
  CHECK(e, bpf_pf_srand48(e, in.i("seed")));
  const int lo = in.cut(rank, world), hi = in.cut(rank + 1, world);
  if (hi > lo)
    CHECK(e, bpf_pf_set_samples(e, in.samples.data() + 4 * (size_t)lo, hi - lo, 1));
  else
    CHECK(e, bpf_shard_adopt_dev(e, nullptr, nullptr, nullptr, 0, n_global, 0, 0));  // a shard without samples
  {
    // no exchange yet: the one-call forms say so
    int cnt = 0;
    double w = 0, p[3];
    long long x = 0;
    const float xyz[3] = { 1.0f, 0.0f, 0.0f };
    const int a = bpf_shard_update_sensor_cloud(e, xyz, 1, n_global);
    const int b = bpf_shard_compute_cluster_stats(e, &cnt, nullptr, nullptr, nullptr);
    const int c = bpf_shard_get_max_weight_pose(e, &w, p);
    const int d = bpf_shard_exchange_count(e, &x);
    std::printf("rank %d unconfigured %d %d %d %d\n", rank, a, b, c, d);
  }
  const std::string addr = "127.0.0.1:" + std::to_string(port);
  int mode = 0;
  nd.global = n_global;
  if (api == 1)
  {
    nd.sf.reset(new amd::ShardedParticleFilter(nd.pf, n_global, 1, 4096));
    mode = nd.sf->bootstrap(rank, world, addr, in.i("max_samples"), flags);
  }
  else
    CHECK(e, bpf_shard_bootstrap(e, rank, world, addr.c_str(), in.i("max_samples"), flags, &mode));
  std::printf("rank %d mode %d\n", rank, mode);
  const bool stats = in.i("stats") != 0;
  if (stats)
  {
    // the split as loaded (the only state in which a shard can be empty: an empty set takes no sensor update)
    if (int rc = dump_set(e, in, rank, "rank" + std::to_string(rank) + ".c0.loaded.bin"))
      return rc;
    if (int rc = print_stats(nd, "loaded", 0))
      return rc;
  }
  if (in.cfg.count("time_pose"))
  {
    // wall time of one global pose evaluated afresh: time_pose = (timed repetitions, untimed ones before them)
    std::vector<double> ms;
    for (int rep = 0; rep < in.i("time_pose", 0) + in.i("time_pose", 1); ++rep)
    {
      CHECK(e, bpf_set_option(e, BPF_OPT_STATS_HOST, in.i("stats_host")));  // drops the cached statistics, not the set
      const auto t0 = std::chrono::steady_clock::now();
      double w = 0, p[3];
      if (int rc = nd.max_weight_pose(&w, p))
        return rc;
      const auto t1 = std::chrono::steady_clock::now();
      if (rep >= in.i("time_pose", 1))
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("rank %d time_pose reps %d median_ms %.4f min_ms %.4f\n", rank, (int)ms.size(), ms[ms.size() / 2], ms[0]);
  }
  for (int cycle = 0; cycle < in.i("cycles"); ++cycle)
  {
    const std::string stem = "rank" + std::to_string(rank) + ".c" + std::to_string(cycle);
    if (int rc = nd.update_sensor(in))
      return rc;
    if (int rc = dump_set(e, in, rank, stem + ".sensor.bin"))
      return rc;
    if (stats)
      if (int rc = print_stats(nd, "sensor", cycle))
        return rc;
    if (int rc = nd.update_resample())
      return rc;
    if (int rc = dump_set(e, in, rank, stem + ".resample.bin"))
      return rc;
    bpf_pf_state st;
    CHECK(e, bpf_pf_get_state(e, &st));
    uint64_t rng = 0;
    CHECK(e, bpf_pf_get_rng_state(e, &rng));
    long long exch = 0;
    CHECK(e, bpf_shard_exchange_count(e, &exch));
    std::printf("rank %d cycle %d M %d leaf %d bins %d windows %d local %d rng %llu miss %d conv %d exch %lld\n", rank, cycle,
                nd.global, nd.leaf, nd.bins, nd.windows, st.sample_count, (unsigned long long)rng, nd.miss, st.converged,
                exch);
    std::fflush(stdout);
    if (stats)
      if (int rc = print_stats(nd, "resample", cycle))
        return rc;
  }
  if (api == 1)
  {
    nd.sf->shutdown();
    nd.sf.reset();
    nd.pf.reset();
    nd.eng.reset();
  }
  else
  {
    CHECK(e, bpf_shard_shutdown(e));
    bpf_destroy(e);
  }
  return 0;
}

static int run_rank(const NodeInputs& in, int rank, int world, int port, int flags, int api)
{
  Node nd;
  nd.api = api;
  nd.rank = rank;
  return run_rank_body(in, nd, world, port, flags);
}

// the same filter on one engine through the ordinary entry points
static int run_unsharded(const NodeInputs& in)
{
  const int rank = -1;
  const int n = (int)in.samples.size() / 4;
  bpf_engine* e = nullptr;
  CHECK(e, bpf_create(0, &e));
  if (int rc = setup(e, in, rank))
    return rc;
  CHECK(e, bpf_pf_create(e, in.i("min_samples"), in.i("max_samples"), 0.0, 0.0, 85.0));
  CHECK(e, bpf_pf_srand48(e, in.i("seed")));
  CHECK(e, bpf_pf_set_samples(e, in.samples.data(), n, 1));
  for (int cycle = 0; cycle < in.i("cycles"); ++cycle)
  {
    const std::string stem = "single.c" + std::to_string(cycle);
    bpf_pf_state st;
    CHECK(e, bpf_pf_get_state(e, &st));
    const int conv_before = st.converged;
    if (in.cloud())
      CHECK(e, bpf_pf_update_sensor_cloud(e, in.points.data(), (int)in.points.size() / 3));
    else
      CHECK(e, bpf_pf_update_sensor_planar(e, in.ranges.data(), in.angles.data(), (int)in.ranges.size(), in.v("range_max")));
    if (int rc = dump_set(e, in, rank, stem + ".sensor.bin"))
      return rc;
    CHECK(e, bpf_pf_update_resample(e));
    if (int rc = dump_set(e, in, rank, stem + ".resample.bin"))
      return rc;
    CHECK(e, bpf_pf_get_state(e, &st));
    uint64_t rng = 0;
    CHECK(e, bpf_pf_get_rng_state(e, &rng));
    std::printf("single cycle %d conv_before %d M %d leaf %d bins %d rng %llu conv %d\n", cycle, conv_before, st.sample_count,
                st.leaf_count, st.bin_count, (unsigned long long)rng, st.converged);
    std::fflush(stdout);
  }
  bpf_destroy(e);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 6)
  {
    std::fprintf(stderr, "usage: dir world port flags api\n");
    return 2;
  }
  NodeInputs in;
  if (!in.read_cfg(argv[1], "kind"))
    return 2;
  in.samples = slurp<double>(in.dir + "/samples.bin");
  if (in.i("kind") == 2)
    ;
  else if (in.cloud())
  {
    in.pose_indices = slurp<uint32_t>(in.dir + "/pose_indices.bin");
    in.ratios = slurp<uint8_t>(in.dir + "/ratios.bin");
    in.points = slurp<float>(in.dir + "/points.bin");
  }
  else
    in.read_planar();
  const int world = std::atoi(argv[2]), port = std::atoi(argv[3]), flags = std::atoi(argv[4]), api = std::atoi(argv[5]);
  return fork_ranks(in.dir, world,
                    [&](int r) { return r < 0 ? run_unsharded(in) : run_rank(in, r, world, port, flags, api); });
}
