// The particle cloud of a sharded filter as a C / C++ node gets it, with nothing but the library between the ranks: this
// program forks one process per rank (all on GPU 0) plus one that holds the whole set on one engine.  Every rank loads
// its slice, calls bpf_shard_bootstrap on 127.0.0.1:<port> and asks for the pose array of the GLOBAL set -- on rank 0
// (root = 0; first 0, stride 1) and on every rank (root = -1; first 3, stride 7) -- through the C call and through
// badger_amcl_amd::ShardedParticleFilter::getPoseArray.  Every process dumps what it received into
// <dir>/rank<r>.<api>.<query>.bin (single.<query>.bin: bpf_pf_get_pose_array) and prints its figures into
// <dir>/rank<r>.txt; tests/test_gpu_cpp_shard_pose_array.py compares.
//
// usage: shard_pose_array dir world port flags [cut_0 .. cut_world]     (dir holds samples.bin: n x 4 doubles)
#include "shard_harness.hpp"

static int dump(const std::string& path, const double* p, size_t n_doubles)
{
  return dump(path, static_cast<const void*>(p), n_doubles * sizeof(double));
}

struct Query
{
  const char* name;
  int root;
  long long first;
  int stride;
};
static const Query kQueries[2] = { { "root0", 0, 0, 1 }, { "all", -1, 3, 7 } };

static long long exchanges(bpf_engine* e)
{
  long long x = -1;
  bpf_shard_exchange_count(e, &x);
  return x;
}

static int run_rank(const std::string& dir, const std::vector<double>& samples, const std::vector<int>& cuts, int rank,
                         int world, int port, int flags)
{
  const int n_global = (int)samples.size() / 4;
  auto eng = std::make_shared<amd::Engine>(0);
  bpf_engine* e = eng->get();
  auto pf = std::make_shared<amd::ParticleFilter>(eng, 100, n_global, 0.0, 0.0, 85.0);  // the GLOBAL bounds on every rank
  const int lo = cuts[(size_t)rank], hi = cuts[(size_t)rank + 1];
  if (hi > lo)
    CHECK(e, bpf_pf_set_samples(e, samples.data() + 4 * (size_t)lo, hi - lo, 1));
  else
    CHECK(e, bpf_shard_adopt_dev(e, nullptr, nullptr, nullptr, 0, n_global, 0, 0));  // a shard without samples
  std::vector<double> buf((size_t)7 * (size_t)n_global, -123.456);
  int count = -1;
  // no exchange yet: the one-call form says so
  std::printf("rank %d unconfigured %d\n", rank, bpf_shard_get_pose_array(e, 0, 0, 1, buf.data(), n_global, &count));
  amd::ShardedParticleFilter sf(pf, n_global, 1, 4096, lo);
  const std::string addr = "127.0.0.1:" + std::to_string(port);
  const int mode = sf.bootstrap(rank, world, addr, n_global, flags);
  std::printf("rank %d mode %d\n", rank, mode);
  const std::string stem = dir + "/rank" + std::to_string(rank);
  for (const Query& q : kQueries)
  {
    const bool receives = q.root < 0 || q.root == rank;
    // the C call
    long long x0 = exchanges(e);
    count = -1;
    CHECK(e, bpf_shard_get_pose_array(e, q.root, q.first, q.stride, receives ? buf.data() : nullptr, n_global, &count));
    long long x1 = exchanges(e);
    std::printf("rank %d query %s api c count %d exch %lld\n", rank, q.name, count, x1 - x0);
    if (receives)
      if (int rc = dump(stem + ".c." + q.name + ".bin", buf.data(), (size_t)7 * (size_t)count))
        return rc;
    // the class
    std::vector<double> poses;
    x0 = exchanges(e);
    const bool got = sf.getPoseArray(q.root, &poses, q.first, q.stride);
    x1 = exchanges(e);
    std::printf("rank %d query %s api a count %d exch %lld received %d\n", rank, q.name, (int)(poses.size() / 7), x1 - x0,
                got ? 1 : 0);
    if (got != receives)
      return 5;
    if (got)
      if (int rc = dump(stem + ".a." + q.name + ".bin", poses.data(), poses.size()))
        return rc;
  }
  {
    // the statistics in force stay in force across a query: the second getMaxWeightPose makes no exchange
    double w0 = 0, w1 = 0;
    std::array<double, 3> p0{}, p1{};
    sf.getMaxWeightPose(&w0, &p0);
    const long long a = exchanges(e);
    CHECK(e, bpf_shard_get_pose_array(e, 0, 0, 1, rank == 0 ? buf.data() : nullptr, n_global, &count));
    const long long b = exchanges(e);
    sf.getMaxWeightPose(&w1, &p1);
    const long long c = exchanges(e);
    const int same = std::memcmp(&w0, &w1, sizeof w0) == 0 && std::memcmp(p0.data(), p1.data(), sizeof(double) * 3) == 0;
    std::printf("rank %d lazy same %d query_exch %lld pose_exch %lld\n", rank, same, b - a, c - b);
  }
  {
    // one pose short on the receiving rank: refused there, untouched, and the other ranks are not left waiting
    std::vector<double> small((size_t)7 * (size_t)n_global, -123.456);
    const int rc = bpf_shard_get_pose_array(e, 0, 0, 1, rank == 0 ? small.data() : nullptr, n_global - 1, &count);
    int touched = 0;
    for (double v : small)
      touched += v != -123.456;
    std::printf("rank %d short rc %d count %d touched %d\n", rank, rc, count, touched);
    // a root outside the world, a stride of 0: refused on every rank before any exchange
    const long long a = exchanges(e);
    const int r1 = bpf_shard_get_pose_array(e, world, 0, 1, small.data(), n_global, &count);
    const int r2 = bpf_shard_get_pose_array(e, 0, 0, 0, small.data(), n_global, &count);
    const int r3 = bpf_shard_get_pose_array(e, 0, -1, 1, small.data(), n_global, &count);
    // a selection past the end: the counts cross, nothing else
    const int r4 = bpf_shard_get_pose_array(e, -1, n_global, 1, small.data(), n_global, &count);
    std::printf("rank %d refused %d %d %d empty %d count %d exch %lld\n", rank, r1, r2, r3, r4, count, exchanges(e) - a);
  }
  std::fflush(stdout);
  sf.shutdown();
  return 0;
}

// the whole set on one engine through the ordinary entry point
static int run_unsharded(const std::string& dir, const std::vector<double>& samples)
{
  const int rank = -1;
  const int n = (int)samples.size() / 4;
  bpf_engine* e = nullptr;
  CHECK(e, bpf_create(0, &e));
  CHECK(e, bpf_pf_create(e, 100, n, 0.0, 0.0, 85.0));
  CHECK(e, bpf_pf_set_samples(e, samples.data(), n, 1));
  std::vector<double> buf((size_t)7 * (size_t)n);
  for (const Query& q : kQueries)
  {
    int count = 0;
    CHECK(e, bpf_pf_get_pose_array(e, (int)q.first, q.stride, buf.data(), n, &count));
    std::printf("single query %s count %d\n", q.name, count);
    if (int rc = dump(dir + "/single." + q.name + ".bin", buf.data(), (size_t)7 * (size_t)count))
      return rc;
  }
  bpf_destroy(e);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 5)
  {
    std::fprintf(stderr, "usage: dir world port flags [cuts]\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int world = std::atoi(argv[2]), port = std::atoi(argv[3]), flags = std::atoi(argv[4]);
  const std::vector<double> samples = slurp<double>(dir + "/samples.bin");
  const int n = (int)samples.size() / 4;
  std::vector<int> cuts;
  for (int r = 0; r <= world; ++r)
    cuts.push_back(argc >= 6 + world ? std::atoi(argv[5 + r]) : (int)((long long)n * r / world));
  if (cuts.front() != 0 || cuts.back() != n)
    return 2;
  return fork_ranks(dir, world, [&](int r) {
    return r < 0 ? run_unsharded(dir, samples) : run_rank(dir, samples, cuts, r, world, port, flags);
  });
}
