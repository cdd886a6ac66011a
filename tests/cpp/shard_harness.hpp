// What the test programs of the sharded filter share (header-only, for tests): reading a case directory (cfg.txt of
// "key value ..." lines and raw .bin arrays, as tests/cpp_driver.py writes them), one engine's map, scanner, model
// and filter, loading and dumping slices, and the fork of one process per rank plus one for the unsharded filter.
#pragma once
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "badger_amcl_amd/adapter.hpp"
#include "badger_pf.h"

namespace amd = badger_amcl_amd;

// a C call in a function with `rank` in scope that returns a process exit code
#define CHECK(e, call)                                                                                          \
  do                                                                                                            \
  {                                                                                                             \
    const int _rc = (call);                                                                                     \
    if (_rc != BPF_OK)                                                                                          \
    {                                                                                                           \
      std::fprintf(stderr, "rank %d: %s -> %d (%s)\n", rank, #call, _rc, (e) ? bpf_last_error_message(e) : ""); \
      return 10 + _rc;                                                                                          \
    }                                                                                                           \
  } while (0)

template <typename T>
static std::vector<T> slurp(const std::string& path)
{
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { std::perror(path.c_str()); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

struct Inputs
{
  std::string dir;
  std::map<std::string, std::vector<double>> cfg;
  std::vector<int32_t> cells;
  std::vector<float> lut;
  std::vector<double> samples, ranges, angles;
  double v(const std::string& k, int i = 0) const { return cfg.at(k).at((size_t)i); }
  int i(const std::string& k, int j = 0) const { return (int)v(k, j); }
  int n() const { return (int)samples.size() / 4; }
  int cut(int r, int world) const { return cfg.count("cuts") ? i("cuts", r) : (int)((long long)n() * r / world); }

  // cfg.txt of `d`; false (and a line on stderr) when it does not hold `must_have`
  bool read_cfg(const std::string& d, const char* must_have)
  {
    dir = d;
    std::ifstream f(dir + "/cfg.txt");
    for (std::string line, key; std::getline(f, line);)
    {
      std::istringstream ss(line);
      ss >> key;
      for (double x; ss >> x;)
        cfg[key].push_back(x);
    }
    if (!cfg.count(must_have))
      std::fprintf(stderr, "no cfg.txt in %s\n", dir.c_str());
    return cfg.count(must_have) != 0;
  }
  // the 2-D map and the scan
  void read_planar()
  {
    cells = slurp<int32_t>(dir + "/cells.bin");
    lut = slurp<float>(dir + "/lut.bin");
    ranges = slurp<double>(dir + "/ranges.bin");
    angles = slurp<double>(dir + "/angles.bin");
  }
  // a whole planar case: cfg.txt, the map, the scan and the sample set
  bool read(const std::string& d)
  {
    if (!read_cfg(d, "max_samples"))
      return false;
    read_planar();
    samples = slurp<double>(dir + "/samples.bin");
    return true;
  }
};

// map, scanner, model and the filter (GLOBAL bounds) of one engine
inline std::shared_ptr<amd::ParticleFilter> make_filter(std::shared_ptr<amd::Engine> eng, const Inputs& in,
                                                        amd::PFResampleModelType model)
{
  bpf_engine* e = eng->get();
  eng->check(bpf_map2d_set(e, in.cells.data(), in.lut.data(), in.i("size"), in.i("size"), (float)in.v("origin", 0),
                           (float)in.v("origin", 1), in.v("res"), in.v("max_dist")));
  eng->check(bpf_planar_init(e, in.i("max_beams")));
  eng->check(bpf_planar_set_model_likelihood_field(e, in.v("model_p", 0), in.v("model_p", 1), in.v("model_p", 2),
                                                   in.v("max_dist")));
  eng->check(bpf_planar_set_map_factors(e, in.v("map_factors", 0), in.v("map_factors", 1), in.v("map_factors", 2)));
  const double pose[3] = { in.v("scanner_pose", 0), in.v("scanner_pose", 1), in.v("scanner_pose", 2) };
  eng->check(bpf_planar_set_scanner_pose(e, pose));
  auto pf = std::make_shared<amd::ParticleFilter>(eng, in.i("min_samples"), in.i("max_samples"), 0.0, 0.0, 85.0);
  pf->setResampleModel(model);
  if (in.cfg.count("kld"))
    eng->check(bpf_pf_set_kld_count(e, in.i("kld")));
  pf->srand48(in.i("seed"));
  return pf;
}

// rank r's slice of the loaded set; leaf: of the WHOLE set's tree (the systematic resampler sizes the new set from it)
inline void load_slice(amd::ParticleFilter& pf, const Inputs& in, int lo, int hi)
{
  bpf_engine* e = pf.engine().get();
  if (hi > lo)
    pf.engine().check(bpf_pf_set_samples(e, in.samples.data() + 4 * (size_t)lo, hi - lo, in.i("leaf")));
  else  // a shard without samples
    pf.engine().check(bpf_shard_adopt_dev(e, nullptr, nullptr, nullptr, 0, in.n(), 0, 0));
}

inline int dump(const std::string& path, const void* p, size_t bytes)
{
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return 3;
  std::fwrite(p, 1, bytes, f);
  std::fclose(f);
  return 0;
}

// the engine's current set into dir/name, up to max_samples of them (a shard without samples: an empty file); a
// process exit code
inline int dump_set(bpf_engine* e, const std::string& dir, int max_samples, int rank, const std::string& name)
{
  std::vector<double> s((size_t)max_samples * 4 + 4);
  int got = 0;
  bpf_pf_state st;
  CHECK(e, bpf_pf_get_state(e, &st));
  if (st.sample_count > 0)
    CHECK(e, bpf_pf_get_samples(e, s.data(), max_samples, &got));
  return dump(dir + "/" + name, s.data(), (size_t)got * 4 * sizeof(double));
}

inline void dump(const Inputs& in, const std::string& name, amd::ParticleFilter& pf)
{
  if (dump_set(pf.engine().get(), in.dir, in.i("max_samples"), 0, name) != 0)
    std::exit(3);
}

inline std::shared_ptr<amd::PlanarData> scan(const Inputs& in)
{
  auto data = std::make_shared<amd::PlanarData>();
  data->range_count_ = (int)in.ranges.size();
  data->range_max_ = in.v("range_max");
  data->ranges_ = in.ranges;
  data->angles_ = in.angles;
  return data;
}

// the motion of every program's odometry step
inline std::shared_ptr<amd::OdomData> odom_data()
{
  auto d = std::make_shared<amd::OdomData>();
  d->pose = { 1.0, 2.0, 0.3 };
  d->delta = { 0.03, -0.01, 0.02 };
  d->absolute_motion = { 0.03, 0.01, 0.02 };
  return d;
}

inline std::vector<long long> exchange_counts(const std::vector<std::shared_ptr<amd::ParticleFilter>>& pfs)
{
  std::vector<long long> x(pfs.size());
  for (size_t r = 0; r < pfs.size(); ++r)
    bpf_shard_exchange_count(pfs[r]->engine().get(), &x[r]);
  return x;
}

// One forked process per rank plus one (r = -1) for the unsharded filter, each printing into dir/rank<r>.txt
// (dir/single.txt) and leaving with what body(r) returns, 9 when it throws; the worst exit code.  Fork BEFORE anything
// touches the GPU: every child initialises HIP for itself.
inline int fork_ranks(const std::string& dir, int world, const std::function<int(int)>& body)
{
  std::vector<pid_t> kids;
  for (int r = -1; r < world; ++r)
  {
    const pid_t pid = fork();
    if (pid == 0)
    {
      // every process prints into a file of its own (a line of a few thousand clusters is no atomic pipe write)
      const std::string out = dir + "/" + (r < 0 ? std::string("single") : "rank" + std::to_string(r)) + ".txt";
      if (!std::freopen(out.c_str(), "w", stdout))
        _exit(3);
      int rc = 9;
      try
      {
        rc = body(r);
      }
      catch (const std::exception& err)
      {
        std::fprintf(stderr, "rank %d: %s\n", r, err.what());
      }
      std::fflush(stdout);
      _exit(rc);
    }
    kids.push_back(pid);
  }
  int worst = 0;
  for (pid_t pid : kids)
  {
    int status = 0;
    waitpid(pid, &status, 0);
    const int code = WIFEXITED(status) ? WEXITSTATUS(status) : 99;
    if (code != 0)
      worst = code;
  }
  return worst;
}

// ---- "name dir mode world port flags": a planar case run by all ranks in this process (mode 0: run_local, followed
// by the unsharded filter) or by forked ranks (mode 1: run_rank per rank beside run_unsharded)
struct ShardProgram
{
  const char* name;
  std::function<int(const Inputs&, int world)> run_local;
  std::function<int(const Inputs&)> run_unsharded;
  std::function<int(const Inputs&, int rank, int world, int port, int flags)> run_rank;

  int main(int argc, char** argv) const
  {
    if (argc != 6)
    {
      std::fprintf(stderr, "usage: dir mode world port flags\n");
      return 2;
    }
    Inputs in;
    if (!in.read(argv[1]))
      return 2;
    const int mode = std::atoi(argv[2]), W = std::atoi(argv[3]), port = std::atoi(argv[4]), flags = std::atoi(argv[5]);
    if (mode != 0)
      return fork_ranks(in.dir, W, [&](int r) { return r < 0 ? run_unsharded(in) : run_rank(in, r, W, port, flags); });
    try
    {
      return run_local(in, W);
    }
    catch (const std::exception& err)
    {
      std::fprintf(stderr, "%s: %s\n", name, err.what());
      return 1;
    }
  }
};

// the unsharded filter's sensor update and resample; prints the rng state before the resample
inline int run_unsharded(const Inputs& in, amd::PFResampleModelType model, bool dump_loaded = false)
{
  auto one = make_filter(std::make_shared<amd::Engine>(0), in, model);
  bpf_engine* e = one->engine().get();
  one->engine().check(bpf_pf_set_samples(e, in.samples.data(), in.n(), in.i("leaf")));
  if (dump_loaded)
    dump(in, "single.loaded.bin", *one);
  one->engine().check(bpf_pf_update_sensor_planar(e, in.ranges.data(), in.angles.data(), (int)in.ranges.size(),
                                                  in.v("range_max")));
  uint64_t rng0 = 0, rng = 0;
  one->engine().check(bpf_pf_get_rng_state(e, &rng0));
  one->updateResample();
  dump(in, "single.resample.bin", *one);
  const bpf_pf_state st = one->getState();
  one->engine().check(bpf_pf_get_rng_state(e, &rng));
  std::printf("single rng0 %llu M %d leaf %d bins %d rng %llu conv %d\n", (unsigned long long)rng0, st.sample_count,
              st.leaf_count, st.bin_count, (unsigned long long)rng, st.converged);
  std::fflush(stdout);
  return 0;
}

// the ranks of a local world with their slices loaded
struct LocalRanks
{
  std::vector<std::shared_ptr<amd::ParticleFilter>> pfs;
  std::vector<int> counts;
  LocalRanks(const Inputs& in, int W, amd::PFResampleModelType model)
  {
    for (int r = 0; r < W; ++r)
    {
      pfs.push_back(make_filter(std::make_shared<amd::Engine>(0), in, model));
      load_slice(*pfs.back(), in, in.cut(r, W), in.cut(r + 1, W));
      counts.push_back(in.cut(r + 1, W) - in.cut(r, W));
    }
  }
};

// the step after a resample takes the slices where they are: a motion update needs every rank's first global index
inline void next_step(amd::LocalShardedParticleFilter& local, const LocalRanks& L, const Inputs& in)
{
  for (auto& p : L.pfs)
    p->engine().check(bpf_odom_set_model(p->engine().get(), BPF_ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.04, 0.03, 0.02, 0.0));
  local.updateAction(odom_data());
  local.updateSensor(scan(in));
  std::printf("next step ok form %d\n", local.formUsed());
}

// ---- one sensor update and one in-place resample through the one-call form, beside the same filter unsharded:
// shard_in_place.cpp and shard_in_place_mn.cpp are this program with their resampler, their way of setting the form
// (a generic callable: it gets a LocalShardedParticleFilter or a ShardedParticleFilter); both print the same rank line
inline void rank_line(int r, amd::ShardedParticleFilter& sf, long long before, long long after)
{
  amd::ParticleFilter& pf = sf.filter();
  const bpf_pf_state st = pf.getState();
  uint64_t rng = 0;
  pf.engine().check(bpf_pf_get_rng_state(pf.engine().get(), &rng));
  std::printf("rank %d M %d leaf %d bins %d windows %d local %d first %lld form %d rng %llu miss %d conv %d eleaf %d "
              "ebins %d exch0 %lld exch1 %lld\n", r, sf.globalSampleCount(), sf.leafCount(), sf.binCount(), sf.windowsUsed(),
              st.sample_count, sf.globalFirst(), sf.formUsed(), (unsigned long long)rng, sf.cdfMiss() ? 1 : 0, st.converged,
              st.leaf_count, st.bin_count, before, after);
  std::fflush(stdout);
}

template <typename SetForm>
ShardProgram in_place_program(const char* name, amd::PFResampleModelType model, SetForm set_form)
{
  ShardProgram P;
  P.name = name;
  P.run_unsharded = [=](const Inputs& in) { return run_unsharded(in, model); };
  P.run_local = [=](const Inputs& in, int W) {
    LocalRanks L(in, W, model);
    amd::LocalShardedParticleFilter local(L.pfs, L.counts, in.i("leaf"), 4096);
    int mode = -1;
    bpf_shard_exchange_mode(L.pfs[0]->engine().get(), &mode);
    std::printf("mode %d\n", mode);
    set_form(local, in);
    local.updateSensor(scan(in));
    const std::vector<long long> before = exchange_counts(L.pfs);
    local.updateResample();
    const std::vector<long long> after = exchange_counts(L.pfs);
    for (int r = 0; r < W; ++r)
    {
      dump(in, "rank" + std::to_string(r) + ".resample.bin", *L.pfs[(size_t)r]);
      rank_line(r, local.rank(r), before[(size_t)r], after[(size_t)r]);
    }
    next_step(local, L, in);
    local.shutdown();
    return run_unsharded(in, model);
  };
  P.run_rank = [=](const Inputs& in, int rank, int W, int port, int flags) {
    auto pf = make_filter(std::make_shared<amd::Engine>(0), in, model);
    load_slice(*pf, in, in.cut(rank, W), in.cut(rank + 1, W));
    amd::ShardedParticleFilter sf(pf, in.n(), in.i("leaf"), 4096, in.cut(rank, W));
    const int mode = sf.bootstrap(rank, W, "127.0.0.1:" + std::to_string(port), in.i("max_samples"), flags);
    std::printf("mode %d\n", mode);
    set_form(sf, in);
    sf.updateSensor(scan(in));
    long long before = 0, after = 0;
    bpf_shard_exchange_count(pf->engine().get(), &before);
    sf.updateResample();
    bpf_shard_exchange_count(pf->engine().get(), &after);
    dump(in, "rank" + std::to_string(rank) + ".resample.bin", *pf);
    rank_line(rank, sf, before, after);
    sf.shutdown();
    return 0;
  };
  return P;
}
