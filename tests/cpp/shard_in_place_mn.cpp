// The multinomial resample of a sharded filter IN PLACE through the one-call form (bpf_shard_update_resample with the
// multinomial form set to BPF_SHARD_RESAMPLE_IN_PLACE), beside the same filter unsharded: one sensor update and one
// resample.
//
//   mode 0   badger_amcl_amd::LocalShardedParticleFilter: all `world` ranks in this process (the local exchange)
//   mode 1   one forked process per rank through badger_amcl_amd::ShardedParticleFilter::bootstrap: the mailbox, or
//            RCCL with BPF_BOOTSTRAP_FORCE_COLLECTIVE in `flags`
//
// Every rank dumps its slice and prints where it sits, the figures of the resample and the exchange count before and
// behind it; tests/test_gpu_cpp_shard_in_place_mn.py sorts the unsharded engine's set by the owner of each sample's
// source.  Every wait inside the library is bounded by the exchange time-out (5 s, bpf_shard_mailbox_set_timeout_ms).
//
// usage: shard_in_place_mn dir mode world port flags   (dir holds cfg.txt and the binary inputs, and takes the dumps)
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "badger_amcl_amd/adapter.hpp"
#include "badger_pf.h"

namespace amd = badger_amcl_amd;

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
};

// map, scanner, model and the filter (GLOBAL bounds) of one engine
static std::shared_ptr<amd::ParticleFilter> make_filter(std::shared_ptr<amd::Engine> eng, const Inputs& in)
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
  pf->setResampleModel(amd::PF_RESAMPLE_MULTINOMIAL);
  eng->check(bpf_pf_set_kld_count(e, in.i("kld")));
  pf->srand48(in.i("seed"));
  return pf;
}

// rank r's slice of the loaded set
static void load_slice(amd::ParticleFilter& pf, const Inputs& in, int lo, int hi)
{
  bpf_engine* e = pf.engine().get();
  if (hi > lo)
    pf.engine().check(bpf_pf_set_samples(e, in.samples.data() + 4 * (size_t)lo, hi - lo, in.i("leaf")));
  else  // a shard without samples
    pf.engine().check(bpf_shard_adopt_dev(e, nullptr, nullptr, nullptr, 0, in.n(), 0, 0));
}

static void dump(const Inputs& in, const std::string& name, amd::ParticleFilter& pf)
{
  std::vector<double> s((size_t)in.i("max_samples") * 4 + 4);
  int got = 0;
  if (pf.getState().sample_count > 0)  // (a shard without samples: an empty file)
    pf.engine().check(bpf_pf_get_samples(pf.engine().get(), s.data(), in.i("max_samples"), &got));
  FILE* f = std::fopen((in.dir + "/" + name).c_str(), "wb");
  if (!f) std::exit(3);
  std::fwrite(s.data(), sizeof(double), (size_t)got * 4, f);
  std::fclose(f);
}

static std::shared_ptr<amd::PlanarData> scan(const Inputs& in)
{
  auto data = std::make_shared<amd::PlanarData>();
  data->range_count_ = (int)in.ranges.size();
  data->range_max_ = in.v("range_max");
  data->ranges_ = in.ranges;
  data->angles_ = in.angles;
  return data;
}

static void rank_line(int r, amd::ShardedParticleFilter& sf, long long before, long long after)
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

static int run_unsharded(const Inputs& in)
{
  auto one = make_filter(std::make_shared<amd::Engine>(0), in);
  bpf_engine* e = one->engine().get();
  one->engine().check(bpf_pf_set_samples(e, in.samples.data(), in.n(), in.i("leaf")));
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

static int run_local(const Inputs& in, int W)
{
  std::vector<std::shared_ptr<amd::ParticleFilter>> pfs;
  std::vector<int> counts;
  for (int r = 0; r < W; ++r)
  {
    pfs.push_back(make_filter(std::make_shared<amd::Engine>(0), in));
    load_slice(*pfs.back(), in, in.cut(r, W), in.cut(r + 1, W));
    counts.push_back(in.cut(r + 1, W) - in.cut(r, W));
  }
  amd::LocalShardedParticleFilter local(pfs, counts, in.i("leaf"), 4096);
  int mode = -1;
  bpf_shard_exchange_mode(pfs[0]->engine().get(), &mode);
  std::printf("mode %d\n", mode);
  local.setResampleForm(BPF_SHARD_RESAMPLE_WINDOW, in.v("max_share"));  // (the cap both forms share)
  local.setMultinomialForm(BPF_SHARD_RESAMPLE_IN_PLACE);
  local.updateSensor(scan(in));
  std::vector<long long> before((size_t)W), after((size_t)W);
  for (int r = 0; r < W; ++r)
    bpf_shard_exchange_count(pfs[(size_t)r]->engine().get(), &before[(size_t)r]);
  local.updateResample();
  for (int r = 0; r < W; ++r)
    bpf_shard_exchange_count(pfs[(size_t)r]->engine().get(), &after[(size_t)r]);
  for (int r = 0; r < W; ++r)
  {
    dump(in, "rank" + std::to_string(r) + ".resample.bin", *pfs[(size_t)r]);
    rank_line(r, local.rank(r), before[(size_t)r], after[(size_t)r]);
  }
  // the step after it takes the slices where they are: a motion update needs every rank's first global index
  auto odo = std::make_shared<amd::OdomData>();
  odo->pose = { 1.0, 2.0, 0.3 };
  odo->delta = { 0.03, -0.01, 0.02 };
  odo->absolute_motion = { 0.03, 0.01, 0.02 };
  for (auto& p : pfs)
    p->engine().check(bpf_odom_set_model(p->engine().get(), BPF_ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.04, 0.03, 0.02, 0.0));
  local.updateAction(odo);
  local.updateSensor(scan(in));
  std::printf("next step ok form %d\n", local.formUsed());
  local.shutdown();
  return run_unsharded(in);
}

static int run_rank(const Inputs& in, int rank, int W, int port, int flags)
{
  auto pf = make_filter(std::make_shared<amd::Engine>(0), in);
  load_slice(*pf, in, in.cut(rank, W), in.cut(rank + 1, W));
  amd::ShardedParticleFilter sf(pf, in.n(), in.i("leaf"), 4096, in.cut(rank, W));
  const int mode = sf.bootstrap(rank, W, "127.0.0.1:" + std::to_string(port), in.i("max_samples"), flags);
  std::printf("mode %d\n", mode);
  sf.setResampleForm(BPF_SHARD_RESAMPLE_WINDOW, in.v("max_share"));  // (the cap both forms share)
  sf.setMultinomialForm(BPF_SHARD_RESAMPLE_IN_PLACE);
  sf.updateSensor(scan(in));
  long long before = 0, after = 0;
  bpf_shard_exchange_count(pf->engine().get(), &before);
  sf.updateResample();
  bpf_shard_exchange_count(pf->engine().get(), &after);
  dump(in, "rank" + std::to_string(rank) + ".resample.bin", *pf);
  rank_line(rank, sf, before, after);
  sf.shutdown();
  return 0;
}

int main(int argc, char** argv)
{
  if (argc != 6)
  {
    std::fprintf(stderr, "usage: dir mode world port flags\n");
    return 2;
  }
  Inputs in;
  in.dir = argv[1];
  {
    std::ifstream f(in.dir + "/cfg.txt");
    std::string line, key;
    while (std::getline(f, line))
    {
      std::istringstream ss(line);
      ss >> key;
      double x;
      while (ss >> x)
        in.cfg[key].push_back(x);
    }
  }
  if (!in.cfg.count("max_samples"))
  {
    std::fprintf(stderr, "no cfg.txt in %s\n", in.dir.c_str());
    return 2;
  }
  in.cells = slurp<int32_t>(in.dir + "/cells.bin");
  in.lut = slurp<float>(in.dir + "/lut.bin");
  in.samples = slurp<double>(in.dir + "/samples.bin");
  in.ranges = slurp<double>(in.dir + "/ranges.bin");
  in.angles = slurp<double>(in.dir + "/angles.bin");
  const int mode = std::atoi(argv[2]), W = std::atoi(argv[3]), port = std::atoi(argv[4]), flags = std::atoi(argv[5]);
  if (mode == 0)
  {
    try
    {
      return run_local(in, W);
    }
    catch (const std::exception& err)
    {
      std::fprintf(stderr, "shard_in_place_mn: %s\n", err.what());
      return 1;
    }
  }
  // fork BEFORE anything touches the GPU: every child initialises HIP for itself
  std::vector<pid_t> kids;
  for (int r = -1; r < W; ++r)
  {
    const pid_t pid = fork();
    if (pid == 0)
    {
      const std::string out = in.dir + "/" + (r < 0 ? std::string("single") : "rank" + std::to_string(r)) + ".txt";
      if (!std::freopen(out.c_str(), "w", stdout))
        _exit(3);
      int rc = 9;
      try
      {
        rc = r < 0 ? run_unsharded(in) : run_rank(in, r, W, port, flags);
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
