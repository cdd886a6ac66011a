// A sharded filter STARTED from plain C++ processes: this program forks one process per rank (all on GPU 0) plus one
// that runs the same filter unsharded.  Every rank bootstraps, then runs through badger_amcl_amd::ShardedParticleFilter
//   initWithGaussian | initWithRandomPoses -> updateAction -> updateSensor -> updateResample -> getMaxWeightPose
// and the unsharded process the same steps on one ParticleFilter.  Every process dumps its set after the init, the
// motion update and the resample and prints its figures; tests/test_gpu_cpp_shard_init.py compares.
//
// usage: shard_init dir world port flags kind n resampler size      (kind 0: Gaussian, 1: random free-space poses)
// dir holds cells.bin lut.bin ranges.bin angles.bin mean.bin (3 doubles) and takes the dumps
#include "shard_harness.hpp"

struct InitInputs
{
  std::string dir;
  std::vector<int32_t> cells;
  std::vector<float> lut;
  std::vector<double> ranges, angles, mean;
  int size = 0, n = 0, kind = 0, resampler = 0;
};

static const std::array<double, 9> kRot = { 0.8, -0.6, 0.0, 0.6, 0.8, 0.0, 0.0, 0.0, 1.0 };
static const std::array<double, 3> kSigma = { 0.15, 0.1, 0.05 };

static int setup(bpf_engine* e, const InitInputs& in, int rank)
{
  const float origin = (float)((in.size / 2) * 0.05);
  CHECK(e, bpf_map2d_set(e, in.cells.data(), in.lut.data(), in.size, in.size, origin, origin, 0.05, 2.0));
  CHECK(e, bpf_planar_init(e, (int)in.ranges.size()));
  CHECK(e, bpf_planar_set_model_likelihood_field(e, 0.95, 0.05, 0.2, 2.0));
  CHECK(e, bpf_planar_set_map_factors(e, 0.95, 0.95, 0.3));
  const double pose[3] = { 0.1, -0.05, 0.2 };
  CHECK(e, bpf_planar_set_scanner_pose(e, pose));
  return 0;
}

static std::shared_ptr<amd::ParticleFilter> make_filter(std::shared_ptr<amd::Engine> eng, const InitInputs& in)
{
  auto pf = std::make_shared<amd::ParticleFilter>(eng, 100, in.n, 0.0, 0.0, 85.0);  // the GLOBAL bounds on every rank
  pf->srand48(42);
  pf->setResampleModel((amd::PFResampleModelType)in.resampler);
  pf->setRandomFreeSpacePoseGenerator(true);
  return pf;
}

static int dump_set(bpf_engine* e, const InitInputs& in, int rank, const std::string& name)
{
  return dump_set(e, in.dir, in.n, rank, name);
}

static int print_state(bpf_engine* e, int rank, const char* tag, long long first, int global, int leaf, int bins)
{
  bpf_pf_state st;
  CHECK(e, bpf_pf_get_state(e, &st));
  uint64_t rng = 0;
  CHECK(e, bpf_pf_get_rng_state(e, &rng));
  std::printf("%s first %lld global %d leaf %d bins %d local %d eleaf %d ebins %d rng %llu conv %d wslow %a wfast %a\n", tag,
              first, global, leaf, bins, st.sample_count, st.leaf_count, st.bin_count, (unsigned long long)rng,
              st.converged, st.w_slow, st.w_fast);
  std::fflush(stdout);
  return 0;
}

static int run_rank_body(const InitInputs& in, int rank, int world, int port, int flags)
{
  auto eng = std::make_shared<amd::Engine>(0);
  bpf_engine* e = eng->get();
  if (int rc = setup(e, in, rank))
    return rc;
  auto pf = make_filter(eng, in);
  amd::ShardedParticleFilter sf(pf, in.n, 1, 4096);
  {
    // no exchange yet: the one-call forms say so, and change nothing
    int a = 0, b = 0;
    std::printf("unconfigured %d %d\n", bpf_shard_init_with_random_poses_all(e), bpf_shard_global_leaf_count(e, &a, &b));
  }
  const int mode = sf.bootstrap(rank, world, "127.0.0.1:" + std::to_string(port), in.n, flags);
  long long x0 = 0, x1 = 0, x2 = 0;
  CHECK(e, bpf_shard_exchange_count(e, &x0));
  if (in.kind == 0)
    sf.initWithGaussian({ in.mean[0], in.mean[1], in.mean[2] }, kRot, kSigma);
  else
    sf.initWithRandomPoses();
  CHECK(e, bpf_shard_exchange_count(e, &x1));
  int leaf2 = 0, bins2 = 0;
  CHECK(e, bpf_shard_global_leaf_count(e, &leaf2, &bins2));  // in force: the same figures, no exchange
  CHECK(e, bpf_shard_exchange_count(e, &x2));
  std::printf("mode %d exch %lld %lld %lld again %d %d route %d\n", mode, x0, x1, x2, leaf2, bins2, sf.treeRoute());
  if (int rc = dump_set(e, in, rank, "rank" + std::to_string(rank) + ".init.bin"))
    return rc;
  if (int rc = print_state(e, rank, "init", sf.globalFirst(), sf.globalSampleCount(), sf.leafCount(), sf.binCount()))
    return rc;
  amd::Odom od(eng);
  od.setModel(amd::ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.04, 0.03, 0.02, 0.0);
  sf.updateAction(odom_data());
  if (int rc = dump_set(e, in, rank, "rank" + std::to_string(rank) + ".moved.bin"))
    return rc;
  auto d = std::make_shared<amd::PlanarData>();
  d->range_count_ = (int)in.ranges.size();
  d->range_max_ = 30.0;
  d->ranges_ = in.ranges;
  d->angles_ = in.angles;
  sf.updateSensor(d);
  sf.updateResample();
  if (int rc = dump_set(e, in, rank, "rank" + std::to_string(rank) + ".resample.bin"))
    return rc;
  if (int rc = print_state(e, rank, "resample", sf.globalFirst(), sf.globalSampleCount(), sf.leafCount(), sf.binCount()))
    return rc;
  double w = 0;
  std::array<double, 3> p{};
  sf.getMaxWeightPose(&w, &p);
  std::printf("pose %a %a %a %a miss %d\n", w, p[0], p[1], p[2], sf.cdfMiss() ? 1 : 0);
  std::fflush(stdout);
  sf.shutdown();
  return 0;
}

// the same filter on one engine through the ordinary entry points
static int run_unsharded_body(const InitInputs& in)
{
  const int rank = -1;
  auto eng = std::make_shared<amd::Engine>(0);
  bpf_engine* e = eng->get();
  if (int rc = setup(e, in, rank))
    return rc;
  auto pf = make_filter(eng, in);
  if (in.kind == 0)
    pf->initWithGaussian({ in.mean[0], in.mean[1], in.mean[2] }, kRot, kSigma);
  else
    pf->initWithRandomPoses();
  if (int rc = dump_set(e, in, rank, "single.init.bin"))
    return rc;
  bpf_pf_state st = pf->getState();
  if (int rc = print_state(e, rank, "init", 0, st.sample_count, st.leaf_count, st.bin_count))
    return rc;
  amd::Odom od(eng);
  od.setModel(amd::ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.04, 0.03, 0.02, 0.0);
  od.updateAction(pf, odom_data());
  if (int rc = dump_set(e, in, rank, "single.moved.bin"))
    return rc;
  CHECK(e, bpf_pf_update_sensor_planar(e, in.ranges.data(), in.angles.data(), (int)in.ranges.size(), 30.0));
  pf->updateResample();
  if (int rc = dump_set(e, in, rank, "single.resample.bin"))
    return rc;
  st = pf->getState();
  if (int rc = print_state(e, rank, "resample", 0, st.sample_count, st.leaf_count, st.bin_count))
    return rc;
  double w = 0;
  std::array<double, 3> p{};
  pf->getMaxWeightPose(&w, &p);
  std::printf("pose %a %a %a %a miss 0\n", w, p[0], p[1], p[2]);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 9)
  {
    std::fprintf(stderr, "usage: dir world port flags kind n resampler size\n");
    return 2;
  }
  InitInputs in;
  in.dir = argv[1];
  const int world = std::atoi(argv[2]), port = std::atoi(argv[3]), flags = std::atoi(argv[4]);
  in.kind = std::atoi(argv[5]);
  in.n = std::atoi(argv[6]);
  in.resampler = std::atoi(argv[7]);
  in.size = std::atoi(argv[8]);
  in.cells = slurp<int32_t>(in.dir + "/cells.bin");
  in.lut = slurp<float>(in.dir + "/lut.bin");
  in.ranges = slurp<double>(in.dir + "/ranges.bin");
  in.angles = slurp<double>(in.dir + "/angles.bin");
  in.mean = slurp<double>(in.dir + "/mean.bin");
  if (in.mean.size() != 3)
    return 2;
  return fork_ranks(in.dir, world,
                    [&](int r) { return r < 0 ? run_unsharded_body(in) : run_rank_body(in, r, world, port, flags); });
}
