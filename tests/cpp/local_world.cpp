// A sharded filter with all its ranks in ONE process, as a single-process node would hold it:
// badger_amcl_amd::LocalShardedParticleFilter over `world` engines on GPU 0, beside the same filter unsharded on one
// more engine, in one program and with no fork, socket or IPC handle.  Every cycle is motion, sensor, resample; after
// each sensor update and each resample the ranks' slices and the single engine's set are dumped, and the global pose
// (bpf_shard_get_max_weight_pose, cluster 0, the particle cloud) is printed next to that of a third engine loaded with
// the concatenation of the ranks' slices.  tests/test_gpu_cpp_local_world.py compares.
//
// usage: local_world dir        (dir holds cfg.txt and the binary inputs, as for shard_node, and takes the dumps)
#include "shard_harness.hpp"

// map, scanner, model, odometry and the filter (GLOBAL bounds) of one engine
static std::shared_ptr<amd::ParticleFilter> make_filter(std::shared_ptr<amd::Engine> eng, const Inputs& in)
{
  auto pf = make_filter(eng, in, in.i("resampler") ? amd::PF_RESAMPLE_SYSTEMATIC : amd::PF_RESAMPLE_MULTINOMIAL);
  eng->check(bpf_odom_set_model(eng->get(), BPF_ODOM_MODEL_DIFF_CORRECTED, 0.05, 0.04, 0.03, 0.02, 0.0));
  return pf;
}

static std::vector<amd::PFSample> slice(const Inputs& in, int lo, int hi)
{
  std::vector<amd::PFSample> s((size_t)(hi - lo));
  std::memcpy(s.data(), in.samples.data() + 4 * (size_t)lo, s.size() * sizeof(amd::PFSample));
  return s;
}

static void dump(const Inputs& in, const std::string& name, const std::vector<amd::PFSample>& s)
{
  if (dump(in.dir + "/" + name, s.data(), s.size() * sizeof(amd::PFSample)) != 0)
    std::exit(3);
}

static std::string pose_line(double w, const std::array<double, 3>& p, bool have, double cw, const std::array<double, 3>& cm)
{
  char buf[400];
  std::snprintf(buf, sizeof buf, "best %a %a %a %a cluster0 %d %a %a %a %a", w, p[0], p[1], p[2], have ? 1 : 0, cw, cm[0],
                cm[1], cm[2]);
  return buf;
}

int main(int argc, char** argv)
{
  if (argc != 2)
    return 2;
  Inputs in;
  if (!in.read(argv[1]))
    return 2;
  const int W = in.i("world"), n = (int)in.samples.size() / 4, cycles = in.i("cycles");
  try
  {
    std::vector<std::shared_ptr<amd::ParticleFilter>> pfs;
    std::vector<int> counts;
    for (int r = 0; r < W; ++r)
    {
      pfs.push_back(make_filter(std::make_shared<amd::Engine>(0), in));
      const int lo = (int)((long long)n * r / W), hi = (int)((long long)n * (r + 1) / W);
      pfs.back()->initWithSamples(slice(in, lo, hi), 1);
      counts.push_back(hi - lo);
    }
    auto one = make_filter(std::make_shared<amd::Engine>(0), in);
    one->initWithSamples(slice(in, 0, n), 1);
    auto concat_engine = std::make_shared<amd::Engine>(0);
    amd::ParticleFilter concat(concat_engine, in.i("min_samples"), in.i("max_samples"), 0.0, 0.0, 85.0);

    int mode = -1;
    bpf_shard_exchange_mode(pfs[0]->engine().get(), &mode);
    std::printf("before mode %d\n", mode);
    amd::LocalShardedParticleFilter local(pfs, counts, 1, 4096);
    bpf_shard_exchange_mode(pfs[W - 1]->engine().get(), &mode);
    std::printf("local mode %d world %d\n", mode, local.world());

    const auto data = scan(in);
    const auto odo = odom_data();

    // the ranks' slices dumped and concatenated; the global pose of the world next to one engine holding them
    auto compare = [&](int cycle, const char* step) {
      std::vector<std::vector<amd::PFSample>> sets((size_t)W);
      local.forEachRank([&](int r, amd::ParticleFilter& pf) { sets[(size_t)r] = pf.getCurrentSet()->samples; });
      std::vector<amd::PFSample> whole;
      for (int r = 0; r < W; ++r)
      {
        dump(in, "rank" + std::to_string(r) + ".c" + std::to_string(cycle) + "." + step + ".bin", sets[(size_t)r]);
        whole.insert(whole.end(), sets[(size_t)r].begin(), sets[(size_t)r].end());
      }
      dump(in, std::string("single.c") + std::to_string(cycle) + "." + step + ".bin", one->getCurrentSet()->samples);
      concat.initWithSamples(whole);
      double w = 0, cw = 0, w1 = 0, cw1 = 0;
      std::array<double, 3> p{}, cm{}, p1{}, cm1{};
      long long before = 0, mid = 0, after = 0;
      bpf_shard_exchange_count(pfs[0]->engine().get(), &before);
      local.getMaxWeightPose(&w, &p);
      const bool have = local.getClusterStats(0, &cw, &cm);
      bpf_shard_exchange_count(pfs[0]->engine().get(), &mid);
      local.getMaxWeightPose(&w, &p);  // nothing changed: no exchange
      bpf_shard_exchange_count(pfs[0]->engine().get(), &after);
      concat.getMaxWeightPose(&w1, &p1);
      const bool have1 = concat.getClusterStats(0, &cw1, &cm1);
      std::vector<double> cloud, cloud1;
      local.getPoseArray(&cloud, 1, 3);
      concat.getPoseArray(&cloud1, 1, 3);
      const int same_cloud = cloud.size() == cloud1.size() && !cloud.empty() &&
                             std::memcmp(cloud.data(), cloud1.data(), cloud.size() * sizeof(double)) == 0;
      std::printf("pose %s %d local %s\n", step, cycle, pose_line(w, p, have, cw, cm).c_str());
      std::printf("pose %s %d concat %s\n", step, cycle, pose_line(w1, p1, have1, cw1, cm1).c_str());
      std::printf("lazy %s %d first %d second %d cloud %d poses %d\n", step, cycle, (int)(mid > before), (int)(after - mid),
                  same_cloud, (int)(cloud.size() / 7));
    };

    for (int cycle = 0; cycle < cycles; ++cycle)
    {
      local.updateAction(odo);
      one->engine().check(bpf_pf_update_action(one->engine().get(), odo->pose.data(), odo->delta.data(),
                                               odo->absolute_motion.data()));
      local.updateSensor(data);
      one->engine().check(bpf_pf_update_sensor_planar(one->engine().get(), in.ranges.data(), in.angles.data(),
                                                      (int)in.ranges.size(), in.v("range_max")));
      compare(cycle, "sensor");
      local.updateResample();
      one->updateResample();
      compare(cycle, "resample");
      const bpf_pf_state s1 = one->getState();
      uint64_t rng = 0;
      one->engine().check(bpf_pf_get_rng_state(one->engine().get(), &rng));
      std::printf("single cycle %d M %d leaf %d bins %d rng %llu conv %d\n", cycle, s1.sample_count, s1.leaf_count,
                  s1.bin_count, (unsigned long long)rng, s1.converged);
      for (int r = 0; r < W; ++r)
      {
        bpf_engine* e = pfs[(size_t)r]->engine().get();
        const bpf_pf_state st = pfs[(size_t)r]->getState();
        long long exch = 0;
        bpf_pf_get_rng_state(e, &rng);
        bpf_shard_exchange_count(e, &exch);
        std::printf("rank %d cycle %d M %d leaf %d bins %d windows %d local %d rng %llu miss %d conv %d exch %lld\n", r, cycle,
                    local.rank(r).globalSampleCount(), local.rank(r).leafCount(), local.rank(r).binCount(),
                    local.rank(r).windowsUsed(), st.sample_count, (unsigned long long)rng, local.rank(r).cdfMiss() ? 1 : 0,
                    st.converged, exch);
      }
    }
    local.shutdown();
    bpf_shard_exchange_mode(pfs[0]->engine().get(), &mode);
    std::printf("after mode %d\n", mode);
  }
  catch (const std::exception& err)
  {
    std::fprintf(stderr, "local_world: %s\n", err.what());
    return 1;
  }
  return 0;
}
