// Rebalancing the slices of a sharded filter through the one-call forms (bpf_shard_rebalance, and
// BPF_SHARD_REBALANCE_AUTO behind bpf_shard_update_resample), beside the same filter unsharded: slices loaded unevenly,
// a stand-alone rebalance(), then one sensor update and one in-place resample with AUTO at trigger_share = 1.
//
//   mode 0   badger_amcl_amd::LocalShardedParticleFilter: all `world` ranks in this process (the local exchange)
//   mode 1   one forked process per rank through badger_amcl_amd::ShardedParticleFilter::bootstrap: the mailbox, or
//            RCCL with BPF_BOOTSTRAP_FORCE_COLLECTIVE in `flags`
//
// Every rank dumps its slice behind the rebalance and behind the resample and prints where it sits, how many samples
// moved and the exchange count around both; the unsharded engine dumps the set it loaded and its resampled set and
// prints the rng state before its resample, from which tests/test_gpu_cpp_shard_rebalance.py forms the rotation.  Every
// wait inside the library is bounded by the exchange time-out (5 s, bpf_shard_mailbox_set_timeout_ms).
//
// usage: shard_rebalance dir mode world port flags     (dir holds cfg.txt and the binary inputs, and takes the dumps)
#include "shard_harness.hpp"

static const amd::PFResampleModelType kModel = amd::PF_RESAMPLE_SYSTEMATIC;

static void rebalance_line(int r, amd::ShardedParticleFilter& sf, long long moved, long long before, long long after)
{
  const bpf_pf_state st = sf.filter().getState();
  std::printf("rebalance %d moved %lld local %d first %lld leaf %d bins %d exch0 %lld exch1 %lld\n", r, moved,
              st.sample_count, sf.globalFirst(), st.leaf_count, st.bin_count, before, after);
  std::fflush(stdout);
}

// rank_line of shard_harness.hpp with the samples the AUTO rebalance moved
static void moved_rank_line(int r, amd::ShardedParticleFilter& sf, long long before, long long after)
{
  amd::ParticleFilter& pf = sf.filter();
  const bpf_pf_state st = pf.getState();
  uint64_t rng = 0;
  pf.engine().check(bpf_pf_get_rng_state(pf.engine().get(), &rng));
  std::printf("rank %d M %d leaf %d bins %d windows %d local %d first %lld form %d rng %llu miss %d conv %d eleaf %d "
              "ebins %d moved %lld exch0 %lld exch1 %lld\n", r, sf.globalSampleCount(), sf.leafCount(), sf.binCount(),
              sf.windowsUsed(), st.sample_count, sf.globalFirst(), sf.formUsed(), (unsigned long long)rng,
              sf.cdfMiss() ? 1 : 0, st.converged, st.leaf_count, st.bin_count, sf.rebalanced(), before, after);
  std::fflush(stdout);
}

static int run_local(const Inputs& in, int W)
{
  LocalRanks L(in, W, kModel);
  amd::LocalShardedParticleFilter local(L.pfs, L.counts, in.i("leaf"), 4096);
  int mode = -1;
  bpf_shard_exchange_mode(L.pfs[0]->engine().get(), &mode);
  std::printf("mode %d\n", mode);
  local.setResampleForm(BPF_SHARD_RESAMPLE_IN_PLACE, in.v("max_share"));
  std::vector<long long> before = exchange_counts(L.pfs);
  const long long moved = local.rebalance();
  std::vector<long long> after = exchange_counts(L.pfs);
  for (int r = 0; r < W; ++r)
  {
    dump(in, "rank" + std::to_string(r) + ".rebalance.bin", *L.pfs[(size_t)r]);
    rebalance_line(r, local.rank(r), moved, before[(size_t)r], after[(size_t)r]);
  }
  local.setRebalance(BPF_SHARD_REBALANCE_AUTO, 1.0);
  local.updateSensor(scan(in));
  before = exchange_counts(L.pfs);
  local.updateResample();
  after = exchange_counts(L.pfs);
  for (int r = 0; r < W; ++r)
  {
    dump(in, "rank" + std::to_string(r) + ".resample.bin", *L.pfs[(size_t)r]);
    moved_rank_line(r, local.rank(r), before[(size_t)r], after[(size_t)r]);
  }
  next_step(local, L, in);
  local.shutdown();
  return run_unsharded(in, kModel, true);
}

// what a refused call left behind: the status the engine keeps, where the slice sits, the samples themselves
static void refused_line(const char* what, int rank, bool threw, amd::ShardedParticleFilter& sf)
{
  bpf_engine* e = sf.filter().engine().get();
  const bpf_pf_state st = sf.filter().getState();
  long long last = -1;
  bpf_shard_rebalance_last(e, &last);
  uint64_t rng = 0;
  bpf_pf_get_rng_state(e, &rng);
  std::printf("%s %d threw %d status %d local %d first %lld M %d committed %d last %lld moved %lld form %d rng %llu\n", what,
              rank, threw ? 1 : 0, st.last_status, st.sample_count, sf.globalFirst(), sf.globalSampleCount(),
              sf.resampleCommitted() ? 1 : 0, last, sf.rebalanced(), sf.formUsed(), (unsigned long long)rng);
  std::fflush(stdout);
}

static int run_rank_refused(const Inputs& in, int rank, amd::ShardedParticleFilter& sf)
{
  amd::ParticleFilter& pf = sf.filter();
  bool threw = false;
  try
  {
    sf.rebalance();
  }
  catch (const std::exception&)
  {
    threw = true;
  }
  dump(in, "rank" + std::to_string(rank) + ".rebalance.bin", pf);
  refused_line("norebalance", rank, threw, sf);
  sf.setRebalance(BPF_SHARD_REBALANCE_AUTO, 1.0);
  sf.updateSensor(scan(in));
  threw = false;
  try
  {
    sf.updateResample();
  }
  catch (const std::exception&)
  {
    threw = true;
  }
  dump(in, "rank" + std::to_string(rank) + ".resample.bin", pf);
  refused_line("noauto", rank, threw, sf);
  sf.shutdown();
  return 0;
}

static int run_rank(const Inputs& in, int rank, int W, int port, int flags)
{
  auto pf = make_filter(std::make_shared<amd::Engine>(0), in, kModel);
  load_slice(*pf, in, in.cut(rank, W), in.cut(rank + 1, W));
  amd::ShardedParticleFilter sf(pf, in.n(), in.i("leaf"), 4096, in.cut(rank, W));
  // cfg "window": mailbox windows too small for the moved rows (4 T > 6 window words): both rebalances are refused with
  // BPF_ERR_CAPACITY, the stand-alone one with the old slice current, AUTO's with the resampled, uneven slice current
  const bool small = in.cfg.count("window") != 0;
  const int mode = sf.bootstrap(rank, W, "127.0.0.1:" + std::to_string(port), small ? in.i("window") : in.i("max_samples"),
                                flags);
  std::printf("mode %d\n", mode);
  sf.setResampleForm(BPF_SHARD_RESAMPLE_IN_PLACE, in.v("max_share"));
  long long before = 0, after = 0;
  if (small)
    return run_rank_refused(in, rank, sf);
  bpf_shard_exchange_count(pf->engine().get(), &before);
  const long long moved = sf.rebalance();
  bpf_shard_exchange_count(pf->engine().get(), &after);
  dump(in, "rank" + std::to_string(rank) + ".rebalance.bin", *pf);
  rebalance_line(rank, sf, moved, before, after);
  sf.setRebalance(BPF_SHARD_REBALANCE_AUTO, 1.0);
  sf.updateSensor(scan(in));
  bpf_shard_exchange_count(pf->engine().get(), &before);
  sf.updateResample();
  bpf_shard_exchange_count(pf->engine().get(), &after);
  dump(in, "rank" + std::to_string(rank) + ".resample.bin", *pf);
  moved_rank_line(rank, sf, before, after);
  sf.shutdown();
  return 0;
}

int main(int argc, char** argv)
{
  const ShardProgram program{ "shard_rebalance", run_local, [](const Inputs& in) { return run_unsharded(in, kModel, true); },
                              run_rank };
  return program.main(argc, argv);
}
