// The systematic resample of a sharded filter IN PLACE through the one-call form (bpf_shard_update_resample with
// BPF_SHARD_RESAMPLE_IN_PLACE set), beside the same filter unsharded: one sensor update and one resample.
//
//   mode 0   badger_amcl_amd::LocalShardedParticleFilter: all `world` ranks in this process (the local exchange)
//   mode 1   one forked process per rank through badger_amcl_amd::ShardedParticleFilter::bootstrap: the mailbox, or
//            RCCL with BPF_BOOTSTRAP_FORCE_COLLECTIVE in `flags`
//
// Every rank dumps its slice and prints where it sits, the figures of the resample and the exchange count before and
// behind it; the unsharded engine prints the rng state before its resample, from which
// tests/test_gpu_cpp_shard_in_place.py forms the rotation.  Every wait inside the library is bounded by the exchange
// time-out (5 s, bpf_shard_mailbox_set_timeout_ms).  The program itself is in_place_program of shard_harness.hpp.
//
// usage: shard_in_place dir mode world port flags     (dir holds cfg.txt and the binary inputs, and takes the dumps)
#include "shard_harness.hpp"

int main(int argc, char** argv)
{
  const auto set_form = [](auto& filter, const Inputs& in) {
    filter.setResampleForm(BPF_SHARD_RESAMPLE_IN_PLACE, in.v("max_share"));
  };
  return in_place_program("shard_in_place", amd::PF_RESAMPLE_SYSTEMATIC, set_form).main(argc, argv);
}
