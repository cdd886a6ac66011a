// libbadger_pf_hip.so -- host engine and C-ABI (include/badger_pf.h) for the MI355X
// sensor-update + resample path.  gfx950 only.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <optional>
#include <functional>
#include <queue>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/badger_pf.h"
#include "device_types.hpp"
#include "kdhist.hpp"
#include "host_poll.hpp"
#include "kernels_cloud.hpp"
#include "kernels_lut3d.hpp"
#include "kernels_motion.hpp"
#include "kernels_mixture.hpp"
#include "kernels_kld.hpp"
#include "kernels_kld2.hpp"
#include "kernels_kld_bins.hpp"
#include "kernels_recovery.hpp"
#include "kernels_pf.hpp"
#include "kernels_pose_array.hpp"
#include "kernels_pose_search.hpp"
#include "kernels_pose_search_joint.hpp"
#include "kernels_pose_refine.hpp"
#include "kernels_pose_moments.hpp"
#include "kernels_fused.hpp"
#include "kernels_stats.hpp"
#include "kernels_shard_stats.hpp"
#include "kernels_shard_init.hpp"
#include "kernels_shard_inplace.hpp"
#include "kernels_shard_inplace_mn.hpp"
#include "kernels_shard_rebalance.hpp"
#include "kernels_score.hpp"
#include "kernels_window.hpp"
#include "kernels_pose_search_pruned.hpp"
#include "kernels_pose_search_cloud_pruned.hpp"

using namespace bpf;

#include "engine_state.hpp"
#include "host_copy.hpp"

namespace
{
#include "host_common.inl"
#include "host_scoring.inl"
#include "host_resample.inl"
}  // namespace

// ====================================================================== C-ABI (include/badger_pf.h)
extern "C" {
namespace
{
void mailbox_release(bpf_engine* e);     // abi_mailbox.inl
void collective_release(bpf_engine* e);  // abi_bootstrap.inl
void host_buffers_release(bpf_engine* e);  // abi_hostbuf.inl
}
#include "abi_lifecycle.inl"
#include "abi_hostbuf.inl"
#include "abi_map2d.inl"
#include "abi_planar.inl"
#include "abi_filter.inl"
#include "abi_mixture.inl"
#include "abi_motion.inl"
#include "abi_statistics.inl"
#include "abi_lut_reference.inl"
#include "abi_wire.inl"
#include "abi_cloud3d.inl"
#include "abi_mailbox.inl"
#include "abi_sharded.inl"
#include "abi_shard_stats.inl"
#include "abi_shard_init.inl"
#include "abi_mailbox_step.inl"
#include "abi_shard_node.inl"
#include "abi_shard_inplace.inl"
#include "abi_shard_inplace_mn.inl"
#include "abi_shard_rebalance.inl"
#include "abi_pose_array.inl"
#include "abi_pose_search.inl"
#include "abi_pose_search_cloud.inl"
#include "abi_pose_search_joint.inl"
#include "abi_pose_search_pruned.inl"
#include "abi_pose_search_cloud_pruned.inl"
#include "abi_shard_search.inl"
#include "abi_pose_refine.inl"
#include "abi_pose_moments.inl"
#include "abi_bootstrap.inl"
#include "abi_shard_local.inl"
#include "abi_measure.inl"
}  // extern "C"
