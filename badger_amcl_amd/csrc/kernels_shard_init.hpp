// A SHARDED set started on its ranks, and the histogram tree of the GLOBAL set without moving a particle.
//
//   init         rank r writes samples [first, first + n) of the set ONE engine would produce: the Gaussian form reads
//                its index range of the global Gaussian stream (generate_gaussians, k_init_gaussian as it is); the
//                free-space form finds call (first + i)'s stream element directly (k_init_free_space_range).
//   tree         the shape of PFKDTree depends only on the order in which DISTINCT keys first appear (pf_kdtree.cpp:
//                97-150: an equal key only adds to `value`), so the bins cross, not the particles:
//     local bins   the slice's distinct packed keys with the global index of each key's first sample, in first-index
//                  order (k_set_keys, k_kld_hash, k_sstat_first_count, k_stats_scan_offsets, k_sstat_compact)
//     -- exchange: all-gather of the lists, int64[world][2][pad] --
//     merge        one table in which a key keeps its smallest first index (k_gtree_insert: a rank's list holds a key
//                  once, so a slot sees at most `world` atomics); the entries that ARE their key's first occurrence
//                  counted per tile (k_gtree_first_count: one ballot per wave and step), scanned (k_stats_scan_offsets)
//                  and compacted, unpacked, in rank-then-list order (k_gtree_compact).  The shards are contiguous, so
//                  that is increasing first-index order: the order the one engine inserts its distinct keys in.
//     tree         the existing device tree, or the host tree, on those distinct keys (abi_shard_init.inl).
//
// No kernel here waits for another rank.  Every probe loop is bounded by the table size; a bound that is hit sets
// flags[3] (it cannot be with a table of at least twice the entries) and is reported as an error.
#pragma once
#include "kernels_motion.hpp"
#include "kernels_shard_stats.hpp"

namespace bpf
{

// ParticleFilter::initWithPoseFn (particle_filter.cpp:135-163) for samples [first, first + n) of the global set:
// k_init_free_space with the call index offset
__global__ void k_init_free_space_range(ParticlesDev dst, int n, long long first, uint64_t rng_state, LcgJump jump,
                                        FreeSpaceDev F, double weight)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const uint64_t xs = lcg_skip(rng_state, free_space_call_elem(F, 1, (uint64_t)(first + i)), jump);
  double x, y, th;
  random_free_space_pose(F, ldexp((double)xs, -48), ldexp((double)lcg_next(xs), -48), &x, &y, &th);
  dst.x[i] = x;
  dst.y[i] = y;
  dst.th[i] = th;
  dst.w[i] = weight;
}

struct GlobalTreeArgs
{
  const long long* all;              // [world][2][pad]: the gathered lists (packed key, global first index)
  int world, pad;
  int counts[kShardStatsMaxWorld];
  unsigned long long* g_key;         // table: packed key per slot (kKldEmpty = free)
  int* g_tmin;                       // smallest global first index of the key
  unsigned g_mask;
  int* eslot;                        // [world pad] table slot of a list entry (-1: none)
  int* tile_sums;                    // [tiles] first occurrences per tile, then their exclusive offsets
  int* flags;                        // [2] scan total = distinct keys, [3] a probe bound was hit
  int* keys_out;                     // [3 cap] the distinct keys, unpacked (AoS), in first-index order
  int cap;
};

__device__ __forceinline__ bool gtree_entry(const GlobalTreeArgs& A, int j, unsigned long long* key, int* first)
{
  if (j >= A.world * A.pad)
    return false;
  const int r = j / A.pad, q = j - r * A.pad;
  if (q >= A.counts[r])
    return false;
  *key = (unsigned long long)A.all[((size_t)r * 2) * A.pad + q];
  *first = (int)A.all[((size_t)r * 2 + 1) * A.pad + q];
  return true;
}

__global__ __launch_bounds__(256) void k_gtree_insert(const GlobalTreeArgs A)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.world * A.pad)
    return;
  unsigned long long pk;
  int first;
  int at = -1;
  if (gtree_entry(A, j, &pk, &first))
  {
    unsigned h = gstat_hash(pk, A.g_mask);
    for (unsigned probe = 0; probe <= A.g_mask; ++probe)
    {
      const unsigned long long prev = atomicCAS(&A.g_key[h], kKldEmpty, pk);
      if (prev == kKldEmpty || prev == pk)
      {
        at = (int)h;
        break;
      }
      h = (h + 1) & A.g_mask;
    }
    if (at < 0)
      atomicExch(&A.flags[3], 1);
    else
      atomicMin(&A.g_tmin[at], first);
  }
  A.eslot[j] = at;
}

// is list entry j the first occurrence of its key in the global set?
__device__ __forceinline__ bool gtree_is_first(const GlobalTreeArgs& A, int j)
{
  unsigned long long pk;
  int first;
  if (!gtree_entry(A, j, &pk, &first))
    return false;
  const int at = A.eslot[j];
  return at >= 0 && A.g_tmin[at] == first;
}

// per tile: the number of first occurrences.  A wave counts its 64 entries of a step with one ballot; the block adds
// its four wave counts; the tiles are scanned by k_stats_scan_offsets -- no atomic at all
__global__ __launch_bounds__(256) void k_gtree_first_count(const GlobalTreeArgs A)
{
  __shared__ int s_w[4];
  const int base = blockIdx.x * kStatTile;
  int cnt = 0;  // wave-uniform
  for (int j = threadIdx.x; j < kStatTile; j += 256)
    cnt += __popcll(__ballot(gtree_is_first(A, base + j)));
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
    A.tile_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the first occurrences in list order -> the dense key list (tile_sums holds the exclusive offsets now)
__global__ __launch_bounds__(256) void k_gtree_compact(const GlobalTreeArgs A)
{
  __shared__ int s_w[4];
  constexpr int per = kStatTile / 256;
  const int base = blockIdx.x * kStatTile + threadIdx.x * per;
  int f[per];
  int sum = 0;
#pragma unroll
  for (int j = 0; j < per; ++j)
  {
    f[j] = gtree_is_first(A, base + j) ? 1 : 0;
    sum += f[j];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = sum;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o)
      incl += u;
  }
  if (lane == 63)
    s_w[wave] = incl;
  __syncthreads();
  int run = A.tile_sums[blockIdx.x] + incl - sum;
  for (int q = 0; q < wave; ++q)
    run += s_w[q];
#pragma unroll
  for (int j = 0; j < per; ++j)
    if (f[j])
    {
      if (run >= 0 && run < A.cap)
      {
        const int r = (base + j) / A.pad, q = (base + j) - r * A.pad;
        const unsigned long long pk = (unsigned long long)A.all[((size_t)r * 2) * A.pad + q];
        // kld_pack, undone
        A.keys_out[3 * (size_t)run] = (int)(pk >> 40) - (1 << 23);
        A.keys_out[3 * (size_t)run + 1] = (int)((pk >> 16) & 0xFFFFFFull) - (1 << 23);
        A.keys_out[3 * (size_t)run + 2] = (int)(pk & 0xFFFFull) - (1 << 15);
      }
      run += 1;
    }
}

}  // namespace bpf
