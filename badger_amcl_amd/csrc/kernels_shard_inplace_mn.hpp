// Multinomial resampling of a SHARDED set in place: every rank resamples its own slice into its own slice, and the KLD
// stop index comes from the ranks' bin lists instead of a replay of every key.
//
// Draw m reads fixed elements of the drand48 stream (2 m + 2, or the recovery chain's), so a rank can evaluate every
// candidate draw 0 .. max_samples - 1 and keep those whose uniform falls into its slice of the global CDF
// (draw_window_column's ownership test as it is; the random poses of w_diff > 0 belong to rank 0).  The histogram tree
// is a function of the distinct keys in first-occurrence order, so the leaf count after every draw follows from the
// (key, first draw index) pairs of all ranks, merged:
//
//   k_mn_select_count     per tile of 256 candidates: how many this rank owns
//   k_stats_scan_offsets  (kernels_stats.hpp) exclusive scan of the tile counts; the total is the kept count
//   k_mn_select_scatter   the owned candidates, in draw order, into the set that is NOT current: pose bits and the draw
//                         index of every kept sample (a wave ballots "owned" and ranks its lanes by popcount)
//   -- the kept samples' bin list: k_set_keys / k_kld_hash / k_sstat_first_count / k_sstat_compact as they are --
//   k_mn_remap_bins       a bin's first LOCAL index -> that sample's draw index (local order is draw order, so the
//                         first local occurrence carries the smallest draw index)
//   -- exchange: the ranks' (bin count, flag) words, then the lists --
//   k_gtree_insert        (kernels_shard_init.hpp) one table in which a key keeps its smallest first draw index
//   k_mn_mark             mark[t] = list entry whose key first occurs at draw t
//   k_mn_mark_count / k_stats_scan_offsets / k_mn_mark_compact
//                         the distinct keys in first-draw order with t_j beside them (the ranks' draws interleave, so
//                         rank-then-list order is NOT draw order: the marks are a counting sort by draw index)
//   -- the tree on those keys: the device tree (whole stream, leaf count after every key) or the host tree --
//   k_mn_stop / k_mn_stop_result
//                         c_j = max(t_j + 1, limit(L_j) + 1); the stop is the smallest c_j <= t_{j+1} (t_B = max)
//   k_mn_owner_hist       every rank's count of the new set: the owner of draws 0 .. M - 1 (an LDS histogram per block)
//   k_mn_owner_check      the rank's kept draws below M are exactly its count (the truncation moves no data)
//   k_mn_fill_weight      weights 1 / M
//
// No kernel here waits for another rank or for another block.
#pragma once
#include <climits>
#include "kernels_pf.hpp"
#include "kernels_shard_init.hpp"

namespace bpf
{

constexpr int kMnTile = 256;  // candidates per block of the select: one per thread

struct MnSelectArgs
{
  // src, n_src, cdf, coarse, rank, world, rng_state, jump, jump_table, chain, write_random, free_space as for
  // k_draw_window; m0 = 0, m1 = max_samples; targets = nullptr; flags = one scratch word (see mn_candidate)
  WindowArgs W;
  double offset, top;  // this shard's slice of the global CDF (shard_slice's values, formed by the host)
  ParticlesDev dst;
  int* draw_idx;       // [max] draw index of every kept sample, ascending
  int* tile_sums;      // [tiles] kept per tile, then their exclusive offsets
  int* first_miss;     // smallest draw index that did (INT_MAX on entry)
};

// dynamic LDS: the CDF subsample when W.coarse is given, as in k_draw_window
__device__ __forceinline__ const double* mn_stage_coarse(const WindowArgs& W, unsigned char* smem)
{
  if (W.coarse == nullptr)
    return nullptr;
  double* s_coarse = reinterpret_cast<double*>(smem);
  const int n_coarse = ((W.n_src - 1) >> W.coarse_shift) + 1;
  for (int k = threadIdx.x; k <= n_coarse; k += blockDim.x)
    s_coarse[k] = W.coarse[k];
  __syncthreads();
  return s_coarse;
}

// the uniform of draw m as draw_window_column forms it (targets == nullptr); *random: a free-space pose instead
__device__ __forceinline__ double mn_draw_uniform(const WindowArgs& A, int m, bool* random)
{
  *random = false;
  if (A.chain != nullptr)
  {
    const int c = A.chain[m];
    if (c < 0)
    {
      *random = true;
      return 0.0;
    }
    return ldexp((double)lcg_skip(A.rng_state, (uint64_t)(c & 0x7fffffff), A.jump), -48);
  }
  if (A.jump_table != nullptr && m < A.jump_table_n)
  {
    const FusedJump J = A.jump_table[m];
    return ldexp((double)((J.a * A.rng_state + J.c) & ((1ull << 48) - 1)), -48);
  }
  return ldexp((double)lcg_skip(A.rng_state, 2ull * (uint64_t)m + 2ull, A.jump), -48);
}

// Candidate o of this rank: true when it is kept.  A candidate whose search fails on this rank (a uniform that rounding
// sends to a shard without particles, or past the last shard's slice) is kept too, as the column the window form would
// have summed, so that the ranks' counts tile the set.  *missed: draw_window_column raised the flag for this candidate
// (its two conditions, restated on the same uniform; W.flags itself is one scratch word nobody reads).
__device__ __forceinline__ bool mn_candidate(const MnSelectArgs& A, int o, long long out[6], const double* s_coarse,
                                             bool* missed)
{
  const bool owned = draw_window_column(A.W, o, out, A.offset, A.top, s_coarse);
  bool random;
  const double r = mn_draw_uniform(A.W, o, &random);
  const bool last = A.W.rank == A.W.world - 1;
  const bool mine = !random && (r >= A.offset) && (r < A.top || last);
  *missed = mine && (A.W.n_src <= 0 || !(r < A.top));
  return owned || *missed;
}

__global__ __launch_bounds__(kMnTile) void k_mn_select_count(const MnSelectArgs A)
{
  extern __shared__ __align__(16) unsigned char mn_smem[];
  __shared__ int s_w[kMnTile / 64];
  const double* s_coarse = mn_stage_coarse(A.W, mn_smem);
  const int o = blockIdx.x * kMnTile + threadIdx.x;
  long long out[6];
  bool missed = false;
  const bool kept = o < A.W.m1 && mn_candidate(A, o, out, s_coarse, &missed);
  const int cnt = __popcll(__ballot(kept));
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int sum = 0;
    for (int w = 0; w < kMnTile / 64; ++w)
      sum += s_w[w];
    A.tile_sums[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(kMnTile) void k_mn_select_scatter(const MnSelectArgs A)
{
  extern __shared__ __align__(16) unsigned char mn_smem[];
  __shared__ int s_w[kMnTile / 64];
  const double* s_coarse = mn_stage_coarse(A.W, mn_smem);
  const int o = blockIdx.x * kMnTile + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long out[6] = { 0, 0, 0, 0, 0, 0 };
  bool missed = false;
  const bool kept = o < A.W.m1 && mn_candidate(A, o, out, s_coarse, &missed);
  const unsigned long long ballot = __ballot(kept);
  if (lane == 0)
    s_w[wave] = __popcll(ballot);
  __syncthreads();
  if (!kept)
    return;
  int pos = A.tile_sums[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w)
    pos += s_w[w];
  if (pos < 0 || pos >= A.W.m1)
    return;  // (cannot happen: the offsets are the scan of the same counts)
  A.dst.x[pos] = __longlong_as_double(out[0]);
  A.dst.y[pos] = __longlong_as_double(out[1]);
  A.dst.th[pos] = __longlong_as_double(out[2]);
  A.draw_idx[pos] = o;
  if (missed)
    atomicMin(A.first_miss, o);
}

// bins = int64[2][n_bins] (k_sstat_compact, global_first = 0): row 1, the first local index, becomes the draw index
__global__ void k_mn_remap_bins(long long* __restrict__ first, int n_bins, const int* __restrict__ draw_idx, int n_kept)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_bins)
    return;
  const long long i = first[b];
  first[b] = (i >= 0 && i < n_kept) ? (long long)draw_idx[i] : -1ll;
}

// mark[t] = 1 + the list entry that is its key's first occurrence, at its draw index t (zero on entry; draw indices of
// first occurrences are distinct: one draw, one key)
__global__ __launch_bounds__(256) void k_mn_mark(const GlobalTreeArgs A, int* __restrict__ mark, int n_draws)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long pk;
  int first;
  if (!gtree_entry(A, j, &pk, &first) || !gtree_is_first(A, j))
    return;
  if (first < 0 || first >= n_draws)
  {
    atomicExch(&A.flags[3], 1);  // a draw index outside the stream: a corrupt list
    return;
  }
  mark[first] = j + 1;
}

__global__ __launch_bounds__(kMnTile) void k_mn_mark_count(const int* __restrict__ mark, int n_draws,
                                                          int* __restrict__ tile_sums)
{
  __shared__ int s_w[kMnTile / 64];
  const int t = blockIdx.x * kMnTile + threadIdx.x;
  const int cnt = __popcll(__ballot(t < n_draws && mark[t] != 0));
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int sum = 0;
    for (int w = 0; w < kMnTile / 64; ++w)
      sum += s_w[w];
    tile_sums[blockIdx.x] = sum;
  }
}

// the distinct keys in first-draw order: A.keys_out (unpacked, AoS) and t_out, both [A.cap]
__global__ __launch_bounds__(kMnTile) void k_mn_mark_compact(const GlobalTreeArgs A, const int* __restrict__ mark,
                                                            int n_draws, const int* __restrict__ tile_offsets,
                                                            int* __restrict__ t_out)
{
  __shared__ int s_w[kMnTile / 64];
  const int t = blockIdx.x * kMnTile + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mk = t < n_draws ? mark[t] : 0;
  const unsigned long long ballot = __ballot(mk != 0);
  if (lane == 0)
    s_w[wave] = __popcll(ballot);
  __syncthreads();
  if (mk == 0)
    return;
  int pos = tile_offsets[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w)
    pos += s_w[w];
  if (pos < 0 || pos >= A.cap)
    return;
  const int j = mk - 1;
  const int r = j / A.pad, q = j - r * A.pad;
  const unsigned long long pk = (unsigned long long)A.all[((size_t)r * 2) * A.pad + q];
  // kld_pack, undone
  A.keys_out[3 * (size_t)pos] = (int)(pk >> 40) - (1 << 23);
  A.keys_out[3 * (size_t)pos + 1] = (int)((pk >> 16) & 0xFFFFFFull) - (1 << 23);
  A.keys_out[3 * (size_t)pos + 2] = (int)(pk & 0xFFFFull) - (1 << 15);
  t_out[pos] = t;
}

// One thread per distinct key j: the stop count its stretch of the stream [t_j + 1, t_{j+1}] would give.  The stretches
// are disjoint and ascend with j, so the smallest c_j that fits its stretch belongs to the smallest such j.
// counts: the device tree's (leaf, bin) counts after every key, or nullptr: L_j = j + 1 (BPF_KLD_COUNT_BINS).
__global__ __launch_bounds__(256) void k_mn_stop(const int* __restrict__ t, int n_bins, const int2* __restrict__ counts,
                                                 const int* __restrict__ limit, int max_samples, int* stop_j)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_bins)
    return;
  const int L = counts != nullptr ? counts[j].x : j + 1;
  const int c = max(t[j] + 1, limit[L] + 1);
  const int t_next = j + 1 < n_bins ? t[j + 1] : max_samples;
  if (c <= t_next)
    atomicMin(stop_j, j);
}

// res[0] = M, res[1] = leaf count, res[2] = distinct keys of the new set
__global__ void k_mn_stop_result(const int* __restrict__ t, int n_bins, const int2* __restrict__ counts,
                                 const int* __restrict__ limit, int max_samples, const int* __restrict__ stop_j,
                                 int* __restrict__ res)
{
  if (blockIdx.x != 0 || threadIdx.x != 0)
    return;
  const bool stopped = *stop_j < n_bins;
  const int j = stopped ? *stop_j : n_bins - 1;
  const int L = counts != nullptr ? counts[j].x : j + 1;
  res[0] = stopped ? max(t[j] + 1, limit[L] + 1) : max_samples;
  res[1] = L;
  res[2] = j + 1;
}

struct MnOwnerArgs
{
  WindowArgs W;                       // rng_state, jump, jump_table, chain as for the select
  double edge[kMailboxMaxWorld + 1];  // shard q owns [edge[q], edge[q + 1]) of the global CDF
  int world;
  int M;
  int* counts;                        // [world] zero on entry
};

// The owner of uniform r is the last q with edge[q] <= r (the slices tile [0, 1): every rank forms the same running
// sum; what lies past the last edge is the last rank's, as in the ownership test).  Random poses are rank 0's.
__global__ __launch_bounds__(256) void k_mn_owner_hist(const MnOwnerArgs A)
{
  __shared__ int s_cnt[kMailboxMaxWorld];
  if (threadIdx.x < kMailboxMaxWorld)
    s_cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int m = blockIdx.x * 256 + threadIdx.x; m < A.M; m += gridDim.x * 256)
  {
    bool random;
    const double r = mn_draw_uniform(A.W, m, &random);
    int q = 0;
    if (!random)
      for (int k = 1; k < A.world; ++k)
        if (A.edge[k] <= r)
          q = k;
    atomicAdd(&s_cnt[q], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < A.world && s_cnt[threadIdx.x] != 0)
    atomicAdd(&A.counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// ok[0] = 1 when the kept draws below M are exactly the first n_new (draw_idx ascends)
__global__ void k_mn_owner_check(const int* __restrict__ draw_idx, int n_kept, const int* __restrict__ counts, int rank,
                                 int M, int* __restrict__ ok)
{
  if (blockIdx.x != 0 || threadIdx.x != 0)
    return;
  const int n_new = counts[rank];
  bool good = n_new >= 0 && n_new <= n_kept;
  if (good && n_new > 0)
    good = draw_idx[n_new - 1] < M;
  if (good && n_new < n_kept)
    good = draw_idx[n_new] >= M;
  ok[0] = good ? 1 : 0;
}

__global__ void k_mn_fill_weight(double* __restrict__ w, int n, double weight)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    w[i] = weight;
}

}  // namespace bpf
