// Exhaustive pose search (bpf_planar_search_poses, abi_pose_search.inl; bpf_cloud_search_poses,
// abi_pose_search_cloud.inl): every free cell of the 2-D map -- or every column of the 3-D map's rectangle -- at every
// one of H headings, scored against one scan by the planar scoring path (one cloud by the 3-D one), the best K kept.
// Four kernels of its own:
//
//   k_search_candidates   one window of candidate poses into the engine's candidate set (one lane per candidate)
//   k_search_select       a block sorts its tile of the window's scores in LDS (bitonic network) and emits its best
//                         min(K, tile); candidates strictly below the K-th best score so far are dropped before the
//                         sort (ballot + compaction), so that after the first windows most blocks sort nothing
//   k_search_merge        ONE block folds the tiles' lists into the running best-K list (bitonic merge of two sorted
//                         halves in LDS, one round per tile that kept something)
//   k_search_hits         the final list as bpf_pose_hit rows
// and two for the sharded search (abi_shard_search.inl): k_search_pack_list, k_search_merge_lists
//
// Order: score descending, equal scores by candidate ascending, NaN below every number.  An entry is 16 bytes: `key`,
// the score's bits mapped so that unsigned order is numeric order (NaN -> 0, -0.0 -> +0.0; a non-negative double
// orders as its own bit pattern), and `inv` = ~candidate, so that "better" is the lexicographically LARGER (key, inv).
// The empty entry (0, 0) is worse than every real one (candidate < 2^31, so inv != 0).  Candidates are distinct, so
// the order is total and the result does not depend on how the compaction placed its survivors.  No atomics on
// doubles, no block that waits for another: the launches' order on the stream is the only synchronisation.
#pragma once
#include "device_types.hpp"

namespace bpf
{

constexpr int kSearchMaxK = 1024;     // API limit of k
constexpr int kSearchTile = 2048;     // candidates per block of k_search_select
constexpr int kSearchThreads = 1024;  // of both kernels

struct SearchEntry
{
  unsigned long long key, inv;
};

// geometry of the candidate enumeration.  Planar search: the strided free list F_s.  Cloud search (cells == nullptr):
// the columns of Node3D::updateFreeSpaceIndices kept by the stride, as rectangle arithmetic the way FreeSpaceDev
// carries its 3-D form -- column f is (i0 + (f / n_j) * stride, j0 + (f % n_j) * stride), n_cells = n_i * n_j
struct SearchSpace
{
  const int2* cells;  // F_s
  int n_cells;
  int headings;
  int size_x, size_y;
  double origin_x, origin_y, resolution;
  int i0, j0, n_j, stride;  // rectangle form
};

__host__ __device__ __forceinline__ unsigned long long search_key_of(double score)
{
  if (score != score)
    return 0ull;
  union
  {
    double d;
    unsigned long long u;
  } v;
  v.d = score + 0.0;  // -0.0 -> +0.0
  return (v.u >> 63) ? ~v.u : (v.u | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ double search_score_of(unsigned long long key)
{
  union
  {
    double d;
    unsigned long long u;
  } v;
  if (key == 0ull)
    v.u = 0x7ff8000000000000ull;
  else
    v.u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return v.d;
}

__device__ __forceinline__ bool search_better(const SearchEntry& a, const SearchEntry& b)
{
  return a.key > b.key || (a.key == b.key && a.inv > b.inv);
}

// the pose of candidate c: the cell expression of random_free_space_pose (2-D: integer halves; 3-D: i * res, j * res
// of OctoMap::convertMapToWorld; no contraction), the heading evaluated in double as written.  The branch on the form
// is uniform over the launch.
__device__ __forceinline__ void search_pose_of(const SearchSpace& S, long long c, int* i, int* j, int* h, double* x,
                                               double* y, double* th)
{
#pragma clang fp contract(off)
  // c < 2^31 (checked before any launch): one 32-bit division
  const unsigned cu = (unsigned)c, H = (unsigned)S.headings;
  const unsigned f = cu / H;
  const unsigned hh = cu - f * H;
  *h = (int)hh;
  if (S.cells != nullptr)
  {
    const int2 cell = S.cells[f];
    *i = cell.x;
    *j = cell.y;
    *x = S.origin_x + (cell.x - S.size_x / 2) * S.resolution;
    *y = S.origin_y + (cell.y - S.size_y / 2) * S.resolution;
  }
  else
  {
    const unsigned fi = f / (unsigned)S.n_j;
    const int ci = S.i0 + (int)fi * S.stride, cj = S.j0 + (int)(f - fi * (unsigned)S.n_j) * S.stride;
    *i = ci;
    *j = cj;
    *x = ci * S.resolution;
    *y = cj * S.resolution;
  }
  *th = (2.0 * 3.14159265358979323846 * (double)hh) / (double)S.headings - 3.14159265358979323846;
}

// candidates c0 .. c0 + n - 1 into dst[0 .. n)
__global__ void k_search_candidates(ParticlesDev dst, int n, long long c0, SearchSpace S)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  int i, j, h;
  double x, y, th;
  search_pose_of(S, c0 + (long long)t, &i, &j, &h, &x, &y, &th);
  dst.x[t] = x;
  dst.y[t] = y;
  dst.th[t] = th;
  dst.w[t] = 1.0;
}

// bitonic sort of s[0 .. P), P a power of two >= 2, best first
__device__ __forceinline__ void search_sort_lds(SearchEntry* s, int P)
{
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
    {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x)
      {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i + j;
        const bool best_first = (i & k) == 0;
        const SearchEntry a = s[i], b = s[l];
        if (search_better(b, a) == best_first)
        {
          s[i] = b;
          s[l] = a;
        }
      }
      __syncthreads();
    }
}

// Block b takes scores[b * kSearchTile ...) of the window's n (candidates c0 + index).  best / best_count: the running
// list of the windows before this one (sorted, best first); with K entries in it, a candidate strictly below the
// K-th is dropped.  Output: tile_out[b * K ...) = the tile's best min(K, kept), best first; tile_count[b] = how many.
// The body serves two kernels: the candidate of slot idx is c0 + idx (IDS false: k_search_select) or ids[idx], a
// negative id marking an empty slot (IDS true: k_prune_select, kernels_pose_search_pruned.hpp).
template <bool IDS>
__device__ __forceinline__ void search_select_tile(const double* __restrict__ scores, int n, long long c0,
                                                   const long long* __restrict__ ids, int K,
                                                   const SearchEntry* __restrict__ best,
                                                   const int* __restrict__ best_count,
                                                   SearchEntry* __restrict__ tile_out, int* __restrict__ tile_count)
{
  __shared__ SearchEntry s[kSearchTile];
  __shared__ int kept;
  const int tid = threadIdx.x;
  if (tid == 0)
    kept = 0;
  __syncthreads();
  const unsigned long long floor_key = *best_count >= K ? best[K - 1].key : 0ull;
  const int base = blockIdx.x * kSearchTile;
  const int lane = tid & 63;
#pragma unroll
  for (int r = 0; r < kSearchTile / kSearchThreads; ++r)
  {
    const int idx = base + r * kSearchThreads + tid;
    SearchEntry en{ 0ull, 0ull };
    bool keep = false;
    if (idx < n)
    {
      const long long c = IDS ? ids[idx] : c0 + (long long)idx;
      if (!IDS || c >= 0)
      {
        en.key = search_key_of(scores[idx]);
        en.inv = ~(unsigned long long)c;
        keep = en.key >= floor_key;
      }
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    int at = 0;
    if (lane == 0 && mask != 0ull)
      at = atomicAdd(&kept, __popcll(mask));
    at = __builtin_amdgcn_readfirstlane(at);
    if (keep)
      s[at + __popcll(mask & ((1ull << lane) - 1ull))] = en;
  }
  __syncthreads();
  const int m = kept;
  if (m == 0)
  {
    if (tid == 0)
      tile_count[blockIdx.x] = 0;
    return;
  }
  int P = 2;
  while (P < m)
    P <<= 1;
  for (int t = m + tid; t < P; t += kSearchThreads)
    s[t] = SearchEntry{ 0ull, 0ull };
  __syncthreads();
  search_sort_lds(s, P);
  const int out_n = m < K ? m : K;
  for (int t = tid; t < out_n; t += kSearchThreads)
    tile_out[(size_t)blockIdx.x * K + t] = s[t];
  if (tid == 0)
    tile_count[blockIdx.x] = out_n;
}

__global__ __launch_bounds__(kSearchThreads) void k_search_select(const double* __restrict__ scores, int n,
                                                                  long long c0, int K,
                                                                  const SearchEntry* __restrict__ best,
                                                                  const int* __restrict__ best_count,
                                                                  SearchEntry* __restrict__ tile_out,
                                                                  int* __restrict__ tile_count)
{
  search_select_tile<false>(scores, n, c0, nullptr, K, best, best_count, tile_out, tile_count);
}

// One block: best[0 .. *best_count) (sorted) and every tile's sorted list -> the best K of them all, sorted, back in
// `best`.  Kp = the power of two >= max(K, 2): the list sits in s[0 .. Kp), a tile's list reversed in s[Kp .. 2 Kp),
// empties between them -- a bitonic sequence, which log2(2 Kp) compare-exchange stages sort.
// The body serves two kernels: list b starts at lists[b * list_stride] and holds counts[b * count_stride] entries --
// the tiles of a window (k_search_merge: stride K, int counts) or the ranks' gathered lists (k_search_merge_lists).
template <typename CountT>
__device__ __forceinline__ void search_merge_body(SearchEntry* __restrict__ best, int* __restrict__ best_count, int K,
                                                  int Kp, const SearchEntry* __restrict__ lists, size_t list_stride,
                                                  const CountT* __restrict__ counts, size_t count_stride, int n_lists)
{
  __shared__ SearchEntry s[2 * kSearchMaxK];
  const int tid = threadIdx.x;
  const int have = *best_count;
  for (int t = tid; t < Kp; t += kSearchThreads)
    s[t] = t < have ? best[t] : SearchEntry{ 0ull, 0ull };
  int total = have;
  for (int b = 0; b < n_lists; ++b)
  {
    const int cnt = (int)counts[(size_t)b * count_stride];  // (the same for every thread: the loop stays uniform)
    if (cnt == 0)
      continue;
    total += cnt;
    for (int t = tid; t < Kp; t += kSearchThreads)
    {
      const int src = Kp - 1 - t;
      s[Kp + t] = src < cnt ? lists[(size_t)b * list_stride + src] : SearchEntry{ 0ull, 0ull };
    }
    __syncthreads();
    for (int j = Kp; j > 0; j >>= 1)
    {
      for (int t = tid; t < Kp; t += kSearchThreads)
      {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i + j;
        const SearchEntry a = s[i], c = s[l];
        if (search_better(c, a))
        {
          s[i] = c;
          s[l] = a;
        }
      }
      __syncthreads();
    }
  }
  const int keep = total < K ? total : K;
  for (int t = tid; t < keep; t += kSearchThreads)
    best[t] = s[t];
  if (tid == 0)
    *best_count = keep;
}

__global__ __launch_bounds__(kSearchThreads) void k_search_merge(SearchEntry* __restrict__ best,
                                                                 int* __restrict__ best_count, int K, int Kp,
                                                                 const SearchEntry* __restrict__ tile_out,
                                                                 const int* __restrict__ tile_count, int n_tiles)
{
  search_merge_body<int>(best, best_count, K, Kp, tile_out, (size_t)K, tile_count, 1, n_tiles);
}

// ---- the ranks' lists of a sharded search (abi_shard_search.inl).  A rank's list travels as K + 1 entries of two
// int64 words each: a header (count, 0), then K rows, the ones behind the count empty.
// this rank's list in that form
__global__ __launch_bounds__(kSearchThreads) void k_search_pack_list(const SearchEntry* __restrict__ best,
                                                                     const int* __restrict__ best_count, int K,
                                                                     SearchEntry* __restrict__ out)
{
  const int have = min(*best_count, K);
  for (int t = threadIdx.x; t < K; t += kSearchThreads)
    out[1 + t] = t < have ? best[t] : SearchEntry{ 0ull, 0ull };
  if (threadIdx.x == 0)
    out[0] = SearchEntry{ (unsigned long long)have, 0ull };
}

// ONE block: the W gathered lists (rank r's header at gathered[r * (K + 1)]) folded into the best K of them all, in
// `best` / `best_count` (which the caller emptied)
__global__ __launch_bounds__(kSearchThreads) void k_search_merge_lists(SearchEntry* __restrict__ best,
                                                                       int* __restrict__ best_count, int K, int Kp,
                                                                       const SearchEntry* __restrict__ gathered,
                                                                       int n_lists)
{
  search_merge_body<unsigned long long>(best, best_count, K, Kp, gathered + 1, (size_t)K + 1, &gathered[0].key,
                                        2 * ((size_t)K + 1), n_lists);
}

// the list as rows for the caller
__global__ void k_search_hits(const SearchEntry* __restrict__ best, const int* __restrict__ best_count, SearchSpace S,
                              bpf_pose_hit* __restrict__ out)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= *best_count)
    return;
  const SearchEntry en = best[t];
  bpf_pose_hit hit;
  hit.candidate = (long long)~en.inv;
  hit.score = search_score_of(en.key);
  search_pose_of(S, hit.candidate, &hit.i, &hit.j, &hit.heading, &hit.pose[0], &hit.pose[1], &hit.pose[2]);
  hit.reserved = 0;
  out[t] = hit;
}

}  // namespace bpf
