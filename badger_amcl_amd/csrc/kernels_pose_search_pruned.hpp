// Pruned pose search (bpf_planar_search_poses_pruned, abi_pose_search_pruned.inl): the rows of the exhaustive search,
// bit for bit, from fewer exact evaluations.  The candidates of one B x B block of cells at one heading ("block
// candidate" q = block * H + h) share an upper bound: the block's anchor pose scored by the unchanged scoring path
// against P_B, a min-pooled copy of the LUT image ("Pose search, pruned form").  A block
// candidate whose bound is strictly below the K-th best exact score so far holds no hit and is never expanded.
//
//   k_pool_rows / k_pool_cols   P_B from lut_tiles: a separable sliding minimum over the u16 level codes, a row's /
//                               a tile's window staged in LDS; the second pass writes the 8x8-tiled layout itself
//   k_prune_anchors             one window of anchor poses into the engine's candidate set
//   k_prune_bounds              the window's weights -> bounds (the factor ceiling, the Gompertz margin)
//   k_prune_seed_plan           ONE block: the best-bound block candidates as the seed, their member offsets
//   k_prune_expand_seed         one window of the seed's members as exact candidates, with their ids
//   k_prune_select              k_search_select keyed by an id array (id < 0: an empty slot of the window)
//   k_prune_survivors           block candidates outside the seed whose bound is not below tau, compacted per chunk of
//                               1024 in index order; the host sums the chunk totals (the call's one intermediate wait)
//   k_prune_expand              one window of the survivors' members; every block candidate is checked once more
//                               against the tau of that moment and dropped whole if its bound is below it
//   k_prune_floor_word / k_prune_floor   a sharded search only: the ranks' K-th keys behind the seed, their maximum as
//                               a floor under tau for the two kernels above
//
// tau lives in device memory (the K-th row of the running exact list) and only changes between kernels of the one
// stream.  No block waits for another.  A dropped or empty slot of a window carries a NaN pose, which the scoring path
// sends off the map without a gather that misses (field_prep_of), and id -1, which the selection skips.
//
// The 3-D cloud search (bpf_cloud_search_poses_pruned, kernels_pose_search_cloud_pruned.hpp) runs the same kernels over
// the rectangle form of SearchSpace and PruneBlocks: anchors and members by arithmetic instead of from lists.
#pragma once
#include "kernels_pose_search.hpp"
#include "kernels_score.hpp"

namespace bpf
{

constexpr int kPruneMaxBlock = 64;                         // the largest B
constexpr int kPruneChunk = 1024;                          // block candidates per block of k_prune_survivors
constexpr int kPruneSeed = kSearchMaxK;                    // block candidates of the seed: what the bound list holds
constexpr long long kPruneMaxBlockCandidates = 1ll << 24;  // capacity limit of one call
constexpr int kPruneWords = 8;  // counters of a call: [0] seed rows [1] seed members [2] dropped at expansion
                                // [3] expanded [4] members of the expanded

// the block list of one (map, radius, stride, B) in CSR over F_s and the range of it a call works on
struct PruneBlocks
{
  const int* start;     // [n_blocks + 1] into member
  const int* member;    // [|F_s|] indices f into F_s, ascending inside a block
  const int2* anchor;   // [n_blocks] the cell (bi * B, bj * B)
  int first_block;      // block candidate q of the call is block first_block + q / H at heading q % H
  int headings;
  // rectangle form (member == nullptr: the 3-D cloud search, kernels_pose_search_cloud_pruned.hpp).  The block list is
  // the product of two per-axis lists, block b = ib * nbj + jb; a block's members are the columns a in [axis_i[ib],
  // axis_i[ib + 1]) x b in [axis_j[jb], axis_j[jb + 1]) of the rectangle C_s, f = a * n_j + b, a outer (f ascending)
  const int* axis_i;    // [nbi + 1]
  const int* axis_j;    // [nbj + 1]
  int nbj, n_j;
};

// what a bound is made of behind the scoring launch
struct PruneBoundForm
{
  double f_max, f_min;  // ceiling / floor of recalc_factor: max / min of (1, off_map_factor, non_free_factor)
  double margin_abs;    // Gompertz: the bound goes up by margin_abs + margin_rel * |p| (0 for the likelihood field)
  double margin_rel;
};

// ------------------------------------------------------------------ the pooled image
// Pass 1, one row v of the padded image per blockIdx.y: R(u, v) = min of the codes at padded u' in [u - 1, u + B];
// the far border u = size_x + 1, where clamp_cell also sends every negative coordinate, takes the cells within B + 1
// of either edge.  Coordinates outside the padded image hold the off-map code, the largest there is.
__global__ __launch_bounds__(256) void k_pool_rows(MapDev M, int B, unsigned koff, uint16_t* __restrict__ R)
{
  __shared__ uint16_t s[256 + kPruneMaxBlock + 2];
  const int Wp = M.size_x + 2;
  const int v = blockIdx.y, u0 = blockIdx.x * 256;
  const int span = 256 + B + 2;  // padded u0 - 1 .. u0 + 256 + B
  for (int t = threadIdx.x; t < span; t += 256)
  {
    const int uu = u0 - 1 + t;
    s[t] = (uu >= 0 && uu < Wp) ? (uint16_t)lut_level8(M, (unsigned)uu, (unsigned)v) : (uint16_t)koff;
  }
  __syncthreads();
  const int u = u0 + (int)threadIdx.x;
  if (u >= Wp)
    return;
  unsigned m = koff;
  if (u < Wp - 1)
  {
    for (int d = 0; d < B + 2; ++d)
      m = min(m, (unsigned)s[threadIdx.x + d]);
  }
  else
  {
    for (int uu = 0; uu <= min(B + 1, Wp - 1); ++uu)
      m = min(m, lut_level8(M, (unsigned)uu, (unsigned)v));
    for (int uu = max(0, M.size_x - B); uu < Wp; ++uu)
      m = min(m, lut_level8(M, (unsigned)uu, (unsigned)v));
  }
  R[(size_t)v * Wp + u] = (uint16_t)m;
}

// Pass 2, a 64 x 64 piece of the tiled image per block: P(u, v) = min of R(u, v') over the same window in v, written
// at the entry's place in the 8x8-tiled layout; what the layout holds beyond the padded image is the off-map code.
__global__ __launch_bounds__(256) void k_pool_cols(MapDev M, int B, unsigned koff, const uint16_t* __restrict__ R,
                                                   uint16_t* __restrict__ P)
{
  __shared__ uint16_t s[(64 + kPruneMaxBlock + 2) * 64];
  const int Wp = M.size_x + 2, Hp = M.size_y + 2;
  const int Wt = M.ltx * 8, Ht = M.lty * 8;
  const int u0 = blockIdx.x * 64, v0 = blockIdx.y * 64;
  const int rows = 64 + B + 2;  // padded v0 - 1 .. v0 + 64 + B
  for (int t = threadIdx.x; t < rows * 64; t += 256)
  {
    const int vv = v0 - 1 + (t >> 6), uu = u0 + (t & 63);
    s[t] = (vv >= 0 && vv < Hp && uu < Wp) ? R[(size_t)vv * Wp + uu] : (uint16_t)koff;
  }
  __syncthreads();
  const int cu = threadIdx.x & 63, u = u0 + cu;
  for (int rr = threadIdx.x >> 6; rr < 64; rr += 4)
  {
    const int v = v0 + rr;
    if (u >= Wt || v >= Ht)
      continue;
    unsigned m = koff;
    if (u < Wp && v < Hp - 1)
    {
      for (int d = 0; d < B + 2; ++d)
        m = min(m, (unsigned)s[(rr + d) * 64 + cu]);
    }
    else if (u < Wp && v == Hp - 1)
    {
      for (int vv = 0; vv <= min(B + 1, Hp - 1); ++vv)
        m = min(m, (unsigned)R[(size_t)vv * Wp + u]);
      for (int vv = max(0, M.size_y - B); vv < Hp; ++vv)
        m = min(m, (unsigned)R[(size_t)vv * Wp + u]);
    }
    P[((size_t)(v >> 3) * M.ltx + (u >> 3)) * 64 + ((u & 7) << 3) + (v & 7)] = (uint16_t)m;
  }
}

// ------------------------------------------------------------------ bounds
// anchor poses of the global block candidates q0 .. q0 + n - 1 (q = block * H + h over the whole block list): the
// cell expression (of either form of the space) and the heading expression of search_pose_of
__global__ void k_prune_anchors(ParticlesDev dst, int n, long long q0, const int2* __restrict__ anchor, SearchSpace S)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  const unsigned q = (unsigned)(q0 + (long long)t), H = (unsigned)S.headings;
  const unsigned b = q / H, hh = q - b * H;
  const int2 cell = anchor[b];
  if (S.cells != nullptr)
  {
    dst.x[t] = S.origin_x + (cell.x - S.size_x / 2) * S.resolution;
    dst.y[t] = S.origin_y + (cell.y - S.size_y / 2) * S.resolution;
  }
  else  // the rectangle form's cell expression (3-D: i * res, j * res)
  {
    dst.x[t] = cell.x * S.resolution;
    dst.y[t] = cell.y * S.resolution;
  }
  dst.th[t] = (2.0 * 3.14159265358979323846 * (double)hh) / (double)S.headings - 3.14159265358979323846;
  dst.w[t] = 1.0;
}

// the anchors' weights, scored with neutral map factors, as bounds: the margin, then the factor's ceiling (its floor
// under a negative value, which only a Gompertz output shift can give).  A NaN stays a NaN.
__global__ void k_prune_bounds(const double* __restrict__ w, int n, double* __restrict__ bounds, PruneBoundForm F)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  double p = w[t];
  p = p + (F.margin_abs + F.margin_rel * fabs(p));
  bounds[t] = p >= 0.0 ? p * F.f_max : p * F.f_min;
}

// exclusive prefix of v over the 1024 threads of the block in thread order, *total = the sum; s_w: 16 ints of LDS
__device__ __forceinline__ int prune_block_scan(int v, int* s_w, int* total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
  {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off)
      inc += o;
  }
  if (lane == 63)
    s_w[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < 16; ++k)
  {
    const int x = s_w[k];
    if (k < wave)
      before += x;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

__device__ __forceinline__ int prune_members_of(const PruneBlocks& L, int q)
{
  const int b = L.first_block + q / L.headings;
  return L.start[b + 1] - L.start[b];
}

// ONE block of 1024: row r of the bound list (`best`, ids = block candidates of the call) becomes seed r.
// seed_off[r] = members of the seeds before r, seed_off[n_seed] = all of them; in_seed[q] = 1; words[0 .. 1].
__global__ __launch_bounds__(1024) void k_prune_seed_plan(const SearchEntry* __restrict__ best,
                                                          const int* __restrict__ best_count, PruneBlocks L,
                                                          int* __restrict__ seed_q, int* __restrict__ seed_off,
                                                          uint8_t* __restrict__ in_seed,
                                                          unsigned long long* __restrict__ words)
{
  __shared__ int s_w[16];
  const int r = threadIdx.x, n_seed = min(*best_count, 1024);
  int q = 0, cnt = 0;
  if (r < n_seed)
  {
    q = (int)~best[r].inv;
    cnt = prune_members_of(L, q);
    seed_q[r] = q;
    in_seed[q] = 1;
  }
  int total;
  const int off = prune_block_scan(cnt, s_w, &total);
  if (r < n_seed)
    seed_off[r] = off;
  if (r == 0)
  {
    seed_off[n_seed] = total;
    words[0] = (unsigned long long)n_seed;
    words[1] = (unsigned long long)total;
  }
}

// slot t of a window as an exact candidate (c >= 0: member r of block candidate q) or as an empty slot
__device__ __forceinline__ void prune_write_slot(ParticlesDev dst, long long* ids, int t, const PruneBlocks& L,
                                                 const SearchSpace& S, bool real, int q, int r)
{
  if (real)
  {
    const int bq = q / L.headings;
    const int h = q - bq * L.headings;
    const int b = L.first_block + bq;
    long long f;
    if (L.member != nullptr)
      f = (long long)L.member[L.start[b] + r];
    else
    {
      const int ib = b / L.nbj, jb = b - ib * L.nbj;
      const int b0 = L.axis_j[jb], nb = L.axis_j[jb + 1] - b0;
      const int ra = r / nb;
      f = (long long)(L.axis_i[ib] + ra) * (long long)L.n_j + (long long)(b0 + (r - ra * nb));
    }
    const long long c = f * (long long)L.headings + (long long)h;
    int i, j, hh;
    double x, y, th;
    search_pose_of(S, c, &i, &j, &hh, &x, &y, &th);
    dst.x[t] = x;
    dst.y[t] = y;
    dst.th[t] = th;
    ids[t] = c;
  }
  else
  {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    dst.x[t] = nan;
    dst.y[t] = nan;
    dst.th[t] = 0.0;
    ids[t] = -1ll;
  }
  dst.w[t] = 1.0;
}

// members base .. base + n - 1 of the concatenated seed into dst[0 .. n); behind the seed's last member: empty slots
__global__ void k_prune_expand_seed(ParticlesDev dst, long long* __restrict__ ids, int n, long long base,
                                    const int* __restrict__ seed_q, const int* __restrict__ seed_off,
                                    const unsigned long long* __restrict__ words, PruneBlocks L, SearchSpace S)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  const int n_seed = (int)words[0];
  const long long m = base + (long long)t;
  if (n_seed == 0 || m >= (long long)seed_off[n_seed])
  {
    prune_write_slot(dst, ids, t, L, S, false, 0, 0);
    return;
  }
  int lo = 0, hi = n_seed - 1;  // the largest r with seed_off[r] <= m (every seed has a member: strictly increasing)
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)seed_off[mid] <= m)
      lo = mid;
    else
      hi = mid - 1;
  }
  prune_write_slot(dst, ids, t, L, S, true, seed_q[lo], (int)(m - (long long)seed_off[lo]));
}

// k_search_select with the candidate of slot idx taken from ids[idx]; a negative id is an empty slot
__global__ __launch_bounds__(kSearchThreads) void k_prune_select(const double* __restrict__ scores, int n,
                                                                 const long long* __restrict__ ids, int K,
                                                                 const SearchEntry* __restrict__ best,
                                                                 const int* __restrict__ best_count,
                                                                 SearchEntry* __restrict__ tile_out,
                                                                 int* __restrict__ tile_count)
{
  search_select_tile<true>(scores, n, 0ll, ids, K, best, best_count, tile_out, tile_count);
}

// tau of this moment: the K-th score of the exact list once it holds K rows (*full), as a double.  floor_key (null in
// the single-engine calls): the largest K-th key any rank of a sharded search published behind its seed
// (k_prune_floor); non-zero, it is a tau of its own -- *full is true and tau the larger of the two.  A zero floor (no
// rank's list was full, or its K-th score was a NaN) changes nothing.
__device__ __forceinline__ double prune_tau(const SearchEntry* best, const int* best_count, int K,
                                            const unsigned long long* floor_key, bool* full)
{
  const bool own = *best_count >= K;
  unsigned long long key = own ? best[K - 1].key : 0ull;
  const unsigned long long fl = floor_key != nullptr ? *floor_key : 0ull;
  if (fl != 0ull)
  {
    // key order is score order, and a NaN K-th score (key 0) is below every floor
    key = (own && key > fl) ? key : fl;
    *full = true;
    return search_score_of(key);
  }
  *full = own;
  return own ? search_score_of(key) : 0.0;
}

// ---- the shared floor of a sharded search (abi_shard_search.inl)
// the word this rank publishes behind its seed: the key of the K-th row of its exact list if it holds K rows, else 0
__global__ void k_prune_floor_word(const SearchEntry* __restrict__ best, const int* __restrict__ best_count, int K,
                                   unsigned long long* __restrict__ word)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *word = *best_count >= K ? best[K - 1].key : 0ull;
}

// one wave: *floor_key = the largest of the W gathered words
__global__ __launch_bounds__(64) void k_prune_floor(const unsigned long long* __restrict__ words, int W,
                                                    unsigned long long* __restrict__ floor_key)
{
  unsigned long long m = (int)threadIdx.x < W ? words[threadIdx.x] : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
    const unsigned long long o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if (threadIdx.x == 0)
    *floor_key = m;
}

// Chunk c = blockIdx.x takes block candidates c * 1024 ...: those outside the seed for which `bound < tau` is not
// true (a NaN bound stays), in index order, to surv_q[c * 1024 + rank]; surv_off = members of the chunk's survivors
// before this one; chunk_info[c] = (survivors, their members).
__global__ __launch_bounds__(kPruneChunk) void k_prune_survivors(const double* __restrict__ bounds, int nq,
                                                                 const uint8_t* __restrict__ in_seed,
                                                                 const SearchEntry* __restrict__ best,
                                                                 const int* __restrict__ best_count, int K,
                                                                 const unsigned long long* __restrict__ floor_key,
                                                                 PruneBlocks L, int* __restrict__ surv_q,
                                                                 int* __restrict__ surv_off,
                                                                 int2* __restrict__ chunk_info)
{
  __shared__ int s_w[16];
  bool full;
  const double tau = prune_tau(best, best_count, K, floor_key, &full);
  const int q = blockIdx.x * kPruneChunk + (int)threadIdx.x;
  bool keep = false;
  int cnt = 0;
  if (q < nq && in_seed[q] == 0)
  {
    keep = !(full && bounds[q] < tau);
    if (keep)
      cnt = prune_members_of(L, q);
  }
  int n_keep, n_members;
  const int rank = prune_block_scan(keep ? 1 : 0, s_w, &n_keep);
  const int off = prune_block_scan(cnt, s_w, &n_members);
  if (keep)
  {
    surv_q[(size_t)blockIdx.x * kPruneChunk + rank] = q;
    surv_off[(size_t)blockIdx.x * kPruneChunk + rank] = off;
  }
  if (threadIdx.x == 0)
    chunk_info[blockIdx.x] = make_int2(n_keep, n_members);
}

// Members base .. base + n - 1 of the concatenated survivors (chunk_moff[c] = members of the chunks before c,
// chunk_moff[n_chunks] = all, from the host).  The survivor a slot belongs to is decided where its first member
// lies: by every thread of it alike in the window it starts in (tau is constant during a kernel), and from state[]
// (1 dropped, 2 expanded; written by the thread of its first member) in the window after, into which its members may
// reach.  words[2 .. 4] count the decisions.
__global__ void k_prune_expand(ParticlesDev dst, long long* __restrict__ ids, int n, long long base,
                               const double* __restrict__ bounds, const SearchEntry* __restrict__ best,
                               const int* __restrict__ best_count, int K,
                               const unsigned long long* __restrict__ floor_key, const int* __restrict__ surv_q,
                               const int* __restrict__ surv_off, const int2* __restrict__ chunk_info,
                               const long long* __restrict__ chunk_moff, int n_chunks, uint8_t* __restrict__ state,
                               unsigned long long* __restrict__ words, PruneBlocks L, SearchSpace S)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  const long long m = base + (long long)t;
  if (m >= chunk_moff[n_chunks])
  {
    prune_write_slot(dst, ids, t, L, S, false, 0, 0);
    return;
  }
  int lo = 0, hi = n_chunks - 1;  // the largest c with chunk_moff[c] <= m: the one chunk with chunk_moff[c + 1] > m
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_moff[mid] <= m)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int c = lo;
  const int local = (int)(m - chunk_moff[c]);
  const int* off = surv_off + (size_t)c * kPruneChunk;
  lo = 0;
  hi = chunk_info[c].x - 1;
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= local)
      lo = mid;
    else
      hi = mid - 1;
  }
  const size_t i = (size_t)c * kPruneChunk + lo;
  const int q = surv_q[i];
  const long long start = chunk_moff[c] + (long long)off[lo];
  bool drop;
  if (start >= base)
  {
    bool full;
    const double tau = prune_tau(best, best_count, K, floor_key, &full);
    drop = full && bounds[q] < tau;
    if (m == start)
    {
      state[i] = drop ? 1 : 2;
      if (drop)
        atomicAdd(&words[2], 1ull);
      else
      {
        atomicAdd(&words[3], 1ull);
        atomicAdd(&words[4], (unsigned long long)prune_members_of(L, q));
      }
    }
  }
  else
    drop = state[i] == 1;
  prune_write_slot(dst, ids, t, L, S, !drop, q, (int)(m - start));
}

}  // namespace bpf
