// Cluster statistics of a set that is SHARDED over several engines (kernels_stats.hpp for one engine): the
// distributed form of ParticleFilter::computeClusterStatsForSet (particle_filter.cpp:505-636) with PFKDTree::cluster
// (pf_kdtree.cpp:58-90,169-194).  No kernel here waits for another rank: the two exchanges happen between launches.
//
//   local bins   the slice's distinct packed keys with the GLOBAL index of each key's first sample, compacted out of
//                the hash table k_kld_hash builds into a dense list in increasing first-index order
//                (k_sstat_first_count, k_stats_scan_offsets, k_sstat_compact)
//   -- exchange 1: all-gather of the lists --
//   merge        one global bin table from every rank's list; a key that several ranks hold keeps its smallest first
//                index (k_gstat_insert).  A rank's list holds a key once, so a table slot sees at most `world` atomics.
//   clusters     union-find over the 26 neighbours of each BIN, the later root hooked under the earlier
//                (k_gstat_union); labels = exclusive scan of "this bin is a root" over the bins in first-index order,
//                which is the order of the gathered lists (k_gstat_roots, k_stats_scan_offsets, k_gstat_labels,
//                k_gstat_binlabel).  Redundant on every rank, same result on every rank.
//   local sums   every sample of the slice finds its bin's label in the global table and adds its ten terms to the
//                rank's own 32.96 fixed-point accumulators (k_sstat_accumulate); they leave as four 32-bit limbs per
//                sum, each in an int64 (k_sstat_export): a lane-wise int64 sum over <= 16 ranks cannot overflow a
//                limb's word, so a plain integer all-reduce adds the 128-bit numbers exactly.
//   -- exchange 2: integer all-reduce(sum) of the limbs --
//   finish       carries propagated back into (hi, lo) (k_sstat_import), then k_stats_clusters / k_stats_set of the
//                single engine on the reduced sums: the same integers, the same finishing code, the same doubles.
//
// The range of the fixed-point sums (|sum| < 2^31, kernels_stats.hpp) is only known once they are formed, after the
// last exchange.  A rank whose own additions leave the format (k_sstat_accumulate) marks every sum it exports with a
// top limb no sum in range can reach (kStatPoison); k_sstat_import finds a top limb that does not fit its 32 bits --
// a marked one, or a total that passed 2^31 although every rank's share fitted -- on EVERY rank alike, since all of
// them read the same reduced words, and raises flags[1]: nothing is installed and every rank takes the host route.
//
// Every probe loop and every union-find walk is bounded by the table size; a bound that is hit sets flags[3] (it
// cannot be with a table of at least twice the bins, and is reported as an error, not waited out).
#pragma once
#include "kernels_stats.hpp"

namespace bpf
{

constexpr int kShardStatsMaxWorld = 16;
constexpr int kStatLimbs = 4;

// the ten terms of one sample, exactly as k_stats_accumulate forms them (particle_filter.cpp:577-600)
__device__ __forceinline__ void stats_terms(double x, double y, double th, double w, Fx* t, bool* bad)
{
  double s, c;
  sincos(th, &s, &c);
  t[0] = fx_from(w, bad);
  t[1] = fx_from(w * x, bad);
  t[2] = fx_from(w * y, bad);
  t[3] = fx_from(w * c, bad);
  t[4] = fx_from(w * s, bad);
  t[5] = fx_from(w * x * x, bad);
  t[6] = fx_from(w * x * y, bad);
  t[7] = fx_from(w * y * x, bad);
  t[8] = fx_from(w * y * y, bad);
  t[9].hi = 1ll << 32;  // the count: 1.0
  t[9].lo = 0;
}

// ---- local bins
struct ShardBinsArgs
{
  ParticlesDev p;
  int n;
  long long global_first;            // global index of the slice's sample 0
  const unsigned long long* h_key;   // the slice's hash table (k_kld_hash)
  const int* h_tmin;
  const int* slot;                   // [n]
  int* flags;                        // [0] key out of range, [1] non-finite term, [2] scan total, [3] bound hit
  int* tile_sums;
  long long* bins;                   // out: [2][flags[2]] packed key, global first index
};

// per tile: the number of first samples of a bin; and the test the sums will make of every term (a non-finite term
// anywhere sends every rank to the host evaluation, so it has to be known before the first exchange)
__global__ __launch_bounds__(256) void k_sstat_first_count(const ShardBinsArgs A)
{
  __shared__ int s_w[4];
  const int base = blockIdx.x * kStatTile;
  int cnt = 0;
  bool bad = false;
  for (int j = threadIdx.x; j < kStatTile; j += 256)
  {
    const int i = base + j;
    if (i < A.n)
    {
      cnt += (A.h_tmin[A.slot[i]] == i) ? 1 : 0;
      Fx t[kStatTerms];
      stats_terms(A.p.x[i], A.p.y[i], A.p.th[i], A.p.w[i], t, &bad);
    }
  }
  if (bad)
    atomicExch(&A.flags[1], 1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
    A.tile_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the first samples in index order -> the dense list (tile_sums holds the exclusive offsets now, flags[2] the total)
__global__ __launch_bounds__(256) void k_sstat_compact(const ShardBinsArgs A)
{
  __shared__ int s_w[4];
  constexpr int per = kStatTile / 256;
  const int base = blockIdx.x * kStatTile + threadIdx.x * per;
  const int total = A.flags[2];
  int f[per];
  int sum = 0;
#pragma unroll
  for (int j = 0; j < per; ++j)
  {
    f[j] = (base + j < A.n && A.h_tmin[A.slot[base + j]] == base + j) ? 1 : 0;
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
      if (run < total)
      {
        A.bins[run] = (long long)A.h_key[A.slot[base + j]];
        A.bins[(size_t)total + run] = A.global_first + base + j;
      }
      run += 1;
    }
}

// ---- merge and label (every rank, redundantly)
struct GlobalBinsArgs
{
  const long long* all;              // [world][2][pad]: the gathered lists
  int world, pad;
  int counts[kShardStatsMaxWorld];
  unsigned long long* g_key;         // global bin table: packed key per slot (kKldEmpty = free)
  int* g_tmin;                       // smallest global first index of the key
  unsigned g_mask;
  unsigned long long* parent;        // [table] union-find: (first index << 32 | slot) of the parent bin
  int* eslot;                        // [world pad] table slot of a list entry
  int* eroot;                        // [world pad] slot of the entry's root (entries that own their bin), else -1
  int* label;                        // [table] cluster index, at the slots of root bins
  int* binlabel;                     // [table] cluster index of every bin
  int* flags;                        // as ShardBinsArgs
};

__device__ __forceinline__ bool gstat_entry(const GlobalBinsArgs& A, int j, unsigned long long* key, int* first)
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

__device__ __forceinline__ unsigned gstat_hash(unsigned long long pk, unsigned mask)
{
  return (unsigned)((pk * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// slot of a key in the global table, -1: not there (or the probe bound was hit)
__device__ __forceinline__ int gstat_lookup(const unsigned long long* g_key, unsigned mask, unsigned long long pk)
{
  unsigned h = gstat_hash(pk, mask);
  for (unsigned probe = 0; probe <= mask; ++probe)
  {
    const unsigned long long held = g_key[h];
    if (held == kKldEmpty)
      return -1;
    if (held == pk)
      return (int)h;
    h = (h + 1) & mask;
  }
  return -1;
}

__global__ void k_gstat_insert(const GlobalBinsArgs A)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long pk;
  int first;
  if (!gstat_entry(A, j, &pk, &first))
    return;
  unsigned h = gstat_hash(pk, A.g_mask);
  int at = -1;
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
  {
    atomicExch(&A.flags[3], 1);
    at = 0;
  }
  else
    atomicMin(&A.g_tmin[at], first);
  A.eslot[j] = at;
}

__device__ __forceinline__ unsigned long long gstat_node(int first, int slot)
{
  return ((unsigned long long)(unsigned)first << 32) | (unsigned)slot;
}

__global__ void k_gstat_init(const GlobalBinsArgs A)
{
  const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= A.g_mask)
    A.parent[s] = gstat_node(A.g_tmin[s], (int)s);  // an occupied slot: the bin is its own root
}

// a chain leads to strictly earlier bins, so it is shorter than the table
__device__ __forceinline__ unsigned long long gstat_find(const GlobalBinsArgs& A, unsigned long long v)
{
  for (unsigned step = 0; step <= A.g_mask; ++step)
  {
    const unsigned long long p =
        __hip_atomic_load(&A.parent[(unsigned)v & A.g_mask], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == v)
      return v;
    v = p;
  }
  atomicExch(&A.flags[3], 1);
  return v;
}

// one thread per bin (the list entry that holds the bin's smallest first index): unite with the occupied neighbours
__global__ void k_gstat_union(const GlobalBinsArgs A)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long mine;
  int first;
  if (!gstat_entry(A, j, &mine, &first))
    return;
  const int my_slot = A.eslot[j];
  if (A.g_tmin[my_slot] != first)
    return;  // a lower rank holds this key too: its entry is the bin
  const int k0 = (int)(mine >> 40) - (1 << 23), k1 = (int)((mine >> 16) & 0xFFFFFFull) - (1 << 23),
            k2 = (int)(mine & 0xFFFFull) - (1 << 15);
  const unsigned long long self = gstat_node(first, my_slot);
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dt = -1; dt <= 1; ++dt)
      {
        if (!dx && !dy && !dt)
          continue;
        const int nk[3] = { k0 + dx, k1 + dy, k2 + dt };
        unsigned long long npk;
        if (!kld_pack(nk, &npk))
          continue;  // a key outside the packing range cannot be in the table
        const int os = gstat_lookup(A.g_key, A.g_mask, npk);
        if (os < 0)
          continue;
        // the later root goes under the earlier (k_stats_union); a root that was hooked meanwhile is followed
        unsigned long long a = gstat_find(A, self), b = gstat_find(A, gstat_node(A.g_tmin[os], os));
        bool done = a == b;
        for (unsigned turn = 0; !done && turn <= 4 * A.g_mask + 64; ++turn)
        {
          if (a < b)
          {
            const unsigned long long t = a;
            a = b;
            b = t;
          }
          const unsigned long long old = atomicMin(&A.parent[(unsigned)a & A.g_mask], b);
          if (old == a)
          {
            done = true;
            break;
          }
          a = gstat_find(A, old);
          b = gstat_find(A, b);
          done = a == b;
        }
        if (!done)
          atomicExch(&A.flags[3], 1);
      }
}

// per list entry: the root of its bin; tile sums of "this entry is a root bin" for the scan
__global__ __launch_bounds__(256) void k_gstat_roots(const GlobalBinsArgs A, int* __restrict__ tile_sums)
{
  __shared__ int s_w[4];
  const int base = blockIdx.x * kStatTile;
  int cnt = 0;
  for (int q = threadIdx.x; q < kStatTile; q += 256)
  {
    const int j = base + q;
    unsigned long long pk;
    int first;
    if (j < A.world * A.pad)
    {
      int root = -1;
      if (gstat_entry(A, j, &pk, &first) && A.g_tmin[A.eslot[j]] == first)
      {
        const unsigned long long self = gstat_node(first, A.eslot[j]);
        const unsigned long long r = gstat_find(A, self);
        root = (int)((unsigned)r & A.g_mask);
        cnt += (r == self) ? 1 : 0;
      }
      A.eroot[j] = root;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0)
    s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
    tile_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// label[root slot] = rank of the root among the roots, in first-index order (= list order: the shards are contiguous)
__global__ __launch_bounds__(256) void k_gstat_labels(const GlobalBinsArgs A, const int* __restrict__ tile_offsets)
{
  __shared__ int s_w[4];
  constexpr int per = kStatTile / 256;
  const int base = blockIdx.x * kStatTile + threadIdx.x * per;
  const int total = A.world * A.pad;
  int f[per];
  int sum = 0;
#pragma unroll
  for (int q = 0; q < per; ++q)
  {
    const int j = base + q;
    f[q] = (j < total && A.eroot[j] >= 0 && A.eroot[j] == A.eslot[j]) ? 1 : 0;
    sum += f[q];
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
  int run = tile_offsets[blockIdx.x] + incl - sum;
  for (int q = 0; q < wave; ++q)
    run += s_w[q];
#pragma unroll
  for (int q = 0; q < per; ++q)
    if (f[q])
    {
      A.label[A.eslot[base + q]] = run;
      run += 1;
    }
}

__global__ void k_gstat_binlabel(const GlobalBinsArgs A)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < A.world * A.pad && A.eroot[j] >= 0)
    A.binlabel[A.eslot[j]] = A.label[A.eroot[j]];
}

// ---- local sums
struct ShardSumsArgs
{
  ParticlesDev p;
  int n;
  const int* keys;                   // [3 n] bin keys of the slice (k_set_keys)
  const unsigned long long* g_key;
  unsigned g_mask;
  const int* binlabel;
  int clusters;                      // stride of the accumulators
  long long* acc_hi;                 // [kStatTerms][clusters]
  unsigned long long* acc_lo;
  int* flags;
};

// As k_stats_accumulate, one level further: a converged set puts every sample of a block into one cluster, and
// same-address atomics serialise in L2, so a block whose four waves share a cluster folds their sums in LDS and sends
// one set of atomics; a wave that shares a cluster sends one set; everything else goes sample by sample.
__global__ __launch_bounds__(256) void k_sstat_accumulate(const ShardSumsArgs A)
{
  __shared__ long long s_hi[kStatTerms];
  __shared__ unsigned long long s_lo[kStatTerms];
  __shared__ int s_c[4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = i < A.n;
  int cidx = -1;
  Fx t[kStatTerms];
  bool bad = false;
  if (threadIdx.x < kStatTerms)
  {
    s_hi[threadIdx.x] = 0;
    s_lo[threadIdx.x] = 0;
  }
  if (live)
  {
    unsigned long long pk;
    const int slot = kld_pack(&A.keys[3 * (size_t)i], &pk) ? gstat_lookup(A.g_key, A.g_mask, pk) : -1;
    if (slot >= 0)
      cidx = A.binlabel[slot];
    if (cidx < 0 || cidx >= A.clusters)
    {
      atomicExch(&A.flags[3], 1);  // the slice's own bins are all in the table: cannot happen
      cidx = -1;
    }
    stats_terms(A.p.x[i], A.p.y[i], A.p.th[i], A.p.w[i], t, &bad);
  }
  else
  {
#pragma unroll
    for (int k = 0; k < kStatTerms; ++k)
    {
      t[k].hi = 0;
      t[k].lo = 0;
    }
  }
  const int first = __builtin_amdgcn_readfirstlane(cidx);
  const bool uniform = __builtin_amdgcn_ballot_w64(live && cidx != first) == 0 && first >= 0;
  if (lane == 0)
    s_c[wave] = uniform ? first : -1;
  __syncthreads();
  const bool block_uniform = s_c[0] >= 0 && s_c[1] == s_c[0] && s_c[2] == s_c[0] && s_c[3] == s_c[0];
  if (uniform)
  {
#pragma unroll
    for (int k = 0; k < kStatTerms; ++k)
    {
      Fx v = t[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)
      {
        Fx u;
        u.hi = __shfl_xor(v.hi, o, 64);
        u.lo = __shfl_xor(v.lo, o, 64);
        v = fx_add(v, u, &bad);
      }
      if (lane == 0)
      {
        if (block_uniform)
          bad |= fx_atomic_add(&s_hi[k], &s_lo[k], v);
        else
          bad |= fx_atomic_add(&A.acc_hi[(size_t)k * A.clusters + first], &A.acc_lo[(size_t)k * A.clusters + first], v);
      }
    }
  }
  else if (live && cidx >= 0)
  {
#pragma unroll
    for (int k = 0; k < kStatTerms; ++k)
      bad |= fx_atomic_add(&A.acc_hi[(size_t)k * A.clusters + cidx], &A.acc_lo[(size_t)k * A.clusters + cidx], t[k]);
  }
  if (block_uniform)
  {
    __syncthreads();
    if (threadIdx.x < kStatTerms)
    {
      Fx v;
      v.hi = s_hi[threadIdx.x];
      v.lo = s_lo[threadIdx.x];
      const size_t at = (size_t)threadIdx.x * A.clusters + s_c[0];
      bad |= fx_atomic_add(&A.acc_hi[at], &A.acc_lo[at], v);
    }
  }
  if (bad)  // a term or a sum outside the format
    atomicExch(&A.flags[1], 1);
}

// A top limb in range is below 2^31 in magnitude, sixteen of them below 2^35: a poisoned one stays out of the 32 bits
// k_sstat_import has for it whatever the other ranks add, and sixteen of them are far from the end of the int64.
constexpr long long kStatPoison = 1ll << 45;

// (hi, lo) -> four 32-bit limbs, least significant first, each in an int64; the top one keeps the sign.  flags[1] up
// (this rank's sums left the format): every top limb is poisoned.
__global__ void k_sstat_export(const long long* __restrict__ acc_hi, const unsigned long long* __restrict__ acc_lo,
                               int n_sums, long long* __restrict__ limbs, const int* __restrict__ flags)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sums)
    return;
  if (flags[1] != 0)
  {
    limbs[(size_t)kStatLimbs * i + 0] = limbs[(size_t)kStatLimbs * i + 1] = limbs[(size_t)kStatLimbs * i + 2] = 0;
    limbs[(size_t)kStatLimbs * i + 3] = kStatPoison;
    return;
  }
  const long long hi = acc_hi[i];
  const unsigned long long lo = acc_lo[i];
  limbs[(size_t)kStatLimbs * i + 0] = (long long)(lo & 0xFFFFFFFFull);
  limbs[(size_t)kStatLimbs * i + 1] = (long long)(lo >> 32);
  limbs[(size_t)kStatLimbs * i + 2] = (long long)((unsigned long long)hi & 0xFFFFFFFFull);
  limbs[(size_t)kStatLimbs * i + 3] = hi >> 32;
}

// limbs summed over the ranks (each below 2^36 in magnitude) -> (hi, lo) with the carries propagated; a total whose top
// limb does not fit the 32 bits left for it in `hi` raises flags[1]
__global__ void k_sstat_import(const long long* __restrict__ limbs, int n_sums, long long* __restrict__ acc_hi,
                               unsigned long long* __restrict__ acc_lo, int* __restrict__ flags, int clusters)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0)
    flags[2] = clusters;  // what k_stats_clusters / k_stats_set read as the cluster count
  if (i >= n_sums)
    return;
  const unsigned long long l0 = (unsigned long long)limbs[(size_t)kStatLimbs * i + 0];
  const unsigned long long l1 = (unsigned long long)limbs[(size_t)kStatLimbs * i + 1] + (l0 >> 32);
  const unsigned long long l2 = (unsigned long long)limbs[(size_t)kStatLimbs * i + 2] + (l1 >> 32);
  const long long l3 = limbs[(size_t)kStatLimbs * i + 3] + (long long)(l2 >> 32);
  acc_lo[i] = (l0 & 0xFFFFFFFFull) | (l1 << 32);
  acc_hi[i] = (long long)((l2 & 0xFFFFFFFFull) | ((unsigned long long)l3 << 32));
  if (l3 != (long long)(int)l3)
    atomicExch(&flags[1], 1);
}

__global__ void k_sstat_fill(double* __restrict__ w, int n, double v)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    w[i] = v;
}

}  // namespace bpf
