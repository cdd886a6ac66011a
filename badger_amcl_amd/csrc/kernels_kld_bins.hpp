// BPF_KLD_COUNT_BINS (bpf_pf_set_kld_count): the KLD stop rule over a long draw stream with k = the number of distinct
// histogram keys among the draws so far.  No tree: after k_kld_hash (tmin[slot[m]] = the first draw with m's key) the
// stop rule is a prefix count of the first occurrences, and k_kld_bins_scan takes it in one look-back launch together
// with the stop test, as k_kld2_scan does for the leaf counts.
#pragma once

#include "kernels_kld.hpp"

namespace bpf
{

// Tiles of kKldTile draws, 256 threads of 8 draws each.  Every block counts its tile's first occurrences and publishes
// the count behind the launch's generation in one 64-bit word of `slots` -- (tag << 40) | count, k_kld2_scan's format:
// the value is its own flag, nothing to reset -- then adds up the tiles before it (blocks are dispatched in index
// order; the wait is bounded all the same, and a time-out sets *status).  counts[m] = distinct keys among draws
// 0 .. m; A.flags[2] = the first m + 1 with m + 1 > resampleLimit(counts[m]) (particle_filter.cpp:416).
__global__ __launch_bounds__(256) void k_kld_bins_scan(const KldArgs A, unsigned long long* __restrict__ slots,
                                                      unsigned generation, int* __restrict__ counts, int* status)
{
  constexpr int per = kKldTile / 256;
  __shared__ int s_w[4];
  __shared__ int s_b[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int base = b * kKldTile + tid * per;
  unsigned bits = 0u;
  int sum = 0;
#pragma unroll
  for (int j = 0; j < per; ++j)
  {
    const int m = base + j;
    const bool first = m < A.n && A.h_tmin[A.slot[m]] == m;
    bits |= first ? (1u << j) : 0u;
    sum += first ? 1 : 0;
  }
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
  const unsigned long long tag = (unsigned long long)(generation % 0xFFFFFFu + 1u) << 40;  // never the zeroed slot's
  if (tid == 0)
    __hip_atomic_store(&slots[b], tag | (unsigned long long)(unsigned)(s_w[0] + s_w[1] + s_w[2] + s_w[3]),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int before = 0;
  for (int t = tid; t < b; t += 256)
  {
    unsigned long long w;
    long long t0 = 0;
    for (unsigned spins = 0; ((w = __hip_atomic_load(&slots[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 40) !=
                             (tag >> 40); ++spins)
    {
      __builtin_amdgcn_s_sleep(1);
      if ((spins & 255u) == 255u)
      {
        const long long now = wall_clock64();
        if (t0 == 0)
          t0 = now;
        else if (now - t0 > 5000000ll)  // 50 ms: the tile counts as empty, the status word says so
        {
          atomicExch(status, 1);
          w = tag;
          break;
        }
      }
    }
    before += (int)(w & 0xFFFFFFFFFFull);
  }
  for (int o = 32; o > 0; o >>= 1)
    before += __shfl_xor(before, o, 64);
  if (lane == 0)
    s_b[wave] = before;
  __syncthreads();
  int run = s_b[0] + s_b[1] + s_b[2] + s_b[3];
  for (int q = 0; q < wave; ++q)
    run += s_w[q];
  run += incl - sum;
  int stop = INT_MAX;
#pragma unroll
  for (int j = 0; j < per; ++j)
  {
    const int m = base + j;
    if (m < A.n)
    {
      run += (int)((bits >> j) & 1u);
      counts[m] = run;
      if (m + 1 > A.limit[run] && stop == INT_MAX)
        stop = m + 1;
    }
  }
  if (stop != INT_MAX)
    atomicMin(&A.flags[2], stop);
}

// The result for the host in pinned memory, four 64-bit words (generation << 32) | value, each a system-scope store
// of its own (see k_kld2_result): [1] key outside the packing, [2] stop index (or -1), [3] distinct keys at the stop
// (or at n), [4] status (0: fine).  whole_stream: the count of all n keys, no stop rule.
__global__ void k_kld_bins_result(const KldArgs A, const int* __restrict__ counts, const int* status, int whole_stream,
                                  volatile int* result_host, int generation)
{
  if (threadIdx.x != 0)
    return;
  const int n = A.n;
  const int stop = whole_stream ? -1 : A.flags[2];
  const bool stopped = stop >= 1 && stop <= n;
  const int M = stopped ? stop : n;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(const_cast<int*>(result_host));
  const unsigned long long g = (unsigned long long)(unsigned)generation << 32;
  const int v[5] = { 0, A.flags[0], stopped ? stop : -1, counts[M - 1], *status };
#pragma unroll
  for (int k = 1; k < 5; ++k)
    __hip_atomic_store(&out[k], g | (unsigned long long)(unsigned)v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace bpf
