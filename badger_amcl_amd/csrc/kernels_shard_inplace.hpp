// Systematic resampling of a SHARDED set in place: every rank resamples its own slice into its own slice.
//
// The comb of targets u0 + i / n is known to every rank (one drand48 and the gathered totals), and the teeth that fall
// into shard q's slice [T_q, T_q+1) of the global CDF pick particles of shard q only.  In ascending-target order the
// teeth of shard 0 come first, then shard 1's, ...: the concatenation of the ranks' new slices is the reference's new
// set with the wrapped teeth moved to the front (a rotation of the teeth; the random poses of w_diff > 0 stay first, on
// rank 0).  No particle and no draw window crosses; what does is W totals, the occupied-bin lists of the new tree
// (kernels_shard_init.hpp) and a few integer words for updateConverged.
//
//   k_systematic_select_local   one thread per sample of the NEW slice: its position is its rank in ascending-target
//                               order (the host hands over the ascending targets from this rank's first tooth on), its
//                               source the bisection of the local CDF with the window kernel's ownership and rounding
//                               rules (draw_window_column as it is); rank 0's head are the random free-space poses
//   k_inplace_xy_sums           32.96 fixed-point sums of the new slice's x and y (kernels_stats.hpp): integer sums, so
//                               order-independent and exact over the ranks; a term that does not fit raises the flag
//   -- exchange: integer all-reduce(sum) of 8 limb words + the flag word --
//   k_inplace_converged_count   the mean from the reduced integers, the same bits on every rank; the slice's particles
//                               within dist_threshold of it on both axes
//   -- exchange: integer all-reduce(sum) of the count --
//
// No kernel here waits for another rank: every exchange sits between launches.
#pragma once
#include "kernels_pf.hpp"
#include "kernels_shard_stats.hpp"

namespace bpf
{

constexpr int kInplaceSumWords = 2 * kStatLimbs + 1;  // x limbs, y limbs, flag

struct InplaceSelectArgs
{
  // src, n_src, cdf, rank, world, flags, rng_state, jump as for k_draw_window; m0 = 0, m1 = samples of the new slice;
  // targets = the ascending targets from this rank's first tooth on; rank 0: n_random, write_random, free_space
  WindowArgs W;
  double offset, top;  // this shard's slice of the global CDF (shard_slice's values, formed by the host)
  ParticlesDev dst;
  double weight;       // 1 / M
};

__global__ __launch_bounds__(256) void k_systematic_select_local(const InplaceSelectArgs A)
{
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= A.W.m1)
    return;
  long long out[6];
  // false: a tooth the host counted into this slice and the ownership test disowns (cannot happen: same comparisons on
  // the same doubles), or a tooth that rounding sends to a shard without particles -- the reference's failed search.
  // The flag is raised and the sample reads as the zero column the window form would have summed.
  if (!draw_window_column(A.W, o, out, A.offset, A.top))
    atomicExch(A.W.flags, 1);
  A.dst.x[o] = __longlong_as_double(out[0]);
  A.dst.y[o] = __longlong_as_double(out[1]);
  A.dst.th[o] = __longlong_as_double(out[2]);
  A.dst.w[o] = A.weight;
}

__device__ __forceinline__ Fx fx_wave_sum(Fx v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    Fx u;
    u.hi = __shfl_xor(v.hi, o, 64);
    u.lo = __shfl_xor(v.lo, o, 64);
    v = fx_add(v, u);
  }
  return v;
}

// acc_hi / acc_lo: [2] (x, y), zero on entry; words[2 * kStatLimbs]: the flag word, zero on entry
__global__ __launch_bounds__(256) void k_inplace_xy_sums(const double* __restrict__ x, const double* __restrict__ y,
                                                        int n, long long* acc_hi, unsigned long long* acc_lo,
                                                        long long* words)
{
  __shared__ long long s_hi[2][4];
  __shared__ unsigned long long s_lo[2][4];
  Fx sx, sy;
  sx.hi = sy.hi = 0;
  sx.lo = sy.lo = 0;
  bool bad = false;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
  {
    sx = fx_add(sx, fx_from(x[i], &bad));
    sy = fx_add(sy, fx_from(y[i], &bad));
  }
  if (bad)
    atomicExch(reinterpret_cast<unsigned long long*>(&words[2 * kStatLimbs]), 1ull);
  sx = fx_wave_sum(sx);
  sy = fx_wave_sum(sy);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
  {
    s_hi[0][wave] = sx.hi;
    s_lo[0][wave] = sx.lo;
    s_hi[1][wave] = sy.hi;
    s_lo[1][wave] = sy.lo;
  }
  __syncthreads();
  if (threadIdx.x < 2)
  {
    Fx v;
    v.hi = s_hi[threadIdx.x][0];
    v.lo = s_lo[threadIdx.x][0];
    for (int w = 1; w < 4; ++w)
    {
      Fx u;
      u.hi = s_hi[threadIdx.x][w];
      u.lo = s_lo[threadIdx.x][w];
      v = fx_add(v, u);
    }
    fx_atomic_add(&acc_hi[threadIdx.x], &acc_lo[threadIdx.x], v);
  }
}

// four limbs summed over the ranks (k_sstat_export's form) -> the sum as a double
__device__ __forceinline__ double inplace_sum_of(const long long* limbs)
{
  const unsigned long long l0 = (unsigned long long)limbs[0];
  const unsigned long long l1 = (unsigned long long)limbs[1] + (l0 >> 32);
  const unsigned long long l2 = (unsigned long long)limbs[2] + (l1 >> 32);
  const long long l3 = limbs[3] + (long long)(l2 >> 32);
  const unsigned long long lo = (l0 & 0xFFFFFFFFull) | (l1 << 32);
  const long long hi = (long long)((l2 & 0xFFFFFFFFull) | ((unsigned long long)l3 << 32));
  return fx_to_double(hi, lo);
}

// reduced: the kInplaceSumWords words after the all-reduce; *count: zero on entry.  A raised flag on any rank leaves the
// count at 0, as the reference's comparisons against a NaN mean do (particle_filter.cpp:170-220).
__global__ __launch_bounds__(256) void k_inplace_converged_count(const double* __restrict__ x,
                                                                const double* __restrict__ y, int n,
                                                                const long long* __restrict__ reduced,
                                                                int global_count, double thr, long long* count)
{
  __shared__ int s_cnt[4];
  if (reduced[2 * kStatLimbs] != 0)
    return;
  const double mx = inplace_sum_of(reduced) / global_count, my = inplace_sum_of(reduced + kStatLimbs) / global_count;
  int c = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    if (fabs(x[i] - mx) <= thr && fabs(y[i] - my) <= thr)
      c++;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    c += __shfl_xor(c, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    s_cnt[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(count),
              (unsigned long long)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]));
}

}  // namespace bpf
