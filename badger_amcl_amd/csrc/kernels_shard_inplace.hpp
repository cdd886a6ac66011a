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
//   k_inplace_xy_sums           fixed-point sums of the new slice's x and y (kernels_stats.hpp's terms, one word wider):
//                               integer sums, so order-independent and exact over the ranks; a term that does not fit
//                               raises the flag
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

// The sums of x and of y are UNWEIGHTED: n x-bar leaves the 32.96 format (|sum| < 2^31, kernels_stats.hpp) at 100 000
// samples 21.5 km from the frame's origin.  They are therefore carried one word wider, as 96.96 two's complement
// (top, mid, lo) with mid = the 32.96 format's hi word: n <= 2^31 samples of |x| < 2e9 stay below 2^62 and cannot wrap.
struct Fx3
{
  long long top;
  unsigned long long mid, lo;
};

__device__ __forceinline__ Fx3 fx3_from(Fx v)
{
  Fx3 r;
  r.top = v.hi >> 63;  // sign extension
  r.mid = (unsigned long long)v.hi;
  r.lo = v.lo;
  return r;
}

__device__ __forceinline__ Fx3 fx3_add(Fx3 a, Fx3 b)
{
  Fx3 r;
  r.lo = a.lo + b.lo;
  const unsigned long long c0 = r.lo < a.lo ? 1 : 0;
  const unsigned long long m = a.mid + b.mid;
  r.mid = m + c0;
  r.top = a.top + b.top + (long long)((m < a.mid ? 1 : 0) + (r.mid < m ? 1 : 0));
  return r;
}

__device__ __forceinline__ Fx3 fx3_wave_sum(Fx3 v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    Fx3 u;
    u.top = __shfl_xor(v.top, o, 64);
    u.mid = __shfl_xor(v.mid, o, 64);
    u.lo = __shfl_xor(v.lo, o, 64);
    v = fx3_add(v, u);
  }
  return v;
}

// acc_top / acc_hi / acc_lo: [2] (x, y), zero on entry; words[2 * kStatLimbs]: the flag word, zero on entry.  The flag
// is for a term that is not a number of the format (NaN, inf, |x| >= 2e9) only -- it zeroes the count, as a NaN mean
// does; a finite far cloud never raises it.
__global__ __launch_bounds__(256) void k_inplace_xy_sums(const double* __restrict__ x, const double* __restrict__ y,
                                                        int n, long long* acc_top, long long* acc_hi,
                                                        unsigned long long* acc_lo, long long* words)
{
  __shared__ Fx3 s_sum[2][4];
  Fx3 sx, sy;
  sx.top = sy.top = 0;
  sx.mid = sy.mid = 0;
  sx.lo = sy.lo = 0;
  bool bad = false;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
  {
    sx = fx3_add(sx, fx3_from(fx_from(x[i], &bad)));
    sy = fx3_add(sy, fx3_from(fx_from(y[i], &bad)));
  }
  if (bad)
    atomicExch(reinterpret_cast<unsigned long long*>(&words[2 * kStatLimbs]), 1ull);
  sx = fx3_wave_sum(sx);
  sy = fx3_wave_sum(sy);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
  {
    s_sum[0][wave] = sx;
    s_sum[1][wave] = sy;
  }
  __syncthreads();
  if (threadIdx.x < 2)
  {
    Fx3 v = s_sum[threadIdx.x][0];
    for (int w = 1; w < 4; ++w)
      v = fx3_add(v, s_sum[threadIdx.x][w]);
    // the carries out of lo and out of mid are counted by the thread whose add wrapped the word (fx_atomic_add)
    const unsigned long long old_lo = atomicAdd(&acc_lo[threadIdx.x], v.lo);
    const unsigned long long c0 = (old_lo + v.lo < old_lo) ? 1 : 0;
    const unsigned long long add_mid = v.mid + c0;
    const unsigned long long old_mid = atomicAdd(reinterpret_cast<unsigned long long*>(&acc_hi[threadIdx.x]), add_mid);
    const unsigned long long c1 = (add_mid < c0 ? 1 : 0) + (old_mid + add_mid < old_mid ? 1 : 0);
    atomicAdd(reinterpret_cast<unsigned long long*>(&acc_top[threadIdx.x]), (unsigned long long)v.top + c1);
  }
}

// (top, hi, lo) -> four limbs, least significant first, each in an int64 (k_sstat_export's form, but the top limb
// carries everything from 2^0 up, sign included: below 2^62 in magnitude, and still an exact lane-wise sum over the ranks)
__global__ void k_inplace_export(const long long* __restrict__ acc_top, const long long* __restrict__ acc_hi,
                                 const unsigned long long* __restrict__ acc_lo, long long* __restrict__ limbs)
{
  const int i = threadIdx.x;
  if (i >= 2)
    return;
  const unsigned long long mid = (unsigned long long)acc_hi[i], lo = acc_lo[i];
  limbs[(size_t)kStatLimbs * i + 0] = (long long)(lo & 0xFFFFFFFFull);
  limbs[(size_t)kStatLimbs * i + 1] = (long long)(lo >> 32);
  limbs[(size_t)kStatLimbs * i + 2] = (long long)(mid & 0xFFFFFFFFull);
  limbs[(size_t)kStatLimbs * i + 3] = (long long)(((unsigned long long)acc_top[i] << 32) | (mid >> 32));
}

// four limbs summed over the ranks (k_inplace_export's form) -> the sum as a double.  Where the sum fits 32.96 this is
// fx_to_double of it bit for bit: top limb * 2^32 + third limb is the hi word, rounded once like the conversion.
__device__ __forceinline__ double inplace_sum_of(const long long* limbs)
{
  const unsigned long long l0 = (unsigned long long)limbs[0];
  const unsigned long long l1 = (unsigned long long)limbs[1] + (l0 >> 32);
  const unsigned long long l2 = (unsigned long long)limbs[2] + (l1 >> 32);
  const long long l3 = limbs[3] + (long long)(l2 >> 32);
  const unsigned long long lo = (l0 & 0xFFFFFFFFull) | (l1 << 32);
  const double hi = (double)l3 * 4294967296.0 + (double)(l2 & 0xFFFFFFFFull);
  return hi * 2.3283064365386963e-10 + (double)lo * 1.2621774483536189e-29;  // 2^-32, 2^-96
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
