// Mixture initialiser on the device: the body of ParticleFilter::initWithGaussian's loop (particle_filter.cpp:112-125,
// pdf_gaussian.cpp:52-70) run over K components in index order, component c taking count_c consecutive samples, all
// of them drawing from the ONE drand48 stream in sample order.
//
// The Gaussian stream is generated as for one component (kernels_motion.hpp): the j-th Gaussian is the j-th accepted
// attempt whatever the components are.  Only the draw()'s argument depends on the component: Gaussian j belongs to
// sample j / 3, and the sample's component is found in the exclusive prefix of the counts (the first c with
// prefix[c + 1] > sample, which skips components without samples).
#pragma once
#include "kernels_motion.hpp"

namespace bpf
{

constexpr int kMixtureMax = 1024;  // components (the pose searches' K limit): the search is at most 10 steps
constexpr int kMixtureRow = 15;    // doubles of a table row: mean[3], rotation[9] row-major, sigma[3]

struct MixtureDev
{
  const double* rows;  // [k][kMixtureRow]; the row of a component without samples is never read
  const int* prefix;   // [k + 1] exclusive prefix of the counts of the GLOBAL set; prefix[k] = global sample count
  int k;
};

__device__ __forceinline__ void mixture_stage_prefix(const MixtureDev& X, int* s_prefix)
{
  for (int i = threadIdx.x; i <= X.k; i += blockDim.x)
    s_prefix[i] = X.prefix[i];
  __syncthreads();
}

// the component of global sample s < prefix[k]
__device__ __forceinline__ int mixture_component_of(const int* s_prefix, int k, int s)
{
  int lo = 0, hi = k - 1;
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (s_prefix[mid + 1] > s)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// k_motion_gauss (same tiles, same ranks, same expression; that kernel stays as it is) with
// draw(sigma[component_of(j / 3)][j % 3]).  A thread's ranks ascend, so it searches again only when a rank leaves the
// component of the one before; the scale is read only for a rank that is written (j < need_total, so j / 3 is a
// sample of the set).
__global__ __launch_bounds__(256) void k_mixture_gauss(const MotionRngArgs A, const MixtureDev X)
{
  __shared__ int s_w[4];
  __shared__ int s_prefix[kMixtureMax + 1];
  mixture_stage_prefix(X, s_prefix);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t0 = ((long long)blockIdx.x * 256 + tid) * kMotionRun;
  const long long base = A.tile_offsets[blockIdx.x];
  const long long end = A.tile_offsets[blockIdx.x + 1];
  const bool overlaps = end > A.gauss_first && base < A.gauss_first + A.gauss_count;
  const bool holds_last = base < A.need_total && end >= A.need_total;
  if (!overlaps && !holds_last)
    return;
  int cnt = 0;
  if (t0 < A.n_attempts)
    motion_attempts(A, t0, [&](int, bool ok, double, double, long long) { cnt += ok ? 1 : 0; });
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o)
      incl += v;
  }
  if (lane == 63)
    s_w[wave] = incl;
  __syncthreads();
  int wave_base = 0;
  for (int q = 0; q < wave; ++q)
    wave_base += s_w[q];
  long long rank = base + wave_base + (incl - cnt);
  int c = 0, c_end = 0;  // samples below c_end belong to c or an earlier component
  if (t0 < A.n_attempts)
    motion_attempts(A, t0, [&](int, bool ok, double x2, double w, long long raw) {
      if (!ok)
        return;
      const long long j = rank++;
      const long long o = j - A.gauss_first;
      if (o >= 0 && o < A.gauss_count)
      {
        const int s = (int)(j / 3);
        if (s >= c_end)
        {
          c = mixture_component_of(s_prefix, X.k, s);
          c_end = s_prefix[c + 1];
        }
        const double sd = X.rows[(size_t)c * kMixtureRow + 12 + (int)(j % 3)];
        A.gauss[o] = (sd * x2 * sqrt(-2.0 * log(w) / w));  // pdf_gaussian.cpp:96
      }
      if (j == A.need_total - 1)
        A.result[0] = raw;
    });
}

// k_init_gaussian with the mean and rotation of each sample's component; sample i of this engine is global sample
// first + i.  A wave holds 64 consecutive samples: where its first and its last fall into one component the row is
// the same for every lane and is read through uniform (scalar) loads; a wave that straddles a boundary searches per
// lane.
__global__ __launch_bounds__(256) void k_init_mixture(ParticlesDev dst, int n, int first,
                                                       const double* __restrict__ gauss, const MixtureDev X,
                                                       double weight)
{
#pragma clang fp contract(off)
  __shared__ int s_prefix[kMixtureMax + 1];
  mixture_stage_prefix(X, s_prefix);
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int i0 = __builtin_amdgcn_readfirstlane(i & ~63);
  if (i0 >= n)
    return;
  const int c0 = __builtin_amdgcn_readfirstlane(mixture_component_of(s_prefix, X.k, first + i0));
  const bool one_component = s_prefix[c0 + 1] > first + min(i0 + 63, n - 1);
  if (i >= n)
    return;
  double row[12];
  if (one_component)
  {
    const double* __restrict__ p = X.rows + (size_t)c0 * kMixtureRow;
#pragma unroll
    for (int q = 0; q < 12; ++q)
      row[q] = p[q];
  }
  else
  {
    const double* __restrict__ p = X.rows + (size_t)mixture_component_of(s_prefix, X.k, first + i) * kMixtureRow;
#pragma unroll
    for (int q = 0; q < 12; ++q)
      row[q] = p[q];
  }
  const double r[3] = { gauss[3 * (size_t)i], gauss[3 * (size_t)i + 1], gauss[3 * (size_t)i + 2] };
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    v[k] = row[k];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      v[k] += row[3 + 3 * k + j] * r[j];
  }
  dst.x[i] = v[0];
  dst.y[i] = v[1];
  dst.th[i] = v[2];
  dst.w[i] = weight;
}

}  // namespace bpf
