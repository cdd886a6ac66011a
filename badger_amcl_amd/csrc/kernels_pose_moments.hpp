// Pose moments (bpf_planar_pose_moments, bpf_cloud_pose_moments; abi_pose_moments.inl): the score-weighted first and
// second moments of one refinement lattice (kernels_pose_refine.hpp: RefineLattice, refine_pose_of,
// k_refine_candidates) per pose.  One kernel of its own:
//
//   k_pose_moments   one block of 256 threads per pose: the largest score and its point (the refinement's order
//                    rule), then the weights w = s - baseline * s_max above the threshold and their ten sums, then
//                    the row
//
// Thread tid owns the points m = tid, tid + 256, ... (at most 8: M <= 2048) and keeps their scores in registers
// between the two passes.  The order of the sums is part of the contract (include/badger_pf.h), so that a numpy model
// reproduces the bits: per thread ascending from 0.0, the wave64 xor butterfly with offsets 32 .. 1 as
// v = v + shfl_xor(v, off), then waves 0, 1, 2, 3 added in that order by thread 0 through LDS.  A point past M counts
// as a NaN score: weight 0, and the +0.0 it adds changes no partial sum (a sum that starts at +0.0 is never -0.0).
// No atomics, no block that waits for another; every store is a vector store.
#pragma once
#include "kernels_pose_refine.hpp"

namespace bpf
{

constexpr int kMomentsThreads = 256;
constexpr int kMomentsPerThread = kRefineMaxPoints / kMomentsThreads;  // 8
constexpr int kMomentsSums = 10;  // W, Sa, Sb, St, Saa, Sab, Sat, Sbb, Sbt, Stt
static_assert(kMomentsPerThread * kMomentsThreads == kRefineMaxPoints, "every point of the largest lattice is owned");

// Block b is pose r0 + b; its lattice, scored, is scores[b * M ...).  Writes out[r0 + b].
__global__ __launch_bounds__(kMomentsThreads) void k_pose_moments(const double* __restrict__ scores, int r0,
                                                                  RefineLattice G, double baseline,
                                                                  const double* __restrict__ centres,
                                                                  bpf_pose_moments* __restrict__ out)
{
#pragma clang fp contract(off)
  constexpr int kWaves = kMomentsThreads / 64;
  __shared__ SearchEntry s_best[kWaves];
  __shared__ double s_max_shared;
  __shared__ double s_sum[kWaves][kMomentsSums];
  __shared__ int s_support[kWaves];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)G.M;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  // ---- pass 1: the scores into registers, the best point
  double sc[kMomentsPerThread];
  SearchEntry best{ 0ull, 0ull };  // worse than every point
#pragma unroll
  for (int j = 0; j < kMomentsPerThread; ++j)
  {
    const int m = tid + j * kMomentsThreads;
    sc[j] = nan;
    if (m < G.M)
    {
      sc[j] = scores[base + m];
      SearchEntry en;
      en.key = search_key_of(sc[j]);
      en.inv = ~(unsigned long long)(m == G.centre ? 0 : m + 1);
      if (search_better(en, best))
        best = en;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
    SearchEntry o;
    o.key = __shfl_xor(best.key, off, 64);
    o.inv = __shfl_xor(best.inv, off, 64);
    if (search_better(o, best))
      best = o;
  }
  if ((tid & 63) == 0)
    s_best[tid >> 6] = best;
  __syncthreads();
  int m_best = 0;
  if (tid == 0)
  {
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
      if (search_better(s_best[w], best))
        best = s_best[w];
    const int rank = (int)~best.inv;
    m_best = rank == 0 ? G.centre : rank - 1;
    const double top = scores[base + m_best];
    s_max_shared = top != top ? nan : top;
  }
  __syncthreads();
  const double s_max = s_max_shared;
  const double thr = baseline * s_max;

  // ---- pass 2: weights and sums
  double v[kMomentsSums];
#pragma unroll
  for (int q = 0; q < kMomentsSums; ++q)
    v[q] = 0.0;
  int support = 0;
  const int nt = 2 * G.A + 1, nb = 2 * G.R + 1;
#pragma unroll
  for (int j = 0; j < kMomentsPerThread; ++j)
  {
    const int m = tid + j * kMomentsThreads;
    const int ab = m / nt;
    const int t = m - ab * nt;
    const int a = ab / nb;
    const int b = ab - a * nb;
    const double da = (double)(a - G.R), db = (double)(b - G.R), dt = (double)(t - G.A);
    const double w = sc[j] > thr ? sc[j] - thr : 0.0;  // (false for a NaN score and for a point past M)
    support += w > 0.0 ? 1 : 0;
    const double wa = w * da, wb = w * db, wt = w * dt;
    v[0] = v[0] + w;
    v[1] = v[1] + wa;
    v[2] = v[2] + wb;
    v[3] = v[3] + wt;
    v[4] = v[4] + wa * da;
    v[5] = v[5] + wa * db;
    v[6] = v[6] + wa * dt;
    v[7] = v[7] + wb * db;
    v[8] = v[8] + wb * dt;
    v[9] = v[9] + wt * dt;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
#pragma unroll
    for (int q = 0; q < kMomentsSums; ++q)
      v[q] = v[q] + __shfl_xor(v[q], off, 64);
    support += __shfl_xor(support, off, 64);
  }
  if ((tid & 63) == 0)
  {
#pragma unroll
    for (int q = 0; q < kMomentsSums; ++q)
      s_sum[tid >> 6][q] = v[q];
    s_support[tid >> 6] = support;
  }
  __syncthreads();
  if (tid != 0)
    return;
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
  {
#pragma unroll
    for (int q = 0; q < kMomentsSums; ++q)
      v[q] = v[q] + s_sum[w][q];
    support += s_support[w];
  }

  // ---- the row
  const double* c = centres + 3 * (size_t)(r0 + blockIdx.x);
  bpf_pose_moments row;
  row.mean[0] = c[0];
  row.mean[1] = c[1];
  row.mean[2] = c[2];
#pragma unroll
  for (int q = 0; q < 6; ++q)
    row.cov[q] = 0.0;
  row.weight_sum = 0.0;
  row.score_max = s_max;
  row.support = 0;
  row.flags = 0;
  if (s_max > 0.0)  // (false for NaN)
  {
    const double d = G.xy_step, q = G.theta_step;
    const double W = v[0];
    const double ma = v[1] / W, mb = v[2] / W, mt = v[3] / W;
    row.mean[0] = c[0] + ma * d;
    row.mean[1] = c[1] + mb * d;
    row.mean[2] = c[2] + mt * q;
    row.cov[0] = (v[4] / W - ma * ma) * d * d;
    row.cov[1] = (v[5] / W - ma * mb) * d * d;
    row.cov[2] = (v[6] / W - ma * mt) * d * q;
    row.cov[3] = (v[7] / W - mb * mb) * d * d;
    row.cov[4] = (v[8] / W - mb * mt) * d * q;
    row.cov[5] = (v[9] / W - mt * mt) * q * q;
    row.weight_sum = W;
    row.support = support;
    const int ab = m_best / nt;
    const int t = m_best - ab * nt;
    const int a = ab / nb;
    const int b = ab - a * nb;
    int flags = BPF_MOMENTS_VALID;
    if (G.R > 0 && (a == 0 || a == 2 * G.R))
      flags |= BPF_MOMENTS_FACE_X;
    if (G.R > 0 && (b == 0 || b == 2 * G.R))
      flags |= BPF_MOMENTS_FACE_Y;
    if (G.A > 0 && (t == 0 || t == 2 * G.A))
      flags |= BPF_MOMENTS_FACE_THETA;
    row.flags = flags;
  }
  out[r0 + blockIdx.x] = row;
}

}  // namespace bpf
