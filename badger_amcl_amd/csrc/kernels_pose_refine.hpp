// Pose refinement (bpf_planar_refine_poses, bpf_cloud_refine_poses; abi_pose_refine.inl): a coarse-to-fine descent on
// a lattice of (2R+1)^2 (2A+1) poses around each of up to 1024 centres.  Level l scores the lattice with steps
// xy_step * 2^-l and theta_step * 2^-l through the scoring path the searches use, moves every centre to its best
// point, and level l + 1 starts from there.  Three kernels of its own:
//
//   k_refine_candidates   the lattice poses of a group of centres into the engine's candidate set (one lane per
//                         (pose, m)); the centres are read from device memory, where the level before left them
//   k_refine_select       one block per pose: argmax of its M scores, the new centre, score, moved, the trace entry
//   k_refine_rows         the result as bpf_pose_refined rows
//
// Order (include/badger_pf.h): score descending, among equal scores the centre first, then m ascending, NaN below
// every number.  It is encoded the way SearchEntry encodes the search's: key = search_key_of(score), inv = ~rank with
// rank 0 for the centre and m + 1 otherwise, "better" the lexicographically larger (key, inv).  Ranks are distinct,
// so the order is total and the result does not depend on which lane met which point.  A centre that is chosen again
// is not written: a flat or all-NaN neighbourhood leaves the pose bit for bit where it was (-0.0 included, which
// cx + 0.0 * d would turn into +0.0).  No atomics, no block that waits for another: the launches' order on the stream
// is the only synchronisation.
#pragma once
#include "device_types.hpp"
#include "kernels_pose_search.hpp"

namespace bpf
{

constexpr int kRefineMaxPoses = 1024;  // API limits
constexpr int kRefineMaxPoints = 2048;
constexpr int kRefineMaxLevels = 16;
constexpr int kRefineThreads = 256;  // of k_refine_select: 4 waves

// the lattice and the steps of one level.  xy_step / theta_step are already scaled (ldexp on the host), and 0.0 where
// the radius is 0 (the caller's step is then not read)
struct RefineLattice
{
  int R, A;    // xy_radius, theta_radius
  int M;       // (2R+1)^2 (2A+1)
  int centre;  // m_c
  double xy_step, theta_step;
};

// the pose of point m around (cx, cy, cth): evaluated in double as written, no contraction
__device__ __forceinline__ void refine_pose_of(const RefineLattice& G, int m, double cx, double cy, double cth,
                                               double* x, double* y, double* th)
{
#pragma clang fp contract(off)
  const int nt = 2 * G.A + 1, nb = 2 * G.R + 1;
  const int ab = m / nt;
  const int t = m - ab * nt;
  const int a = ab / nb;
  const int b = ab - a * nb;
  *x = cx + (double)(a - G.R) * G.xy_step;
  *y = cy + (double)(b - G.R) * G.xy_step;
  *th = cth + (double)(t - G.A) * G.theta_step;
}

// poses r0 .. r0 + n_group - 1: lane t is point t % M of pose r0 + t / M, written to dst[t]
__global__ void k_refine_candidates(ParticlesDev dst, int n_group, int r0, const double* __restrict__ centres,
                                    RefineLattice G)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_group * G.M)
    return;
  const int r = t / G.M;
  const int m = t - r * G.M;
  const double* c = centres + 3 * (size_t)(r0 + r);
  double x, y, th;
  refine_pose_of(G, m, c[0], c[1], c[2], &x, &y, &th);
  dst.x[t] = x;
  dst.y[t] = y;
  dst.th[t] = th;
  dst.w[t] = 1.0;
}

// Block b is pose r0 + b; its lattice, scored, is cand[b * M ...).  Writes centres / score / moved of that pose and
// trace[(r0 + b) * levels + level]; level 0 sets score_in and moved first.
__global__ __launch_bounds__(kRefineThreads) void k_refine_select(ParticlesDev cand, int r0, RefineLattice G, int level,
                                                                  int levels, double* __restrict__ centres,
                                                                  double* __restrict__ score,
                                                                  double* __restrict__ score_in,
                                                                  int* __restrict__ moved, int* __restrict__ trace)
{
  const double* __restrict__ scores = cand.w;
  __shared__ SearchEntry s[kRefineThreads / 64];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)G.M;
  SearchEntry best{ 0ull, 0ull };  // worse than every point: inv of a point is ~rank with rank <= 2048
  for (int m = tid; m < G.M; m += kRefineThreads)
  {
    SearchEntry en;
    en.key = search_key_of(scores[base + m]);
    en.inv = ~(unsigned long long)(m == G.centre ? 0 : m + 1);
    if (search_better(en, best))
      best = en;
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
    s[tid >> 6] = best;
  __syncthreads();
  if (tid != 0)
    return;
#pragma unroll
  for (int w = 1; w < kRefineThreads / 64; ++w)
    if (search_better(s[w], best))
      best = s[w];
  const int rank = (int)~best.inv;
  const int m = rank == 0 ? G.centre : rank - 1;
  const int r = r0 + blockIdx.x;
  int mv = level == 0 ? 0 : moved[r];
  if (level == 0)
    score_in[r] = scores[base + G.centre];
  if (m != G.centre)
  {
    // the pose as k_refine_candidates wrote it: the same three expressions, not evaluated a second time
    centres[3 * (size_t)r] = cand.x[base + m];
    centres[3 * (size_t)r + 1] = cand.y[base + m];
    centres[3 * (size_t)r + 2] = cand.th[base + m];
    ++mv;
  }
  score[r] = scores[base + m];
  moved[r] = mv;
  trace[(size_t)r * levels + level] = m;
}

// the result as rows for the caller
__global__ void k_refine_rows(int n, const double* __restrict__ centres, const double* __restrict__ score,
                              const double* __restrict__ score_in, const int* __restrict__ moved,
                              bpf_pose_refined* __restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n)
    return;
  bpf_pose_refined row;
  row.pose[0] = centres[3 * (size_t)r];
  row.pose[1] = centres[3 * (size_t)r + 1];
  row.pose[2] = centres[3 * (size_t)r + 2];
  row.score = score[r];
  row.score_in = score_in[r];
  row.moved = moved[r];
  row.reserved = 0;
  out[r] = row;
}

}  // namespace bpf
