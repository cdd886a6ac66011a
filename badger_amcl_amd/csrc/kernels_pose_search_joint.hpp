// Joint pose search (bpf_planar_search_poses_joint, bpf_cloud_search_poses_joint, abi_pose_search_joint.inl): every
// candidate of the exhaustive search scored against S scans, scan s taken at the candidate's base pose composed with a
// rigid offset D_s = (dx, dy, dth), the weight carried from scan to scan.  One kernel of its own:
//
//   k_search_compose   one window of composed poses into the engine's candidate set (one lane per candidate)
//
// The composition is coordAdd's (planar_scanner.cpp:693-701), left to right and without contraction:
//   x_s = (x + dx * C_h) - dy * S_h,  y_s = (y + dx * S_h) + dy * C_h,  th_s = th_h + dth   (not normalised)
// C_h = cos(th_h) and S_h = sin(th_h) are NOT evaluated here: they come from a table of H entries that the host fills
// with the C library's cos / sin (bpf_pose_search_heading_table), so that a composed pose is bit for bit what a host
// model computes.  Candidate c has heading c mod H, and c varies fastest across lanes: a wave reads at most two
// contiguous runs of either table.  For the first scan the kernel also writes w = 1.0; for the later ones it leaves
// w alone, and the scoring path multiplies the carried weight in place.
// This is the only place the composition is written: the diagnostic calls (bpf_*_search_joint_poses) launch the same
// kernel with a list of candidates in place of the window's first.
#pragma once
#include "kernels_pose_search.hpp"

namespace bpf
{

constexpr int kSearchJointMaxScans = 16;
constexpr int kSearchJointMaxHeadings = 65536;

// slot t holds candidate ids[t] (ids != nullptr: uniform over the launch) or c0 + t
__global__ __launch_bounds__(256) void k_search_compose(ParticlesDev dst, int n, long long c0,
                                                         const long long* __restrict__ ids, SearchSpace S,
                                                         const double* __restrict__ cos_h,
                                                         const double* __restrict__ sin_h, double dx, double dy,
                                                         double dth, int first_scan)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  int i, j, h;
  double x, y, th;
  search_pose_of(S, ids != nullptr ? ids[t] : c0 + (long long)t, &i, &j, &h, &x, &y, &th);
  const double c = cos_h[h], s = sin_h[h];
  dst.x[t] = (x + dx * c) - dy * s;
  dst.y[t] = (y + dx * s) + dy * c;
  dst.th[t] = th + dth;
  if (first_scan)
    dst.w[t] = 1.0;
}

}  // namespace bpf
