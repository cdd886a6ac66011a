// The particle-cloud message (Node::publishParticleCloud, node.cpp:335-357) formed on the device: PoseArray entries
// {x, y, 0, qx, qy, qz, qw} with q = setRPY(0, 0, theta) = (0, 0, sin(theta / 2), cos(theta / 2)) -- the layout and the
// arithmetic of bpf_wire_samples_to_pose_array (abi_wire.inl) -- and the rows a shard contributes to it.
#pragma once
#include "device_types.hpp"

namespace bpf
{

constexpr int kPoseBlock = 256;  // poses per block of k_pose_array: 256 x 7 doubles = 14 KB of LDS

// Pose k = sample i0 + k * stride of an SoA source, k = 0 .. count - 1.  The source is the resident set, or gathered
// rows int64[3][n] seen as doubles (x = rows, y = rows + row_stride, th = rows + 2 * row_stride; i0 = 0, stride = 1).
//
// 24 B in and 56 B out per pose: the store side is the cost.  Seven 8-byte stores per lane, 56 B apart, would touch
// every output line seven times from one wave, so a block stages its poses in LDS (lane t writes doubles 7t .. 7t+6:
// 8-byte LDS stores go in groups of 16 lanes over 32 banks, and 14 t mod 32 puts the 16 lanes of a group on 16
// different even banks, so the stores are conflict-free) and then streams the tile out in address order, 16 B per
// lane: a wave's store covers 1 KB of consecutive addresses.
__global__ __launch_bounds__(kPoseBlock) void k_pose_array(const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ th, long long i0,
                                                           long long stride, int count, double* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) double s_tile[kPoseBlock * 7];
  const long long k0 = (long long)blockIdx.x * kPoseBlock;
  const long long k = k0 + threadIdx.x;
  if (k < count)
  {
    const long long i = i0 + k * stride;
    double s, c;
    sincos(th[i] * 0.5, &s, &c);  // theta * 0.5 is exact
    double* o = s_tile + 7 * threadIdx.x;
    o[0] = x[i];
    o[1] = y[i];
    o[2] = 0.0;
    o[3] = 0.0;
    o[4] = 0.0;
    o[5] = s;
    o[6] = c;
  }
  __syncthreads();
  const long long left = (long long)count - k0;
  const int m = 7 * (int)(left < kPoseBlock ? left : kPoseBlock);  // doubles of this tile
  // k0 * 56 B is a multiple of 16 B (k0 is a multiple of 256), so the tile starts 16-byte aligned wherever out does
  double* o = out + (size_t)k0 * 7;
  const double2* s2 = reinterpret_cast<const double2*>(s_tile);
  double2* o2 = reinterpret_cast<double2*>(o);
  for (int j = threadIdx.x; j < m / 2; j += kPoseBlock)
    o2[j] = s2[j];
  if ((m & 1) && threadIdx.x == 0)
    o[m - 1] = s_tile[m - 1];
}

// A shard's contribution: the bit patterns of x / y / theta of its selected samples as int64[3][n_sel] (row stride
// n_sel), in index order.  The selection is arithmetic -- with g = global_first + i, sample i is selected iff
// g >= first and (g - first) % stride == 0 -- so the host hands over the first selected local index and the count.
__global__ void k_pose_rows(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ th,
                            long long i0, long long stride, int n_sel, long long* __restrict__ rows)
{
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_sel)
    return;
  const long long i = i0 + k * stride;
  rows[k] = __double_as_longlong(x[i]);
  rows[(size_t)n_sel + k] = __double_as_longlong(y[i]);
  rows[2 * (size_t)n_sel + k] = __double_as_longlong(th[i]);
}

}  // namespace bpf
