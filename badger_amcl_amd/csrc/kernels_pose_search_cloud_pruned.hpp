// Pruned pose search with the 3-D map and the cloud scanner (bpf_cloud_search_poses_pruned,
// abi_pose_search_cloud_pruned.inl): the rows of bpf_cloud_search_poses, bit for bit, from fewer exact evaluations.
// The structure is the planar one (kernels_pose_search_pruned.hpp), and so are the kernels behind the bound pass:
// k_prune_anchors and the expansion kernels through the rectangle form of SearchSpace / PruneBlocks, k_prune_bounds,
// k_prune_seed_plan, k_prune_survivors and the selection unchanged.  What is new here is the pooled volume P_B
// ("Pose search, pruned 3-D form"), which the BORDER form of k_cloud_score reads in place of
// Map3dDev::dense when it scores an anchor:
//
//   k_pool3_rows   per z plane and grid row y: the sliding minimum along x of the u8 volume, a row segment's window
//                  staged in LDS, into a padded row-major scratch
//   k_pool3_cols   per z plane and 64 x 64 piece of the tiled plane: the sliding minimum along y of that scratch, the
//                  piece's window staged in LDS, written at the entry's place in the 8 x 8-tiled layout
//
// Entry (x, y, k), x and y grid positions (cell - min + 1), is the smallest ratio of the on-map cells of
// W(x) x W(y) in plane k, or border_code when the window holds none.  W(g) = [g - 1, g + B] for g <= span + 1; the
// far border g = span + 2, onto which the kernel's clamp min(c1, span + 2) also sends everything that wraps below grid
// position 0, takes the grid positions within B + 1 of either edge.  No pooling over z.
//
// Between the passes a value travels as one byte in which border_code is above every ratio: border_code is the highest
// code no cell holds, so the codes above it move down by one and 255 is free for it (pool3_in / pool3_out).
#pragma once
#include "kernels_cloud.hpp"
#include "kernels_pose_search_pruned.hpp"

namespace bpf
{

struct Pool3Geom
{
  int w2, h2;      // grid positions in use: 0 .. w + 1 and 0 .. h + 1 (the map's w x h columns and the border ring)
  int ntx, nty;    // 8 x 8 tiles of a plane
  unsigned plane;  // bytes of a plane, ntx * nty * 64
  unsigned border; // Map3dDev::border_code
  int B;
};

__device__ __forceinline__ unsigned pool3_in(unsigned c, unsigned border)
{
  return c == border ? 255u : c - (c > border ? 1u : 0u);
}

__device__ __forceinline__ unsigned pool3_out(unsigned v, unsigned border)
{
  return v == 255u ? border : v + (v >= border ? 1u : 0u);
}

// byte offset of grid position (x, y) inside a plane (Map3dDev)
__device__ __forceinline__ size_t pool3_offset(int x, int y, int ntx)
{
  return ((size_t)(y >> 3) * ntx + (x >> 3)) * 64 + ((x & 7) << 3) + (y & 7);
}

// Pass 1.  blockIdx.y = grid row, blockIdx.z = plane (of the planes `vol` and `R` start at): R(x, y) = min of the
// row's values at x' in W(x).  Positions outside 0 .. w + 1 count as border.
__global__ __launch_bounds__(256) void k_pool3_rows(Pool3Geom G, const uint8_t* __restrict__ vol,
                                                    uint8_t* __restrict__ R)
{
  __shared__ uint8_t s[256 + kPruneMaxBlock + 2];
  const int y = blockIdx.y, x0 = blockIdx.x * 256;
  const uint8_t* pl = vol + (size_t)blockIdx.z * G.plane;
  const int span = 256 + G.B + 2;  // x0 - 1 .. x0 + 256 + B
  for (int t = threadIdx.x; t < span; t += 256)
  {
    const int xx = x0 - 1 + t;
    s[t] = (xx >= 0 && xx < G.w2) ? (uint8_t)pool3_in(pl[pool3_offset(xx, y, G.ntx)], G.border) : (uint8_t)255;
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= G.w2)
    return;
  unsigned m = 255u;
  if (x < G.w2 - 1)
  {
    for (int d = 0; d < G.B + 2; ++d)
      m = min(m, (unsigned)s[threadIdx.x + d]);
  }
  else
  {
    for (int xx = 0; xx <= min(G.B + 1, G.w2 - 1); ++xx)
      m = min(m, pool3_in(pl[pool3_offset(xx, y, G.ntx)], G.border));
    for (int xx = max(0, G.w2 - 2 - G.B); xx < G.w2; ++xx)
      m = min(m, pool3_in(pl[pool3_offset(xx, y, G.ntx)], G.border));
  }
  R[((size_t)blockIdx.z * G.h2 + y) * G.w2 + x] = (uint8_t)m;
}

// Pass 2.  A 64 x 64 piece of the tiled plane blockIdx.z per block: P(x, y) = min of R(x, y') over y' in W(y), decoded;
// what the layout holds beyond the grid positions in use is border_code, as in Map3dDev::dense.
__global__ __launch_bounds__(256) void k_pool3_cols(Pool3Geom G, const uint8_t* __restrict__ R, uint8_t* __restrict__ P)
{
  __shared__ uint8_t s[(64 + kPruneMaxBlock + 2) * 64];
  const int Wt = G.ntx * 8, Ht = G.nty * 8;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
  const uint8_t* Rp = R + (size_t)blockIdx.z * G.h2 * G.w2;
  uint8_t* Pp = P + (size_t)blockIdx.z * G.plane;
  const int rows = 64 + G.B + 2;  // y0 - 1 .. y0 + 64 + B
  for (int t = threadIdx.x; t < rows * 64; t += 256)
  {
    const int yy = y0 - 1 + (t >> 6), xx = x0 + (t & 63);
    s[t] = (yy >= 0 && yy < G.h2 && xx < G.w2) ? Rp[(size_t)yy * G.w2 + xx] : (uint8_t)255;
  }
  __syncthreads();
  const int cx = threadIdx.x & 63, x = x0 + cx;
  for (int rr = threadIdx.x >> 6; rr < 64; rr += 4)
  {
    const int y = y0 + rr;
    if (x >= Wt || y >= Ht)
      continue;
    unsigned m = 255u;
    if (x < G.w2 && y < G.h2 - 1)
    {
      for (int d = 0; d < G.B + 2; ++d)
        m = min(m, (unsigned)s[(rr + d) * 64 + cx]);
    }
    else if (x < G.w2 && y == G.h2 - 1)
    {
      for (int yy = 0; yy <= min(G.B + 1, G.h2 - 1); ++yy)
        m = min(m, (unsigned)Rp[(size_t)yy * G.w2 + x]);
      for (int yy = max(0, G.h2 - 2 - G.B); yy < G.h2; ++yy)
        m = min(m, (unsigned)Rp[(size_t)yy * G.w2 + x]);
    }
    Pp[pool3_offset(x, y, G.ntx)] = (uint8_t)pool3_out(m, G.border);
  }
}

}  // namespace bpf
