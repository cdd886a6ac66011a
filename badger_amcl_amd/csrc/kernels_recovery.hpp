// Augmented-MCL recovery draws of resampleMultinomial (particle_filter.cpp:383-400, w_diff > 0):
//
//     if (drand48() < w_diff)  pose = random_pose_fn_();          // Node::randomFreeSpacePose: 2 more draws
//     else                   { r = drand48(); ... CDF search }    // 1 more draw
//
// Every candidate draw starts with a test on the next stream element and then consumes 2 or 1 further
// elements, so where draw m finds its elements depends on the outcome of every earlier test -- a pointer chase
// through the stream (next(q) = q + 3 or q + 2).  It is resolved in three passes over fixed segments of the
// stream: per segment and per possible entry offset (0, 1, 2) the number of draws that start inside it and the
// offset at which the walk leaves it; a scan that composes those little maps gives every segment its real
// entry offset and first draw index; a last pass walks each segment once more and records, per draw, the
// stream element it reads first (its test element + 1) and whether it is a random pose.
//
// With Node::uniformPoseGenerator's score check active every random pose call rejects `retries` = K trials first
// (include/badger_pf.h, bpf_pf_set_uniform_pose_check): a random draw consumes 2 K + 3 elements and takes its pose
// from its accepted trial, test + 1 + 2 K.  That jump does not fit the three entry offsets of the segment scheme;
// k_chain_chase resolves the chain for K > 0 in one wavefront instead: 64 lanes test the next 64 positions of the
// current parity class at once (a jump of 2 keeps the class), the first hit ends a run of plain draws, and the
// state jumps 2 K + 3 elements past the random draw's test.  One trip per random draw or per 64 plain draws, each
// an affine map, a ballot and a shuffle; the trip count is bounded by the number of draws.
#pragma once
#include "device_types.hpp"
#include "kernels_pf.hpp"

namespace bpf
{

constexpr int kChainSeg = 128;  // stream positions per segment

struct ChainArgs
{
  uint64_t rng_state;  // drand48 state before the resample; stream position q (1-based) = q steps from it
  double w_diff;
  int n_seg;
  int max_draws;       // chain[] is filled for draws 0 .. max_draws (inclusive: where the stream would go on)
  uint64_t* seg_bits;  // [n_seg][2] outcome bit per position (1: r < w_diff)
  int* seg_cnt;        // [n_seg][3] draws that start in the segment, per entry offset
  int* seg_exit;       // [n_seg][3] offset into the next segment at which the walk leaves, per entry offset
  int* seg_entry;      // [n_seg] real entry offset
  int* seg_base;       // [n_seg] index of the first draw that starts in the segment
  int* chain;          // [max_draws + 1] stream element draw m reads first, bit 31 = random pose
  int retries;         // k_chain_chase: rejected trials per random pose call (K > 0)
  LcgJump jump;
};

__device__ __forceinline__ bool chain_bit(const uint64_t b[2], int pos)
{
  return (b[pos >> 6] >> (pos & 63)) & 1ull;
}

__global__ void k_chain_segments(const ChainArgs A)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= A.n_seg)
    return;
  // outcomes of the tests at positions 1 + s*S + [0, S)
  uint64_t x = lcg_skip(A.rng_state, (uint64_t)s * kChainSeg + 1, A.jump);
  uint64_t b[2] = { 0, 0 };
  for (int p = 0; p < kChainSeg; ++p)
  {
    if (ldexp((double)x, -48) < A.w_diff)
      b[p >> 6] |= 1ull << (p & 63);
    x = lcg_next(x);
  }
  A.seg_bits[2 * (size_t)s] = b[0];
  A.seg_bits[2 * (size_t)s + 1] = b[1];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    int pos = a, cnt = 0;
    while (pos < kChainSeg)
    {
      ++cnt;
      pos += chain_bit(b, pos) ? 3 : 2;
    }
    A.seg_cnt[3 * (size_t)s + a] = cnt;
    A.seg_exit[3 * (size_t)s + a] = pos - kChainSeg;
  }
}

// a map {0,1,2} -> (draws, exit offset); (f then g)[a] = (f.cnt[a] + g.cnt[f.exit[a]], g.exit[f.exit[a]])
struct ChainMap
{
  int cnt[3];
  int exit[3];
};

__device__ __forceinline__ ChainMap chain_compose(const ChainMap& f, const ChainMap& g)
{
  ChainMap h;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    const int e = f.exit[a];
    h.cnt[a] = f.cnt[a] + g.cnt[e];
    h.exit[a] = g.exit[e];
  }
  return h;
}

__global__ __launch_bounds__(1024) void k_chain_scan(const ChainArgs A)
{
  __shared__ ChainMap s_map[1024];
  const int tid = threadIdx.x;
  const int per = (A.n_seg + 1023) / 1024;
  const int lo = min(tid * per, A.n_seg), hi = min(lo + per, A.n_seg);
  ChainMap mine;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    mine.cnt[a] = 0;
    mine.exit[a] = a;  // identity
  }
  for (int s = lo; s < hi; ++s)
  {
    ChainMap g;
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      g.cnt[a] = A.seg_cnt[3 * (size_t)s + a];
      g.exit[a] = A.seg_exit[3 * (size_t)s + a];
    }
    mine = chain_compose(mine, g);
  }
  s_map[tid] = mine;
  __syncthreads();
  // inclusive scan under composition (order matters: earlier chunks first)
  for (int o = 1; o < 1024; o <<= 1)
  {
    ChainMap left;
    const bool have = tid >= o;
    if (have)
      left = s_map[tid - o];
    __syncthreads();
    if (have)
      s_map[tid] = chain_compose(left, s_map[tid]);
    __syncthreads();
  }
  // the walk enters the first segment at offset 0 with draw 0; this thread's chunk starts where the
  // composition of all earlier chunks leaves it
  int entry = 0, base = 0;
  if (tid > 0)
  {
    entry = s_map[tid - 1].exit[0];
    base = s_map[tid - 1].cnt[0];
  }
  for (int s = lo; s < hi; ++s)
  {
    A.seg_entry[s] = entry;
    A.seg_base[s] = base;
    base += A.seg_cnt[3 * (size_t)s + entry];
    entry = A.seg_exit[3 * (size_t)s + entry];
  }
}

__global__ void k_chain_emit(const ChainArgs A)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= A.n_seg)
    return;
  const uint64_t b[2] = { A.seg_bits[2 * (size_t)s], A.seg_bits[2 * (size_t)s + 1] };
  int pos = A.seg_entry[s], m = A.seg_base[s];
  while (pos < kChainSeg && m <= A.max_draws)
  {
    const bool random = chain_bit(b, pos);
    A.chain[m] = (int)((unsigned)(s * kChainSeg + pos + 2) | (random ? 0x80000000u : 0u));
    ++m;
    pos += random ? 3 : 2;
  }
}

// the LCG advanced by k elements as one affine map x -> a x + c (mod 2^48)
__device__ __forceinline__ void lcg_affine(uint64_t k, const LcgJump& J, uint64_t* a_out, uint64_t* c_out)
{
  const uint64_t mask = (1ull << 48) - 1;
  uint64_t a = 1, c = 0;
  for (int j = 0; k != 0 && j < 48; ++j, k >>= 1)
    if (k & 1)
    {
      a = (a * J.A[j]) & mask;
      c = (c * J.A[j] + J.C[j]) & mask;
    }
  *a_out = a;
  *c_out = c;
}

// one wavefront (blockDim 64); the host has checked that (2 K + 3)(max_draws + 1) + 3 positions fit 31 bits
__global__ __launch_bounds__(64) void k_chain_chase(const ChainArgs A)
{
  const uint64_t mask = (1ull << 48) - 1;
  const int lane = threadIdx.x;
  const unsigned jump_len = 2u * (unsigned)A.retries + 3u;
  uint64_t a_l, c_l, a_j, c_j, a_2, c_2;
  lcg_affine(2ull * (uint64_t)lane, A.jump, &a_l, &c_l);  // test position q -> q + 2 lane
  lcg_affine((uint64_t)jump_len, A.jump, &a_j, &c_j);     // random draw's test -> the next test
  lcg_affine(2ull, A.jump, &a_2, &c_2);
  uint64_t xq = lcg_skip(A.rng_state, 1ull, A.jump);  // element q, the current test
  unsigned q = 1;  // (< 2^31 while draws remain; the last trip may step past it)
  int m = 0;
  while (m <= A.max_draws)
  {
    const uint64_t x = (a_l * xq + c_l) & mask;  // element q + 2 lane
    const bool hit = ldexp((double)x, -48) < A.w_diff;
    const unsigned long long hits = __ballot(hit);
    const int f = hits ? __builtin_ctzll(hits) : 64;  // plain draws before the first random one
    if (lane < f && m + lane <= A.max_draws)
      A.chain[m + lane] = (int)(q + 2u * (unsigned)lane + 1u);
    const uint64_t x_end = __shfl(x, f < 64 ? f : 63);
    m += f;
    if (f < 64)
    {
      q += 2u * (unsigned)f;
      if (lane == 0 && m <= A.max_draws)
        A.chain[m] = (int)((q + 1u + 2u * (unsigned)A.retries) | 0x80000000u);
      ++m;
      q += jump_len;
      xq = (a_j * x_end + c_j) & mask;
    }
    else
    {
      q += 128u;
      xq = (a_2 * x_end + c_2) & mask;
    }
  }
}

// BPF_POSE_CHECK_SENSOR_MODEL: the trial poses at stream elements first + stride t, t < n, as a one-sample-set each
// (weight 1.0) for the planar scoring kernels
__global__ void k_candidate_poses(ParticlesDev dst, int n, unsigned first, unsigned stride, uint64_t rng_state,
                                  LcgJump jump, FreeSpaceDev F)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  const uint64_t xs = lcg_skip(rng_state, (uint64_t)first + (uint64_t)stride * (uint64_t)t, jump);
  double x, y, th;
  random_free_space_pose(F, ldexp((double)xs, -48), ldexp((double)lcg_next(xs), -48), &x, &y, &th);
  dst.x[t] = x;
  dst.y[t] = y;
  dst.th[t] = th;
  dst.w[t] = 1.0;
}

}  // namespace bpf
