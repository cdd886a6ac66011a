// Exchange between the engines of ONE process ("local world", abi_shard_local.inl).
//
// All ranks of the sharded filter live in one address space, so a rank can read its peers' send buffers directly: both
// kernels PULL.  Each rank's launch reads the W published send spans and writes only its own destination, so no rank
// ever stores into memory another rank's stream is working on, and the ordering that remains -- "the peers' send data
// is complete" before, "the peers have finished reading my send buffer" after -- is carried by events between the
// streams (hipStreamWaitEvent), never by a kernel that waits: sibling streams may share a hardware queue, and a
// consumer spinning for a producer queued behind it would stall until its time-out.
//
// Both kernels take their table of <= 16 spans by value (kernel arguments: the loop over the ranks is wave-uniform, so
// the entries come in by scalar loads), run in blocks of 256 with a grid stride, and move 16 bytes per lane wherever
// source and destination allow it, with a scalar head up to the destination's 16-byte boundary and a scalar tail.
#pragma once
#include "kernels_mailbox.hpp"

namespace bpf
{

// ragged all-gather of 8-byte words (int64, or the bits of f64): rank r's `count[r]` words at src[r] go to
// dst[dst_off[r] ...]; count[r] == 0 (an empty shard) is legal and src[r] is then never dereferenced
struct LxGather
{
  int world;
  const long long* src[kMailboxMaxWorld];
  long long count[kMailboxMaxWorld];
  long long dst_off[kMailboxMaxWorld];
};

__global__ void __launch_bounds__(256) k_local_gather_words(const LxGather T, long long* __restrict__ dst)
{
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (int r = 0; r < T.world; ++r)
  {
    const long long n = T.count[r];
    if (n <= 0)
      continue;
    const long long* __restrict__ s = T.src[r];
    long long* __restrict__ d = dst + T.dst_off[r];
    // one word of head brings the destination to 16 bytes; the body is wide when the source is aligned there too
    const long long head = ((reinterpret_cast<uintptr_t>(d) & 15u) != 0) ? 1 : 0;
    const bool wide = n > head && (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0;
    if (!wide)
    {
      for (long long i = tid; i < n; i += step)
        d[i] = s[i];
      continue;
    }
    const long long pairs = (n - head) / 2;
    const longlong2* __restrict__ s2 = reinterpret_cast<const longlong2*>(s + head);
    longlong2* __restrict__ d2 = reinterpret_cast<longlong2*>(d + head);
    for (long long i = tid; i < pairs; i += step)
      d2[i] = s2[i];
    if (tid == 0 && head)
      d[0] = s[0];
    if (tid == 1 && head + 2 * pairs < n)
      d[n - 1] = s[n - 1];
  }
}

// all-reduce(sum): dst[i] = src[0][i] + src[1][i] + ... in RANK ORDER (every rank adds in the same order and so ends
// with the same bits), n int64 words, or n int32 words widened to int64 for the sum as k_mailbox_take_sum has them.
// dst is this rank's own buffer; src[r] are the ranks' staged copies (this rank's included), never dst itself.
struct LxReduce
{
  int world;
  const void* src[kMailboxMaxWorld];
  long long n;
};

__global__ void __launch_bounds__(256) k_local_reduce_sum_i64(const LxReduce T, long long* __restrict__ dst)
{
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long n = T.n;
  const long long head = std::min<long long>(n, (reinterpret_cast<uintptr_t>(dst) & 15u) ? 1 : 0);
  bool wide = n - head >= 2;
  for (int r = 0; r < T.world; ++r)
    wide = wide && (reinterpret_cast<uintptr_t>(static_cast<const long long*>(T.src[r]) + head) & 15u) == 0;
  if (!wide)
  {
    for (long long i = tid; i < n; i += step)
    {
      long long acc = 0;
      for (int r = 0; r < T.world; ++r)
        acc += static_cast<const long long*>(T.src[r])[i];
      dst[i] = acc;
    }
    return;
  }
  const long long pairs = (n - head) / 2;
  longlong2* __restrict__ d2 = reinterpret_cast<longlong2*>(dst + head);
  for (long long i = tid; i < pairs; i += step)
  {
    longlong2 acc = make_longlong2(0, 0);
    for (int r = 0; r < T.world; ++r)
    {
      const longlong2 v = reinterpret_cast<const longlong2*>(static_cast<const long long*>(T.src[r]) + head)[i];
      acc.x += v.x;
      acc.y += v.y;
    }
    d2[i] = acc;
  }
  // head and tail: at most one word each
  const long long tail = head + 2 * pairs;
  const long long at = tid == 0 ? (head ? 0 : -1) : (tid == 1 ? (tail < n ? tail : -1) : -1);
  if (at >= 0)
  {
    long long acc = 0;
    for (int r = 0; r < T.world; ++r)
      acc += static_cast<const long long*>(T.src[r])[at];
    dst[at] = acc;
  }
}

__global__ void __launch_bounds__(256) k_local_reduce_sum_i32(const LxReduce T, int* __restrict__ dst)
{
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long step = (long long)gridDim.x * blockDim.x;
  const long long n = T.n;
  // words up to the destination's 16-byte boundary (0 .. 3)
  const long long head = std::min<long long>(n, (long long)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4);
  bool wide = n - head >= 4;
  for (int r = 0; r < T.world; ++r)
    wide = wide && (reinterpret_cast<uintptr_t>(static_cast<const int*>(T.src[r]) + head) & 15u) == 0;
  auto one = [&](long long i) {
    long long acc = 0;
    for (int r = 0; r < T.world; ++r)
      acc += (long long)static_cast<const int*>(T.src[r])[i];
    dst[i] = (int)acc;
  };
  if (!wide)
  {
    for (long long i = tid; i < n; i += step)
      one(i);
    return;
  }
  const long long quads = (n - head) / 4;
  int4* __restrict__ d4 = reinterpret_cast<int4*>(dst + head);
  for (long long i = tid; i < quads; i += step)
  {
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int r = 0; r < T.world; ++r)
    {
      const int4 v = reinterpret_cast<const int4*>(static_cast<const int*>(T.src[r]) + head)[i];
      a0 += v.x;
      a1 += v.y;
      a2 += v.z;
      a3 += v.w;
    }
    d4[i] = make_int4((int)a0, (int)a1, (int)a2, (int)a3);
  }
  // head (<= 3 words) and tail (<= 3 words) by the first lanes
  const long long tail = head + 4 * quads;
  if (tid < head)
    one(tid);
  else if (tid < head + (n - tail))
    one(tail + (tid - head));
}

}  // namespace bpf
