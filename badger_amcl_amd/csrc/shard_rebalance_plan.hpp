// The plan of a rebalance of a sharded set (kernels_shard_rebalance.hpp, abi_shard_rebalance.inl): the slices go back
// to the even split in GLOBAL order, and only the samples that sit on the wrong rank move.  With contiguous shards the
// plan is a pure function of the W local counts, so every rank derives the same one with no exchange.
//
//   old prefix  P[r] = counts[0] + ... + counts[r - 1]              rank r holds global [P[r], P[r + 1])
//   new prefix  Q[r] = (G r) / W, G = P[W]                          rank r will hold    [Q[r], Q[r + 1])
//   kept        [max(P[r], Q[r]), min(P[r + 1], Q[r + 1])), or the empty range at P[r]
//   outgoing    the rest of the old slice in ascending global index: a head span, then a tail span
//
// Host code only: no HIP include, so that a stand-alone host program can compile it.  The two look-ups carry
// BPF_RB_HD, which is __host__ __device__ under hipcc: the assemble kernel runs the functions the host tests check.
#pragma once

#if defined(__HIPCC__)
#define BPF_RB_HD __host__ __device__
#else
#define BPF_RB_HD
#endif

namespace bpf
{

constexpr int kRebalanceMaxWorld = 16;  // kMailboxMaxWorld

struct RebalancePlan
{
  int world = 0;
  long long P[kRebalanceMaxWorld + 1] = { 0 };   // old prefix
  long long Q[kRebalanceMaxWorld + 1] = { 0 };   // new prefix (the even split)
  long long keep_lo[kRebalanceMaxWorld] = { 0 }; // first global index rank r keeps (P[r] when it keeps nothing)
  long long keep_n[kRebalanceMaxWorld] = { 0 };  //   and how many
  long long out[kRebalanceMaxWorld] = { 0 };     // samples rank r sends: counts[r] - keep_n[r]
  long long moved = 0;                           // T = sum(out); 0: the split is even already
};

// false: world outside 1 .. 16 or a negative count (nothing was written)
inline bool rebalance_plan(const long long* counts, int world, RebalancePlan* R)
{
  if (!counts || !R || world < 1 || world > kRebalanceMaxWorld)
    return false;
  for (int r = 0; r < world; ++r)
    if (counts[r] < 0)
      return false;
  *R = RebalancePlan{};
  R->world = world;
  for (int r = 0; r < world; ++r)
    R->P[r + 1] = R->P[r] + counts[r];
  const long long G = R->P[world];
  for (int r = 0; r <= world; ++r)
    R->Q[r] = (G * r) / world;
  for (int r = 0; r < world; ++r)
  {
    const long long lo = R->P[r] > R->Q[r] ? R->P[r] : R->Q[r];
    const long long hi = R->P[r + 1] < R->Q[r + 1] ? R->P[r + 1] : R->Q[r + 1];
    R->keep_lo[r] = hi > lo ? lo : R->P[r];
    R->keep_n[r] = hi > lo ? hi - lo : 0;
    R->out[r] = counts[r] - R->keep_n[r];
    R->moved += R->out[r];
  }
  return true;
}

// the rank q with P[q] <= g < P[q + 1]: the last one whose prefix does not exceed g (empty ranks share a prefix with
// their successor and are passed over)
BPF_RB_HD inline int rebalance_owner(const long long* P, int world, long long g)
{
  int q = 0;
  for (int r = 1; r < world; ++r)
    q = g >= P[r] ? r : q;
  return q;
}

// position of global index g, which its owner does NOT keep, in the owner's outgoing list: the head span lies below
// the kept range [keep_lo, keep_lo + keep_n), the tail span above it
BPF_RB_HD inline long long rebalance_out_entry(long long g, long long p_owner, long long keep_lo, long long keep_n)
{
  return g < keep_lo ? g - p_owner : g - p_owner - keep_n;
}

// local index (in the old slice) of entry i of a rank's outgoing list; head = keep_lo - P[rank]
BPF_RB_HD inline long long rebalance_out_local(long long i, long long head, long long keep_n)
{
  return i < head ? i : i + keep_n;
}

}  // namespace bpf
