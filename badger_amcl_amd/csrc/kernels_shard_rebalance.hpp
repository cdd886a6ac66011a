// Rebalancing a SHARDED set: the slices go back to the even split in global order, and only the samples that sit on
// the wrong rank move (shard_rebalance_plan.hpp has the plan: a pure function of the W local counts).
//
//   k_rebalance_pack       one thread per OUTGOING sample of this rank: x, y, theta, w of the head and tail spans of the
//                          current set into a staging block int64[4][out], as bit patterns
//   -- exchange: ragged all-gather of the staging blocks (4 words per moved sample) --
//   k_rebalance_assemble   one thread per sample of the NEW slice: global index g = Q[rank] + o; the owner q of g under
//                          the old split; from the current set when q is this rank, else entry j of rank q's gathered
//                          rows; written into the set that is NOT current
//
// The bits are copied, never recomputed.  No atomics, and no kernel here waits for another rank: the exchange sits
// between the two launches.
#pragma once
#include "device_types.hpp"
#include "shard_rebalance_plan.hpp"

namespace bpf
{

struct RebalancePackArgs
{
  ParticlesDev src;    // the current set
  long long head;      // outgoing samples below the kept range: local [0, head)
  long long keep_n;    // kept samples: local [head, head + keep_n); the tail span follows
  long long n_out;     // head + tail
  long long* rows;     // int64[4][n_out]
};

__global__ __launch_bounds__(256) void k_rebalance_pack(const RebalancePackArgs A)
{
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n_out; i += (long long)gridDim.x * 256)
  {
    const long long l = rebalance_out_local(i, A.head, A.keep_n);
    A.rows[i] = __double_as_longlong(A.src.x[l]);
    A.rows[A.n_out + i] = __double_as_longlong(A.src.y[l]);
    A.rows[2 * A.n_out + i] = __double_as_longlong(A.src.th[l]);
    A.rows[3 * A.n_out + i] = __double_as_longlong(A.src.w[l]);
  }
}

// By value, like MbRagged: the plan's fields are scalar operands.  g is per lane, so the owner search below is a chain of
// vector compares against them and the selected prefix, kept range and offset are per-lane values; the lanes of a wave
// agree except where a span border falls inside it.
struct RebalanceAssembleArgs
{
  int world, rank;
  long long n_new;                          // Q[rank + 1] - Q[rank]
  long long q_first;                        // Q[rank]
  long long P[kRebalanceMaxWorld + 1];      // old prefix
  long long keep_lo[kRebalanceMaxWorld];    // every rank's kept range
  long long keep_n[kRebalanceMaxWorld];
  long long rank_off[kRebalanceMaxWorld];   // rank q's row k of the gathered rows starts at rank_off[q] + k * row_stride
  long long row_stride;
  const long long* rows;                    // the gathered rows (null when nothing moved into this rank)
  ParticlesDev src, dst;                    // the current set, the set that is not current
};

__global__ __launch_bounds__(256) void k_rebalance_assemble(const RebalanceAssembleArgs A)
{
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= A.n_new)
    return;
  const long long g = A.q_first + o;
  // rebalance_owner, with what belongs to the owner selected along the way
  int q = 0;
  long long p_q = A.P[0], lo = A.keep_lo[0], kn = A.keep_n[0], off = A.rank_off[0];
#pragma unroll
  for (int r = 1; r < kRebalanceMaxWorld; ++r)
  {
    const bool at = r < A.world && g >= A.P[r];
    q = at ? r : q;
    p_q = at ? A.P[r] : p_q;
    lo = at ? A.keep_lo[r] : lo;
    kn = at ? A.keep_n[r] : kn;
    off = at ? A.rank_off[r] : off;
  }
  long long x, y, th, w;
  if (q == A.rank)
  {
    const long long l = g - p_q;
    x = __double_as_longlong(A.src.x[l]);
    y = __double_as_longlong(A.src.y[l]);
    th = __double_as_longlong(A.src.th[l]);
    w = __double_as_longlong(A.src.w[l]);
  }
  else
  {
    const long long* row = A.rows + off + rebalance_out_entry(g, p_q, lo, kn);
    x = row[0];
    y = row[A.row_stride];
    th = row[2 * A.row_stride];
    w = row[3 * A.row_stride];
  }
  A.dst.x[o] = __longlong_as_double(x);
  A.dst.y[o] = __longlong_as_double(y);
  A.dst.th[o] = __longlong_as_double(th);
  A.dst.w[o] = __longlong_as_double(w);
}

}  // namespace bpf
