// Stand-alone host check of badger_amcl_amd/csrc/shard_rebalance_plan.hpp against a brute-force enumeration of every
// global index: the outgoing counts, the owner and the entry of every sample of every new slice, and the pack order.
// No GPU and no library: g++ -std=c++17 -fsanitize=address,undefined -static-libasan -static-libubsan -I badger_amcl_amd/csrc ... && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "shard_rebalance_plan.hpp"

using bpf::RebalancePlan;

static int failures = 0;

static void fail(const std::vector<long long>& c, const char* what, long long a, long long b)
{
  if (++failures > 10)
    return;
  std::fprintf(stderr, "FAIL %s (%lld vs %lld) for counts [", what, a, b);
  for (long long v : c)
    std::fprintf(stderr, " %lld", v);
  std::fprintf(stderr, " ]\n");
}

static void check(const std::vector<long long>& c)
{
  const int W = (int)c.size();
  RebalancePlan R;
  if (!bpf::rebalance_plan(c.data(), W, &R))
    return fail(c, "plan refused", 0, 0);
  long long G = 0;
  for (long long v : c)
    G += v;
  std::vector<int> old_owner, new_owner;
  std::vector<long long> old_local;
  for (int r = 0; r < W; ++r)
    for (long long i = 0; i < c[r]; ++i)
    {
      old_owner.push_back(r);
      old_local.push_back(i);
    }
  for (int r = 0; r < W; ++r)
  {
    const long long n = (G * (r + 1)) / W - (G * r) / W;
    if (R.Q[r + 1] - R.Q[r] != n)
      fail(c, "new count", R.Q[r + 1] - R.Q[r], n);
    for (long long i = 0; i < n; ++i)
      new_owner.push_back(r);
  }
  if ((long long)new_owner.size() != G)
    return fail(c, "new split does not tile", (long long)new_owner.size(), G);
  // the outgoing lists by enumeration, and every entry's position
  std::vector<std::vector<long long>> out(W);
  std::vector<long long> entry(G, -1);
  for (long long g = 0; g < G; ++g)
    if (old_owner[g] != new_owner[g])
    {
      entry[g] = (long long)out[old_owner[g]].size();
      out[old_owner[g]].push_back(g);
    }
  long long T = 0;
  for (int r = 0; r < W; ++r)
  {
    if (R.out[r] != (long long)out[r].size())
      fail(c, "out count", R.out[r], (long long)out[r].size());
    T += (long long)out[r].size();
    // the pack order: entry i of rank r's list is its local sample rebalance_out_local(i)
    const long long head = R.keep_lo[r] - R.P[r];
    for (long long i = 0; i < (long long)out[r].size() && i < R.out[r]; ++i)
    {
      const long long l = bpf::rebalance_out_local(i, head, R.keep_n[r]);
      if (l < 0 || l >= c[r] || R.P[r] + l != out[r][i])
        fail(c, "pack order", R.P[r] + l, out[r][i]);
    }
  }
  if (R.moved != T)
    fail(c, "moved", R.moved, T);
  for (long long g = 0; g < G; ++g)
  {
    const int q = bpf::rebalance_owner(R.P, W, g);
    if (q != old_owner[g])
    {
      fail(c, "owner", q, old_owner[g]);
      continue;
    }
    if (q == new_owner[g])
    {
      if (g < R.keep_lo[q] || g >= R.keep_lo[q] + R.keep_n[q])
        fail(c, "a sample that stays lies outside the kept range", g, R.keep_lo[q]);
      if (g - R.P[q] != old_local[g])
        fail(c, "local index", g - R.P[q], old_local[g]);
    }
    else
    {
      const long long j = bpf::rebalance_out_entry(g, R.P[q], R.keep_lo[q], R.keep_n[q]);
      if (j != entry[g])
        fail(c, "entry", j, entry[g]);
    }
  }
}

int main()
{
  const std::vector<std::vector<long long>> named = {
    { 1, 1, 1, 497, 1, 399, 299, 1 }, { 1, 1198, 1 }, { 0, 1200, 0 }, { 0, 0, 2, 298, 0, 300, 1, 598, 1 }, { 1200 },
    { 150, 150, 150, 150, 150, 150, 150, 150 }, { 5, 0, 0, 0, 0, 0, 0, 0 }, { 0, 0, 0, 0, 0, 0, 0, 3 },
    { 1, 69999 }, { 0 }, { 0, 0, 0 },
  };
  for (const auto& c : named)
    check(c);
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto next = [&s]() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  };
  int n_random = 0;
  for (int k = 0; k < 3000; ++k)
  {
    const int W = 1 + (int)(next() % 16);
    std::vector<long long> c(W);
    const int shape = (int)(next() % 3);
    for (int r = 0; r < W; ++r)
    {
      c[r] = (long long)(next() % (shape == 0 ? 8 : 200));
      if (shape == 2 && next() % 3 == 0)
        c[r] = 0;
    }
    check(c);
    ++n_random;
  }
  // refusals
  RebalancePlan R;
  const long long neg[2] = { 3, -1 };
  std::vector<long long> many(17, 1);
  if (bpf::rebalance_plan(neg, 2, &R) || bpf::rebalance_plan(many.data(), 17, &R) || bpf::rebalance_plan(neg, 0, &R))
    fail({ 3, -1 }, "a bad argument was accepted", 0, 0);
  std::printf("checked %d named and %d random count vectors: %d failures\n", (int)named.size(), n_random, failures);
  return failures ? 1 : 0;
}
