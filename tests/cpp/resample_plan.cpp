// Stand-alone host check of badger_amcl_amd/csrc/resample_plan.hpp against the arithmetic the two resample drivers
// carried inline before they shared it, transcribed here as it stood: the multinomial window schedule of the single
// engine and of the sharded driver (which never hands the stream to the device tree before a first host window), the
// systematic budget, the stream account and the target chain.  Every value must be equal.
// No GPU and no library: g++ -std=c++17 -I badger_amcl_amd/csrc tests/cpp/resample_plan.cpp && ./a.out
// (with -fsanitize=address,undefined -static-libasan -static-libubsan for a watched run).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "resample_plan.hpp"

static long long failures = 0, checks = 0;

static void expect(bool ok, const char* what, long long a, long long b, long long c, long long d)
{
  ++checks;
  if (!ok && ++failures <= 10)
    std::fprintf(stderr, "FAIL %s (%lld %lld %lld %lld)\n", what, a, b, c, d);
}

// ---- the window schedule: the trace of a stream that never stops, (kind, m0, m1) per step
struct Step
{
  int device, m0, m1;
  bool operator==(const Step& o) const { return device == o.device && m0 == o.m0 && m1 == o.m1; }
};
using Trace = std::vector<Step>;

static int old_window_for(int x)
{
  return std::max(1024, (x + x / 4 + 1023) / 1024 * 1024);
}

// limits[k]: the bound for the leaves seen after the k-th host window; device_ok: the device tree takes the stream
static Trace old_single(int hint, int maxs, int device_min, const std::vector<int>& limits, bool device_ok)
{
  Trace t;
  int m0 = 0, k = 0, replay_limit = 0;
  int window = std::max(1024, std::min(hint, maxs));
  bool device_declined = false;
  if (window > 4096 && maxs - 4096 >= device_min)
    window = 4096;
  while (m0 < maxs)
  {
    const int m1 = std::min(maxs, m0 + window);
    const bool long_stream = (m0 > 0 ? replay_limit - m0 >= device_min : hint >= maxs) && maxs - m0 >= device_min;
    if (long_stream && !device_declined)
    {
      t.push_back({ 1, m0, maxs });
      if (device_ok)
        break;
      device_declined = true;
    }
    t.push_back({ 0, m0, m1 });
    replay_limit = limits[k++ % limits.size()];
    m0 = m1;
    const int need = replay_limit - m0;
    window = old_window_for(need);
  }
  return t;
}

static Trace old_sharded(int hint, int max_global, int device_min, const std::vector<int>& limits, bool device_ok)
{
  Trace t;
  int m0 = 0, need = 0, k = 0;
  int win = std::max(1024, std::min(hint, max_global));
  bool device_declined = false;
  if (win > 4096 && max_global - 4096 >= device_min)
    win = 4096;
  while (m0 < max_global)
  {
    if (m0 > 0 && !device_declined && max_global - m0 >= device_min && need >= device_min)
    {
      t.push_back({ 1, m0, max_global });
      if (device_ok)
        break;
      device_declined = true;
    }
    const int m1 = std::min(max_global, m0 + win);
    t.push_back({ 0, m0, m1 });
    m0 = m1;
    const int lim = limits[k++ % limits.size()];
    need = lim - m0;
    win = old_window_for(need);
  }
  return t;
}

static Trace shared(int hint, int maxs, int device_min, const std::vector<int>& limits, bool device_ok, bool at_start)
{
  Trace t;
  bpf::WindowSchedule s = bpf::window_schedule(hint, maxs, device_min, at_start);
  int limit = 0, k = 0;
  while (s.m0 < maxs)
  {
    if (s.whole_stream_due(limit))
    {
      t.push_back({ 1, s.m0, maxs });
      if (device_ok)
        break;
      s.device_declined = true;
    }
    t.push_back({ 0, s.m0, s.m1() });
    limit = limits[k++ % limits.size()];
    s.next(limit);
  }
  return t;
}

static void check_schedule()
{
  const int hints[] = { 0, 1, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 5120, 8192, 20480, 100000, 1 << 30 };
  const int maxes[] = { 1, 100, 1024, 2000, 3000, 4096, 4097, 5000, 6000, 8191, 8192, 12288, 12289, 20000, 100000 };
  const int mins[] = { 1, 2, 1000, 1904, 1905, 4096, 8192, 100000, 0x7fffffff };
  const std::vector<std::vector<int>> limit_seqs = {
    { 0 }, { 100 }, { 1500, 1900, 2500 }, { 5000 }, { 9000, 9500, 12000, 30000 }, { 100000 }, { 4096, 8192, 12288 },
    { 1 << 30 }, { 50, 100000, 60 }, { 6000, 6001, 6002, 6003, 6004 },
  };
  for (int hint : hints)
    for (int maxs : maxes)
      for (int dmin : mins)
        for (const auto& limits : limit_seqs)
          for (int ok = 0; ok < 2; ++ok)
          {
            expect(shared(hint, maxs, dmin, limits, ok, true) == old_single(hint, maxs, dmin, limits, ok), "single schedule",
                   hint, maxs, dmin, ok);
            expect(shared(hint, maxs, dmin, limits, ok, false) == old_sharded(hint, maxs, dmin, limits, ok),
                   "sharded schedule", hint, maxs, dmin, ok);
          }
  // the one difference is there: a hint at the maximum sends only the single engine to the device at the start
  expect(old_single(4096, 3000, 1, { 3000 }, true).size() == 1 && old_sharded(4096, 3000, 1, { 3000 }, true).size() == 1 &&
             old_single(4096, 3000, 1, { 3000 }, true)[0].device == 1 &&
             old_sharded(4096, 3000, 1, { 3000 }, true)[0].device == 0,
         "the known difference", 0, 0, 0, 0);
  for (int x = -5000; x < 300000; x += 7)
    expect(bpf::resample_window_for(x) == old_window_for(x), "window_for", x, 0, 0, 0);
}

// ---- the systematic budget and the 31-bit check
static void check_budget()
{
  const double w_diffs[] = { 0.0, -0.5, 1e-9, 0.01, 0.0317, 0.25, 0.5, 0.999, 1.0 };
  const int limits[] = { 1, 100, 101, 2499, 2500, 4096, 99999, 100000, 1000000 };
  const int maxes[] = { 100, 2500, 4096, 100000, 1000000 };
  for (double w_diff : w_diffs)
    for (int limit : limits)
      for (int maxs : maxes)
      {
        if (limit > maxs)
          continue;  // resampleLimit never exceeds max_samples
        int count = limit, num_random = 0;
        if (w_diff > 0.0)
        {
          count *= (1.0 + w_diff);
          if (count > maxs)
            count = maxs;
          num_random = (int)(w_diff * count);
        }
        const bpf::SystematicBudget b = bpf::systematic_budget(limit, w_diff, maxs);
        expect(b.count == count && b.n_random == num_random, "budget", limit, maxs, b.count, b.n_random);
      }
  const int retries[] = { 0, 1, 2, 7, 100, 4095, 1 << 20, (1 << 30) - 1 };
  const int randoms[] = { 0, 1, 2, 79, 2500, 100000, 1000000, 0x7fffffff };
  for (int r : retries)
    for (int n : randoms)
      expect(bpf::random_calls_fit(r, n) == !(1ll + (2ll * r + 2) * n >= 0x7fffffffll), "31-bit check", r, n, 0, 0);
}

// ---- the stream account: M x retries x n_random, chain words, resolved calls
static void check_stream()
{
  const int Ms[] = { 1, 2, 100, 2076, 2500, 4096, 100000, 1 << 30 };
  const int retries[] = { 0, 1, 2, 7, 100, 4095 };
  const int randoms[] = { 0, 1, 79, 2500, 100000 };
  for (int M : Ms)
  {
    bpf::StreamUse plain;
    expect(bpf::stream_consumed(plain, M, 12345) == 2ull * (uint64_t)M, "multinomial", M, 0, 0, 0);
    for (int r : retries)
      for (int n : randoms)
      {
        // the single engine: the start, then (for num_random > 0) the random pose calls; the sharded driver: one formula
        uint64_t random_consumed = 0;
        if (n > 0)
          random_consumed = (2ull * (uint64_t)r + 2ull) * (uint64_t)n;
        const uint64_t sharded = 1ull + (2ull * (uint64_t)r + 2ull) * (uint64_t)n;
        bpf::StreamUse sys;
        sys.regime = bpf::STREAM_SYSTEMATIC;
        sys.retries = r;
        sys.n_random = n;
        const uint64_t got = bpf::stream_consumed(sys, M, -1);
        expect(got == 1ull + random_consumed && got == sharded, "systematic", M, r, n, (long long)got);
      }
    const unsigned ends[] = { 2u, 3u, 4u, 1000u, 0x7ffffff0u };
    for (unsigned end : ends)
    {
      bpf::StreamUse scored;
      scored.regime = bpf::STREAM_SYSTEMATIC_SCORED;
      scored.n_random = 5;
      scored.scored_end = end;
      expect(bpf::stream_consumed(scored, M, 0) == 1ull + ((uint64_t)end - 2ull), "scored calls", M, end, 0, 0);
    }
  }
  const int words[] = { 0, 1, 2, 5000, 0x7fffffff, (int)0x80000000u, (int)0x80000001u, (int)0x80001388u, -1 };
  for (int w : words)
  {
    const uint64_t want = (uint64_t)((unsigned)w & 0x7fffffffu) + (w < 0 ? 1ull : 0ull);
    bpf::StreamUse chain;
    chain.regime = bpf::STREAM_MULTINOMIAL_CHAIN;
    expect(bpf::chain_consumed(w) == want && bpf::stream_consumed(chain, 77, w) == want, "chain word", w, 0, 0, 0);
  }
}

// ---- the target chain, bit for bit, into a buffer of exactly n doubles
static void check_targets()
{
  const double starts[] = { 0.0, 1e-300, 0.25, 0.5, 0.999999999999, 1.0 - 1.0 / 281474976710656.0 };
  const int ns[] = { 1, 2, 3, 100, 2421, 2500, 4096, 100000 };
  for (double start : starts)
    for (int n : ns)
    {
      std::vector<double> want((size_t)n), got((size_t)n);
      const double delta = 1.0 / n;
      double t = start;
      for (int i = 0; i < n; ++i)
      {
        want[i] = t;
        t += delta;
        if (t > 1.0)
          t -= 1.0;
      }
      bpf::systematic_target_chain(start, n, got.data());
      expect(std::memcmp(want.data(), got.data(), (size_t)n * sizeof(double)) == 0, "targets", n, 0, 0, 0);
    }
}

int main()
{
  check_schedule();
  check_budget();
  check_stream();
  check_targets();
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
