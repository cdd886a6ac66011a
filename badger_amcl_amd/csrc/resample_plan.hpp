// The arithmetic the resample drivers share (host_resample.inl: the single engine; abi_mailbox_step.inl and
// abi_sharded.inl: the sharded filter): the multinomial window schedule, the systematic resampler's recovery budget and
// target chain, and the account of the drand48 stream.  Host code only, no HIP include, so that a stand-alone host
// program can compile it (tests/cpp/resample_plan.cpp).
#pragma once

#include <algorithm>
#include <cstdint>

namespace bpf
{

// a resample window for a stop expected x draws ahead: a quarter more, in whole 1024s.  The window hint after a
// resample that kept x samples, and the next window's size from the bound for the leaves seen so far.
inline int resample_window_for(int x)
{
  return std::max(1024, (x + x / 4 + 1023) / 1024 * 1024);
}

// ---- the multinomial resampler's window schedule: which candidate draws [m0, m1) the next window takes, and when
// the whole stream goes to the device tree instead of the host's ordered replay
struct WindowSchedule
{
  int max_samples = 0, device_min = 0;
  bool device_at_start = false;   // the previous cycle ran to the end, and the driver lets that count (window_schedule)
  bool device_declined = false;   // the latch: this stream is outside what the device tree takes, host replay from here
  int m0 = 0, window = 0;

  int m1() const { return std::min(max_samples, m0 + window); }

  // Long stream ahead: the windows so far found no stop and the bound for the leaves seen so far (`limit`, a lower
  // estimate of where the stop will be; read only behind a first window) is still far away -- the whole stream goes
  // to the device tree, unless it declined this stream before.
  bool whole_stream_due(int limit) const
  {
    const bool long_stream = m0 > 0 ? limit - m0 >= device_min : device_at_start;
    return long_stream && max_samples - m0 >= device_min && !device_declined;
  }

  // behind a host-replayed window: the next one reaches a quarter past the bound for the leaves seen so far
  void next(int limit)
  {
    m0 = m1();
    window = resample_window_for(limit - m0);
  }
};

// The first window is the hint within [1024, max], kept short (4096) when the device tree could take over after it.
// whole_stream_at_start: with a hint at or beyond max_samples the device tree may take the stream before any host
//   window.  The single engine passes true, the sharded driver false: a difference as found, recorded in DESIGN.md.
inline WindowSchedule window_schedule(int hint, int max_samples, int device_min, bool whole_stream_at_start)
{
  WindowSchedule s;
  s.max_samples = max_samples;
  s.device_min = device_min;
  s.device_at_start = whole_stream_at_start && hint >= max_samples;
  s.window = std::max(1024, std::min(hint, max_samples));
  if (s.window > 4096 && max_samples - 4096 >= device_min)
    s.window = 4096;
  return s;
}

// ---- the systematic resampler's sample budget (particle_filter.cpp:276, 295-306): with w_diff > 0 room for random
// poses on top of the systematic ones.  `limit`: resampleLimit of the current set's leaf count.
struct SystematicBudget
{
  int count = 0, n_random = 0;
};

inline SystematicBudget systematic_budget(int limit, double w_diff, int max_samples)
{
  SystematicBudget b;
  b.count = limit;
  if (w_diff > 0.0)
  {
    b.count *= (1.0 + w_diff);
    if (b.count > max_samples)
      b.count = max_samples;
    b.n_random = (int)(w_diff * b.count);
  }
  return b;
}

// the random pose calls (2 (retries + 1) uniforms each, right behind the systematic start) stay within 31-bit positions
inline bool random_calls_fit(int retries, int n_random)
{
  return 1ll + (2ll * retries + 2) * n_random < 0x7fffffffll;
}

// the systematic targets: a serial floating-point chain (particle_filter.cpp:337-341), target += delta, and
// target -= 1 once it passes 1
inline void systematic_target_chain(double start, int n_systematic, double* out)
{
  const double delta = 1.0 / n_systematic;
  double t = start;
  for (int i = 0; i < n_systematic; ++i)
  {
    out[i] = t;
    t += delta;
    if (t > 1.0)
      t -= 1.0;
  }
}

// ---- the account of the drand48 stream: elements a resample that kept M samples consumed
enum StreamRegime
{
  STREAM_MULTINOMIAL,         // two uniforms per draw: 2 M
  STREAM_MULTINOMIAL_CHAIN,   // w_diff > 0: where the draw chain says draw M - 1 ended
  STREAM_SYSTEMATIC,          // the start, then 2 (retries + 1) uniforms per random pose call
  STREAM_SYSTEMATIC_SCORED,   // the start, then the resolved calls up to stream position scored_end
};

// stream elements the draws 0 .. m consumed, from chain[m]: up to r, or up to the second element of the accepted trial
inline uint64_t chain_consumed(int chain_word)
{
  return (uint64_t)((unsigned)chain_word & 0x7fffffffu) + (chain_word < 0 ? 1ull : 0ull);
}

struct StreamUse
{
  StreamRegime regime = STREAM_MULTINOMIAL;
  int retries = 0, n_random = 0;   // STREAM_SYSTEMATIC
  unsigned scored_end = 0;         // STREAM_SYSTEMATIC_SCORED: resolve_scored_calls' end (the calls began at 2)
};

// chain_word: chain[M - 1], read only in STREAM_MULTINOMIAL_CHAIN
inline uint64_t stream_consumed(const StreamUse& s, int M, int chain_word)
{
  switch (s.regime)
  {
    case STREAM_MULTINOMIAL_CHAIN:
      return chain_consumed(chain_word);
    case STREAM_SYSTEMATIC:
      return 1ull + (2ull * (uint64_t)s.retries + 2ull) * (uint64_t)s.n_random;
    case STREAM_SYSTEMATIC_SCORED:
      return 1ull + ((uint64_t)s.scored_end - 2ull);
    default:
      return 2ull * (uint64_t)M;
  }
}

}  // namespace bpf
