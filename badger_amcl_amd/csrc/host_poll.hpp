// The host's side of a result that a kernel publishes in pinned host memory: the kernel writes its words, each tagged
// with the launch's generation, and this thread polls them instead of paying for a copy plus a stream synchronisation.
// The waits are bounded: a kernel of some tens of microseconds that has not published after milliseconds is not going
// to, and the caller falls back to what it did before (await_published in host_common.inl, or a fall-back of its own).
//
// Host code only: no HIP include, so that a stand-alone host program can compile it.
#pragma once

#include <chrono>

namespace bpf
{

// Spins until ready() is true; looks at the clock every 1024 spins and gives up (false) once `ms` have passed.
template <class Ready>
inline bool spin_until(Ready&& ready, int ms)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins)
  {
    if (ready())
      return true;
    if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms))
      return false;
    __builtin_ia32_pause();
  }
}

// words[first .. first + count): true when every one carries `generation` in its high half (acquire loads: what the
// kernel wrote before a word is visible behind it); out[0 .. count) then holds their low halves.  A word of another
// generation is never accepted, and `out` is written only on success.  (A generation's words are written once, so the
// second pass reads what the first one saw.)
inline bool tagged_words(const unsigned long long* words, int first, int count, unsigned generation, int* out)
{
  for (int k = first; k < first + count; ++k)
    if ((unsigned)(__atomic_load_n(words + k, __ATOMIC_ACQUIRE) >> 32) != generation)
      return false;
  for (int k = 0; k < count; ++k)
    out[k] = (int)(unsigned)__atomic_load_n(words + first + k, __ATOMIC_RELAXED);
  return true;
}

// the generation after g: 1 .. 0x3fffffff and round again, never 0 (what a zeroed word holds)
inline int next_generation(int g)
{
  return (g % 0x3fffffff) + 1;
}

}  // namespace bpf
