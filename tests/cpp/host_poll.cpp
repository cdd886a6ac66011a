// Stand-alone host check of badger_amcl_amd/csrc/host_poll.hpp, the host's side of a result that a kernel publishes in
// pinned memory behind a generation tag.  A writer thread stands in for the kernel.
// No GPU and no library: g++ -std=c++17 -O1 -pthread -I badger_amcl_amd/csrc tests/cpp/host_poll.cpp && ./a.out
#include <chrono>
#include <cstdio>
#include <thread>

#include "host_poll.hpp"

static int failures = 0;

static void expect(bool ok, const char* what)
{
  if (!ok && ++failures <= 10)
    std::fprintf(stderr, "FAIL %s\n", what);
}

static unsigned long long tagged(unsigned generation, int low)
{
  return ((unsigned long long)generation << 32) | (unsigned)low;
}

constexpr int kWords = 8, kFirst = 1, kCount = 7;  // the pieces form's block: word 0 unused, words 1 .. 7 polled
constexpr int kSentinel = -12345;

static bool untouched(const int* out)
{
  for (int k = 0; k < kCount; ++k)
    if (out[k] != kSentinel)
      return false;
  return true;
}

// every partial state of a block on its way from generation g - 1 to g, on one thread
static void partial_blocks_are_refused()
{
  const unsigned g = 7;
  for (int written = 0; written <= kCount; ++written)
  {
    unsigned long long words[kWords];
    for (int k = 0; k < kWords; ++k)
      words[k] = tagged(k - kFirst < written ? g : g - 1, 100 * (k - kFirst < written ? 2 : 1) + k);
    words[0] = tagged(g - 1, 0);  // outside the range: not looked at
    int out[kCount];
    for (int k = 0; k < kCount; ++k)
      out[k] = kSentinel;
    const bool ok = bpf::tagged_words(words, kFirst, kCount, g, out);
    if (written < kCount)
      expect(!ok && untouched(out), "a block with words of the previous generation was accepted or out was written");
    else
    {
      expect(ok, "a complete block was refused");
      for (int k = 0; k < kCount; ++k)
        expect(out[k] == 200 + kFirst + k, "low half");
    }
  }
  // a complete block of the previous generation, and one of a later generation
  unsigned long long words[kWords];
  int out[kCount];
  for (int k = 0; k < kCount; ++k)
    out[k] = kSentinel;
  for (int k = 0; k < kWords; ++k)
    words[k] = tagged(g - 1, k);
  expect(!bpf::tagged_words(words, kFirst, kCount, g, out) && untouched(out), "the previous generation was accepted");
  for (int k = 0; k < kWords; ++k)
    words[k] = tagged(g + 1, k);
  expect(!bpf::tagged_words(words, kFirst, kCount, g, out) && untouched(out), "another generation was accepted");
  // a negative low half comes back as it went in (a stop count of -1)
  for (int k = 0; k < kWords; ++k)
    words[k] = tagged(g, -1 - k);
  expect(bpf::tagged_words(words, kFirst, kCount, g, out) && out[0] == -2 && out[kCount - 1] == -1 - kFirst - (kCount - 1),
         "negative low halves");
}

// the writer publishes word after word with a pause between them; the reader spins on the block
static void a_block_arrives_word_by_word()
{
  for (unsigned g = 2; g < 6; ++g)
  {
    alignas(64) static unsigned long long words[kWords];
    for (int k = 0; k < kWords; ++k)
      __atomic_store_n(&words[k], tagged(g - 1, 1000 + k), __ATOMIC_RELAXED);
    int published = 0;  // words the writer has stored so far
    std::thread writer([&] {
      for (int k = kFirst; k < kFirst + kCount; ++k)
      {
        std::this_thread::sleep_for(std::chrono::microseconds(300));
        __atomic_store_n(&words[k], tagged(g, (int)(10 * g) + k), __ATOMIC_RELEASE);
        __atomic_store_n(&published, k - kFirst + 1, __ATOMIC_RELEASE);
      }
    });
    int out[kCount];
    for (int k = 0; k < kCount; ++k)
      out[k] = kSentinel;
    long polls = 0, early = 0;
    const bool seen = bpf::spin_until(
        [&] {
          ++polls;
          const bool ok = bpf::tagged_words(words, kFirst, kCount, g, out);
          const int after = __atomic_load_n(&published, __ATOMIC_ACQUIRE);
          if (ok && after < kCount - 1)
            ++early;  // (the last word may be visible a moment before the writer's counter)
          if (!ok && !untouched(out))
            ++early;
          return ok;
        },
        5000);
    writer.join();
    expect(seen, "the block never arrived");
    expect(early == 0, "success before every word carried the generation, or out written by a refused poll");
    std::printf("generation %u: complete after %ld polls\n", g, polls);
    for (int k = 0; k < kCount; ++k)
      expect(out[k] == (int)(10 * g) + kFirst + k, "low half of a published word");
  }
}

static void a_wait_that_never_ends_takes_its_bound()
{
  const auto t0 = std::chrono::steady_clock::now();
  const bool seen = bpf::spin_until([] { return false; }, 30);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  expect(!seen, "a ready() that is never true was reported ready");
  expect(ms >= 30.0, "gave up before its bound");
  expect(ms < 5000.0, "took far longer than its bound");
  std::printf("a 30 ms wait gave up after %.2f ms\n", ms);
  expect(bpf::spin_until([] { return true; }, 0), "a ready() that is true at once");
}

static void generations_wrap_past_zero()
{
  expect(bpf::next_generation(0) == 1, "0 -> 1");
  expect(bpf::next_generation(1) == 2, "1 -> 2");
  expect(bpf::next_generation(0x3ffffffe) == 0x3fffffff, "0x3ffffffe -> 0x3fffffff");
  expect(bpf::next_generation(0x3fffffff) == 1, "0x3fffffff -> 1");
  int g = 0x3fffffff - 5;
  for (int k = 0; k < 12; ++k)
  {
    const int next = bpf::next_generation(g);
    expect(next >= 1 && next <= 0x3fffffff && next != g, "a generation outside 1 .. 0x3fffffff, or the same again");
    g = next;
  }
  expect(g == 7, "twelve steps from 0x3ffffffa");
}

int main()
{
  partial_blocks_are_refused();
  a_block_arrives_word_by_word();
  a_wait_that_never_ends_takes_its_bound();
  generations_wrap_past_zero();
  std::printf("host_poll: %d failures\n", failures);
  return failures ? 1 : 0;
}
