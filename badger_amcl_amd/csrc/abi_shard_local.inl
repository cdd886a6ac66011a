// C-ABI: all ranks of one sharded filter inside ONE process ("local world").
//
//   bpf_shard_connect_local(engines, world, 0)      engines[r] becomes rank r
//
// A third provider behind ShardExchange's function table (abi_mailbox_step.inl), next to the mailbox and RCCL: a
// single-process node drives W engines from W host threads, every collective one-call form works unchanged, and the
// exchanges are kernels_local_exchange.hpp's pulls between the engines' streams.
//
// No kernel waits for another rank here.  Sibling engines' streams can share a hardware queue, where a consumer that
// spins for a producer queued behind it never sees it arrive; the order is made by events and a host barrier instead.
// One exchange, on every rank (each on its own host thread):
//   1  record `ready` on the own stream (everything that produced the send data is in front of it)
//   2  publish {send, recv, count, op} in the world object
//   3  host barrier: every rank has recorded and published -- in particular every `ready` record is already in its
//      queue, so a wait for it that is enqueued from here on cannot sit in front of what it waits for
//   4  the own stream waits for the peers' `ready`
//   5  ONE launch pulls the peers' send spans into the own destination
//   6  record `done`; second host barrier
//   7  the own stream waits for the peers' `done`: nothing queued later can overwrite a send buffer a peer still reads
// The host never waits for a stream (ShardExchange::finish stays the only synchronisation); what it waits for is the
// other host threads, bounded by bpf_shard_mailbox_set_timeout_ms.  A barrier that runs out marks the world broken:
// the waiting ranks return an error with their destinations untouched (nothing was launched), and every later
// exchange fails at once until bpf_shard_connect_local makes a new world.
#include "kernels_local_exchange.hpp"

namespace
{
struct LocalWorld;

enum
{
  kLxGather = 1,
  kLxReduce64 = 2,
  kLxReduce32 = 3
};

// one rank's seat in the world; e->coll.comm points at it
struct LocalRank
{
  LocalWorld* world = nullptr;
  bpf_engine* e = nullptr;
  int rank = 0;
  bool attached = false;
  hipEvent_t ready = nullptr, done = nullptr;
  DevBuf<long long> stage;  // the send copy of an in-place all-reduce (with room to match the destination's alignment)
  // published for the exchange in progress (written before the first barrier, read by the peers after it)
  int op = 0;
  const void* send = nullptr;
  long long count = 0;
};

struct LocalWorld
{
  int world = 0;
  LocalRank seat[kMailboxMaxWorld];
  std::mutex m;
  std::condition_variable cv;
  int attached = 0;  // seats still attached; the last detach frees the world
  int arrived = 0;
  unsigned long long phase = 0;
  bool broken = false;

  // every attached rank arrives, or the world breaks: false = broken (timed out here or elsewhere, or a rank left)
  bool barrier(int timeout_ms)
  {
    std::unique_lock<std::mutex> lk(m);
    if (broken)
      return false;
    if (++arrived == world)
    {
      arrived = 0;
      ++phase;
      cv.notify_all();
      return true;
    }
    const unsigned long long mine = phase;
    const bool ok = cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&] { return phase != mine || broken; });
    if (!ok || (broken && phase == mine))
    {
      broken = true;
      cv.notify_all();
      return false;
    }
    return true;
  }
  void mark_broken()
  {
    std::lock_guard<std::mutex> lk(m);
    broken = true;
    cv.notify_all();
  }
};

thread_local std::string g_local_error;
const char* local_last_error() { return g_local_error.c_str(); }
int local_fail(const std::string& what)
{
  g_local_error = what;
  return 1;
}

int lx_grid(long long items)
{
  return (int)std::max<long long>(1, std::min<long long>((items + 255) / 256, 1024));
}

// steps 1 .. 7 above.  send: what the peers read (count words of this rank); recv: this rank's destination; dst_off:
// gather only, where rank r's words go in recv (nullptr: r * count, the uniform all-gather)
int local_exchange(LocalRank* me, int op, const void* send, long long count, void* recv, const long long* dst_off)
{
  LocalWorld* w = me->world;
  bpf_engine* e = me->e;
  hipStream_t stream = e->stream;
  const int W = w->world, timeout_ms = e->mb_timeout_ms;
  if (hipEventRecord(me->ready, stream) != hipSuccess)
  {
    w->mark_broken();
    return local_fail("local exchange: cannot record an event");
  }
  me->op = op;
  me->send = send;
  me->count = count;
  if (!w->barrier(timeout_ms))
    return local_fail("local exchange: a rank of the world did not arrive in time; the world is broken until "
                      "bpf_shard_connect_local");
  bool same = true;
  for (int r = 0; r < W; ++r)
    same = same && w->seat[r].op == op && (op == kLxGather || w->seat[r].count == count);
  if (!same)
  {
    // every rank sees the same seats and decides alike
    w->mark_broken();
    return local_fail("local exchange: the ranks entered different exchanges");
  }
  hipError_t err = hipSuccess;
  for (int r = 0; r < W && err == hipSuccess; ++r)
    if (r != me->rank)
      err = hipStreamWaitEvent(stream, w->seat[r].ready, 0);
  if (err == hipSuccess)
  {
    if (op == kLxGather)
    {
      LxGather T{};
      T.world = W;
      long long widest = 0;
      for (int r = 0; r < W; ++r)
      {
        T.src[r] = static_cast<const long long*>(w->seat[r].send);
        T.count[r] = w->seat[r].count;
        T.dst_off[r] = dst_off ? dst_off[r] : (long long)r * count;
        widest = std::max(widest, T.count[r]);
      }
      hipLaunchKernelGGL(k_local_gather_words, dim3(lx_grid((widest + 1) / 2)), dim3(256), 0, stream, T,
                         static_cast<long long*>(recv));
    }
    else
    {
      LxReduce T{};
      T.world = W;
      T.n = count;
      for (int r = 0; r < W; ++r)
        T.src[r] = w->seat[r].send;
      if (op == kLxReduce64)
        hipLaunchKernelGGL(k_local_reduce_sum_i64, dim3(lx_grid((count + 1) / 2)), dim3(256), 0, stream, T,
                           static_cast<long long*>(recv));
      else
        hipLaunchKernelGGL(k_local_reduce_sum_i32, dim3(lx_grid((count + 3) / 4)), dim3(256), 0, stream, T,
                           static_cast<int*>(recv));
    }
    err = hipGetLastError();
  }
  if (err == hipSuccess)
    err = hipEventRecord(me->done, stream);
  if (err != hipSuccess)
  {
    w->mark_broken();
    return local_fail(std::string("local exchange: ") + hipGetErrorString(err));
  }
  if (!w->barrier(timeout_ms))
    return local_fail("local exchange: a rank of the world did not finish the exchange in time; the world is broken");
  for (int r = 0; r < W; ++r)
    if (r != me->rank && hipStreamWaitEvent(stream, w->seat[r].done, 0) != hipSuccess)
    {
      w->mark_broken();
      return local_fail("local exchange: cannot wait for a peer's event");
    }
  return 0;
}

// the in-place all-reduces read a staged copy: a peer must not see the sums this rank's launch is writing.  The copy
// sits at the destination's offset within 16 bytes, so that the wide path of the kernel holds for it too.
int local_reduce(LocalRank* me, void* buf, size_t n, bool i32)
{
  bpf_engine* e = me->e;
  const size_t bytes = n * (i32 ? sizeof(int) : sizeof(long long));
  if (me->stage.reserve(bytes / sizeof(long long) + 3) != hipSuccess)
  {
    me->world->mark_broken();
    return local_fail("local exchange: staging allocation");
  }
  char* stage = reinterpret_cast<char*>(me->stage.p) + (reinterpret_cast<uintptr_t>(buf) & 15u);
  if (bytes > 0 && copy_d2d(stage, static_cast<const char*>(buf), bytes, e->stream) != hipSuccess)
  {
    me->world->mark_broken();
    return local_fail("local exchange: staging copy");
  }
  return local_exchange(me, i32 ? kLxReduce32 : kLxReduce64, stage, (long long)n, buf, nullptr);
}

int local_allgather_f64(void* comm, const double* send, double* recv, size_t count, void*)
{
  return local_exchange(static_cast<LocalRank*>(comm), kLxGather, send, (long long)count, recv, nullptr);
}
int local_allgather_i64(void* comm, const long long* send, long long* recv, size_t count, void*)
{
  return local_exchange(static_cast<LocalRank*>(comm), kLxGather, send, (long long)count, recv, nullptr);
}
int local_allreduce_sum_i64(void* comm, long long* buf, size_t count, void*)
{
  return local_reduce(static_cast<LocalRank*>(comm), buf, count, false);
}
int local_allreduce_sum_i32(void* comm, int* buf, size_t count, void*)
{
  return local_reduce(static_cast<LocalRank*>(comm), buf, count, true);
}

// fn.destroy of the local table (collective_release, with the engine's device selected): this seat leaves; a world
// that has lost a rank cannot exchange any more; the last one out frees it
int local_detach(void* comm)
{
  LocalRank* me = static_cast<LocalRank*>(comm);
  if (!me || !me->attached)
    return 0;
  LocalWorld* w = me->world;
  (void)hipStreamSynchronize(me->e->stream);  // teardown, not an exchange: nothing of this rank is in flight afterwards
  if (me->ready)
    (void)hipEventDestroy(me->ready);
  if (me->done)
    (void)hipEventDestroy(me->done);
  me->ready = me->done = nullptr;
  me->stage.release();
  bool last = false;
  {
    std::lock_guard<std::mutex> lk(w->m);
    me->attached = false;
    w->broken = true;
    last = --w->attached == 0;
    w->cv.notify_all();
  }
  if (last)
    delete w;
  return 0;
}

bool local_active(const bpf_engine* e) { return e->coll.active && e->coll.local; }
}  // namespace

int bpf_shard_connect_local(bpf_engine* const* engines, int world, int flags)
{
  if (!engines || world < 1 || world > kMailboxMaxWorld || flags != 0)
    return BPF_ERR_INVALID_ARGUMENT;
  for (int r = 0; r < world; ++r)
  {
    if (!engines[r] || !engines[r]->have_pf)
      return BPF_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < r; ++q)
      if (engines[q] == engines[r])
        return BPF_ERR_INVALID_ARGUMENT;
    if (engines[r]->min_samples != engines[0]->min_samples || engines[r]->max_samples != engines[0]->max_samples)
      return BPF_ERR_INVALID_ARGUMENT;  // the engines of a sharded filter carry the GLOBAL bounds
  }
  int device_before = 0;
  if (hipGetDevice(&device_before) != hipSuccess)
    return BPF_ERR_HIP;
  // engines on different devices read each other's buffers: peer access, both ways
  for (int r = 0; r < world; ++r)
    for (int q = 0; q < world; ++q)
    {
      const int a = engines[r]->device, b = engines[q]->device;
      int can = 0;
      if (a != b && (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can))
        return BPF_ERR_UNSUPPORTED;
    }
  LocalWorld* w = new LocalWorld();
  w->world = world;
  bool ok = true;
  for (int r = 0; r < world && ok; ++r)
  {
    LocalRank& s = w->seat[r];
    s.world = w;
    s.e = engines[r];
    s.rank = r;
    ok = hipSetDevice(engines[r]->device) == hipSuccess &&
         hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
    for (int q = 0; q < world && ok; ++q)
      if (engines[q]->device != engines[r]->device)
      {
        const hipError_t pe = hipDeviceEnablePeerAccess(engines[q]->device, 0);
        if (pe == hipErrorPeerAccessAlreadyEnabled)
          (void)hipGetLastError();
        else
          ok = pe == hipSuccess;
      }
  }
  if (!ok)
  {
    (void)hipGetLastError();
    for (int r = 0; r < world; ++r)
    {
      (void)hipSetDevice(engines[r]->device);
      if (w->seat[r].ready)
        (void)hipEventDestroy(w->seat[r].ready);
      if (w->seat[r].done)
        (void)hipEventDestroy(w->seat[r].done);
    }
    delete w;
    (void)hipSetDevice(device_before);
    return BPF_ERR_HIP;
  }
  // from here on nothing fails: the engines change hands
  w->attached = world;
  for (int r = 0; r < world; ++r)
  {
    bpf_engine* e = engines[r];
    (void)hipSetDevice(e->device);
    collective_release(e);  // (an earlier local world included)
    (void)bpf_shard_mailbox_destroy(e);
    bpf_engine::Collective& c = e->coll;
    c.fn = bpf_engine::Collective::Fn{};
    c.fn.last_error = local_last_error;
    c.fn.destroy = local_detach;
    c.fn.allgather_f64 = local_allgather_f64;
    c.fn.allgather_i64 = local_allgather_i64;
    c.fn.allreduce_sum_i64 = local_allreduce_sum_i64;
    c.fn.allreduce_sum_i32 = local_allreduce_sum_i32;
    w->seat[r].attached = true;
    c.comm = &w->seat[r];
    c.local = true;
    c.active = true;
    c.exchanges = 0;
    e->shard_rank = r;
    e->shard_world = world;
    e->mb_totals_valid = false;
  }
  (void)hipSetDevice(device_before);
  return BPF_OK;
}

int bpf_shard_exchange_mode(const bpf_engine* e, int* mode_out)
{
  if (!e || !mode_out)
    return BPF_ERR_INVALID_ARGUMENT;
  *mode_out = e->mb.active ? BPF_SHARD_EXCHANGE_MAILBOX
                           : !e->coll.active ? 0 : e->coll.local ? BPF_SHARD_EXCHANGE_LOCAL : BPF_SHARD_EXCHANGE_RCCL;
  return BPF_OK;
}

namespace
{
// what rank r contributes to word i of a self-test exchange (never zero, different for every rank, round and word)
long long lx_pattern(int rank, int round, int kind, long long i)
{
  return (long long)(((unsigned long long)(rank + 1) << 40) ^ ((unsigned long long)(round + 1) << 32) ^
                     ((unsigned long long)kind << 28) ^ ((unsigned long long)i * 0x9E3779B1ull & 0xFFFFFFFull));
}
int lx_pattern32(int rank, int round, long long i)
{
  // large enough that the int32 sum of 16 of them wraps: the widened sum narrowed again must equal it
  return (int)(0x0C000000 * (rank + 1) + 977 * (round + 1) + (int)(i * 31));
}
}  // namespace

// Every kind of exchange the local transport has, with payloads that can be checked cell by cell: ragged int64 gathers
// (the rank `round % world` contributes nothing; odd counts leave the later ranks' spans off the 16-byte grid, and odd
// ranks send from an odd word), the uniform f64 all-gather, and the int64 / int32 all-reduces in place at every
// offset within 16 bytes; word counts 0, 1, 255, 256, 257 and 6 * 4096 + 3.  The words in front of and behind every
// destination must come back untouched.  Collective: every rank calls it with the same `rounds`.
int bpf_shard_local_selftest(bpf_engine* e, int rounds)
{
  if (!e || rounds < 1 || rounds > 64)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!local_active(e))
    return e->fail(BPF_ERR_NOT_CONFIGURED, "no local world (bpf_shard_connect_local)");
  HIPCHK(e, hipSetDevice(e->device));
  LocalRank* me = static_cast<LocalRank*>(e->coll.comm);
  const int W = e->shard_world, rank = e->shard_rank;
  static const long long kWords[] = { 0, 1, 255, 256, 257, 6 * 4096 + 3 };
  const long long kGuard = 4, kFill = 0x5A5A5A5A5A5A5A5All;
  const long long widest = kWords[5] + W;
  DevBuf<long long> d_send, d_recv;
  HIPCHK(e, d_send.reserve((size_t)widest + 8));
  HIPCHK(e, d_recv.reserve((size_t)(widest * W + 2 * kGuard + 8)));
  std::vector<long long> h_send, h_recv, want;
  auto exchange_failed = [&]() { return e->fail(BPF_ERR_EXCHANGE, std::string("local self-test: ") + local_last_error()); };
  auto mismatch = [&](const char* what, long long n) {
    // the peers must not wait for this rank in the next exchange
    me->world->mark_broken();
    return e->fail(BPF_ERR_EXCHANGE, std::string("local self-test: ") + what + " of " + std::to_string(n) +
                                         " words did not arrive as the ranks wrote them");
  };
  for (int round = 0; round < rounds; ++round)
    for (long long n : kWords)
    {
      // ---- ragged gather of int64 words
      {
        const int empty = W > 1 ? round % W : -1;
        long long counts[kMailboxMaxWorld], off[kMailboxMaxWorld], total = 0;
        for (int r = 0; r < W; ++r)
        {
          counts[r] = r == empty ? 0 : n + r;
          off[r] = kGuard + total;
          total += counts[r];
        }
        const int lead = rank & 1;  // odd ranks send from an odd word
        h_send.assign((size_t)(counts[rank] + lead), 0);
        for (long long i = 0; i < counts[rank]; ++i)
          h_send[(size_t)(i + lead)] = lx_pattern(rank, round, 1, i);
        h_recv.assign((size_t)(total + 2 * kGuard), kFill);
        if (!h_send.empty())
          H2D_OR_RETURN(h2d_from_host(e, d_send.p, h_send.data(), h_send.size() * 8, e->stream));
        // (the pageable sources are reused below: the pageable way up has read them when it returns)
        H2D_OR_RETURN(h2d_from_host_sync(e, d_recv.p, h_recv.data(), h_recv.size() * 8));
        if (local_exchange(me, kLxGather, d_send.p + lead, counts[rank], d_recv.p, off) != 0)
          return exchange_failed();
        H2D_OR_RETURN(d2h_to_host(e, h_recv.data(), d_recv.p, h_recv.size() * 8, e->stream));
        want.assign(h_recv.size(), kFill);
        for (int r = 0; r < W; ++r)
          for (long long i = 0; i < counts[r]; ++i)
            want[(size_t)(off[r] + i)] = lx_pattern(r, round, 1, i);
        if (want != h_recv)
          return mismatch("a ragged gather", n);
      }
      // ---- uniform all-gather of f64 (the totals' entry point), destination one word off the 16-byte grid
      {
        std::vector<double> hs((size_t)n), hr((size_t)(n * W + 2 * kGuard + 1)), wt;
        for (long long i = 0; i < n; ++i)
          hs[(size_t)i] = (double)(rank + 1) + 1e-3 * (double)i + 1e-7 * round;
        std::fill(hr.begin(), hr.end(), -1.0);
        if (n > 0)
          H2D_OR_RETURN(h2d_from_host(e, d_send.p, hs.data(), hs.size() * 8, e->stream));
        H2D_OR_RETURN(h2d_from_host_sync(e, d_recv.p, hr.data(), hr.size() * 8));
        double* recv = reinterpret_cast<double*>(d_recv.p) + kGuard + 1;
        if (e->coll.fn.allgather_f64(me, reinterpret_cast<const double*>(d_send.p), recv, (size_t)n, e->stream) != 0)
          return exchange_failed();
        H2D_OR_RETURN(d2h_to_host(e, hr.data(), d_recv.p, hr.size() * 8, e->stream));
        wt.assign(hr.size(), -1.0);
        for (int r = 0; r < W; ++r)
          for (long long i = 0; i < n; ++i)
            wt[(size_t)(kGuard + 1 + r * n + i)] = (double)(r + 1) + 1e-3 * (double)i + 1e-7 * round;
        if (std::memcmp(wt.data(), hr.data(), hr.size() * 8) != 0)
          return mismatch("an f64 all-gather", n);
      }
      // ---- all-reduce(sum) of int64 in place, at an even and an odd word
      for (int lead = 0; lead < 2; ++lead)
      {
        h_recv.assign((size_t)(n + 2 * kGuard + lead), kFill);
        for (long long i = 0; i < n; ++i)
          h_recv[(size_t)(kGuard + lead + i)] = lx_pattern(rank, round, 2 + lead, i);
        H2D_OR_RETURN(h2d_from_host_sync(e, d_recv.p, h_recv.data(), h_recv.size() * 8));
        if (e->coll.fn.allreduce_sum_i64(me, d_recv.p + kGuard + lead, (size_t)n, e->stream) != 0)
          return exchange_failed();
        H2D_OR_RETURN(d2h_to_host(e, h_recv.data(), d_recv.p, h_recv.size() * 8, e->stream));
        want.assign(h_recv.size(), kFill);
        for (long long i = 0; i < n; ++i)
        {
          unsigned long long acc = 0;
          for (int r = 0; r < W; ++r)
            acc += (unsigned long long)lx_pattern(r, round, 2 + lead, i);
          want[(size_t)(kGuard + lead + i)] = (long long)acc;
        }
        if (want != h_recv)
          return mismatch("an int64 all-reduce", n);
      }
      // ---- all-reduce(sum) of int32 in place, at each of the four offsets within 16 bytes
      for (int lead = 0; lead < 4; ++lead)
      {
        std::vector<int> hb((size_t)(n + 4 * kGuard + lead), 0x5A5A5A5A), wt;
        for (long long i = 0; i < n; ++i)
          hb[(size_t)(2 * kGuard + lead + i)] = lx_pattern32(rank, round, i);
        int* d = reinterpret_cast<int*>(d_recv.p);
        H2D_OR_RETURN(h2d_from_host_sync(e, d, hb.data(), hb.size() * 4));
        if (e->coll.fn.allreduce_sum_i32(me, d + 2 * kGuard + lead, (size_t)n, e->stream) != 0)
          return exchange_failed();
        wt.assign(hb.size(), 0x5A5A5A5A);
        H2D_OR_RETURN(d2h_to_host(e, hb.data(), d, hb.size() * 4, e->stream));
        for (long long i = 0; i < n; ++i)
        {
          long long acc = 0;
          for (int r = 0; r < W; ++r)
            acc += (long long)lx_pattern32(r, round, i);
          wt[(size_t)(2 * kGuard + lead + i)] = (int)acc;
        }
        if (wt != hb)
          return mismatch("an int32 all-reduce", n);
      }
    }
  return BPF_OK;
}

// Measurement: `reps` exchanges of one kind back to back over the engine's collective provider (the local world, or
// RCCL), the host's wall time per exchange between two stream synchronisations.  kind 0: f64 all-gather of `words`
// words per rank (1 = the totals); kind 1: int64 all-reduce(sum) in place of `words` words (6 * 4096 = a draw window).
// Collective: every rank calls it with the same arguments; one exchange in front of the clock lines the ranks up.
int bpf_shard_exchange_probe(bpf_engine* e, int kind, long long words, int reps, double* ms_per_exchange_out)
{
  if (!e || !ms_per_exchange_out || kind < 0 || kind > 1 || words < 1 || words > (1ll << 24) || reps < 1 || reps > 100000)
    return BPF_ERR_INVALID_ARGUMENT;
  if (!e->coll.active)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "exchange probe: no collective exchange (bpf_shard_connect_local / bootstrap)");
  HIPCHK(e, hipSetDevice(e->device));
  bpf_engine::Collective& c = e->coll;
  HIPCHK(e, c.send.reserve((size_t)words));
  HIPCHK(e, c.recv.reserve((size_t)words * (size_t)e->shard_world));
  HIPCHK(e, hipMemsetAsync(c.send.p, 0, (size_t)words * sizeof(long long), e->stream));
  auto once = [&]() {
    return kind == 0 ? c.fn.allgather_f64(c.comm, reinterpret_cast<const double*>(c.send.p),
                                          reinterpret_cast<double*>(c.recv.p), (size_t)words, e->stream)
                     : c.fn.allreduce_sum_i64(c.comm, c.send.p, (size_t)words, e->stream);
  };
  if (once() != 0)
    return e->fail(BPF_ERR_EXCHANGE, std::string("exchange probe: ") + c.fn.last_error());
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < reps; ++k)
    if (once() != 0)
      return e->fail(BPF_ERR_EXCHANGE, std::string("exchange probe: ") + c.fn.last_error());
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *ms_per_exchange_out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
  return BPF_OK;
}
