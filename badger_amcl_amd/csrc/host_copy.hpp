// Every copy between host and device, and every device-to-device copy, of the engine: the only file of csrc/ that
// names the runtime's copy calls (tests/test_abi.py keeps it that way).  Part of the one translation unit engine.hip.
//
// The rule: the KIND of the host memory is in the function's name and argument types.
//   pinned_up / pinned_down    the host side is an engine PinnedBuf, passed as the buffer with an element offset: a
//                              std::vector's data() or a stack address does not compile.  Asynchronous.
//   h2d_from_host[_sync] /     PAGEABLE memory (the caller's, or a std::vector of the engine's): the only functions
//   d2h_to_host                that take a void* host address.  They decide between the bounce buffer and the runtime.
//   small_down_sync (and its   a few words on their way into a local variable: through the engine's small pinned
//   queue / read halves)       scratch, behind one stream synchronisation.
//   copy_d2d                   both sides on the device.
//
// Why: a copy from or to PAGEABLE memory of more than a megabyte makes the runtime pin the range on the fly, and it
// keeps such pins in a small cache keyed by address and size.  A buffer that has been freed and allocated again at
// the same address -- what an allocator does all day -- then meets a pin of pages that are gone: the copy reads stale
// data (seen as a weight vector from the previous call in tests/test_gpu_seam_a.py, once in ~20 runs of the suite) or
// the GPU faults on the host address ("Memory access fault ... Reason: Unknown" at a heap address in
// tests/test_gpu_soaks.py, one run in five; none in nine runs with the runtime's pinned transfers switched off).  So
// pageable memory of any size crosses through the engine's own pinned bounce buffer, two halves of kBounceHalf: this
// thread copies a piece into (out of) one half while the copy engine empties (fills) the other.  Registered buffers
// (bpf_host_buffer_register: the owner's promise that the memory stays) and BPF_OPT_HOST_DIRECT_PAGEABLE = 1 (the
// same promise for every buffer) go to the runtime as they are.
#pragma once

namespace
{
constexpr size_t kBounceHalf = (size_t)2 << 20;
#define H2D_OR_RETURN(call)   \
  do                          \
  {                           \
    const int _rc = (call);   \
    if (_rc != BPF_OK)        \
      return _rc;             \
  } while (0)

// the registered range (bpf_host_buffer_register, BPF_OPT_HOST_AUTO_REGISTER) that holds [ptr, ptr + bytes), or null
bpf_engine::HostReg* host_reg_find(bpf_engine* e, const void* ptr, size_t bytes)
{
  const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  for (auto& r : e->host_regs)
    if (a >= r.base && a + bytes <= r.base + r.bytes)
      return &r;
  return nullptr;
}

// ------------------------------------------------------------------ pinned host memory
// `count` elements of the DEVICE buffer's type D between dev[dev_off ...] and host[host_off ...] (host_off in
// elements of H; H differs from D only where a staging buffer is lent out, download_weights).  Both ranges are checked
// against the buffers' capacities.  In stream order on `st`; nothing waits.
template <class H, class D>
int pinned_range_ok(bpf_engine* e, const PinnedBuf<H>& host, size_t host_off, const DevBuf<D>& dev, size_t dev_off,
                    size_t count)
{
  if (host_off * sizeof(H) + count * sizeof(D) > host.cap * sizeof(H) || dev_off + count > dev.cap)
    return e->fail(BPF_ERR_CAPACITY, "copy between pinned and device memory: range outside a buffer");
  return BPF_OK;
}

template <class H, class D>
int pinned_up(bpf_engine* e, DevBuf<D>& dev, size_t dev_off, const PinnedBuf<H>& host, size_t host_off, size_t count,
              hipStream_t st)
{
  H2D_OR_RETURN(pinned_range_ok(e, host, host_off, dev, dev_off, count));
  HIPCHK(e, hipMemcpyAsync(dev.p + dev_off, host.p + host_off, count * sizeof(D), hipMemcpyHostToDevice, st));
  return BPF_OK;
}

template <class H, class D>
int pinned_down(bpf_engine* e, PinnedBuf<H>& host, size_t host_off, const DevBuf<D>& dev, size_t dev_off, size_t count,
                hipStream_t st)
{
  H2D_OR_RETURN(pinned_range_ok(e, host, host_off, dev, dev_off, count));
  HIPCHK(e, hipMemcpyAsync(host.p + host_off, dev.p + dev_off, count * sizeof(D), hipMemcpyDeviceToHost, st));
  return BPF_OK;
}

// the download and the wait for it, where the host reads the words next
template <class H, class D>
int pinned_down_sync(bpf_engine* e, PinnedBuf<H>& host, size_t host_off, const DevBuf<D>& dev, size_t dev_off,
                     size_t count, hipStream_t st)
{
  H2D_OR_RETURN(pinned_down(e, host, host_off, dev, dev_off, count, st));
  HIPCHK(e, hipStreamSynchronize(st));
  return BPF_OK;
}

// ------------------------------------------------------------------ a few words into a local variable
// `count` T from the device into the engine's small pinned scratch at byte `at`, in stream order; small_read hands
// them out once the caller has synchronised the stream.  small_down_sync is the usual sequence of the three.
template <class T>
int small_down(bpf_engine* e, size_t at, const T* dev_src, size_t count, hipStream_t st)
{
  if (at + count * sizeof(T) > kSmallResultBytes)
    return e->fail(BPF_ERR_CAPACITY, "small result larger than the engine's pinned scratch");
  HIPCHK(e, e->h_small.reserve(kSmallResultBytes));
  HIPCHK(e, hipMemcpyAsync(e->h_small.p + at, dev_src, count * sizeof(T), hipMemcpyDeviceToHost, st));
  return BPF_OK;
}

template <class T>
void small_read(const bpf_engine* e, size_t at, T* out, size_t count)
{
  std::memcpy(out, e->h_small.p + at, count * sizeof(T));
}

template <class T>
int small_down_sync(bpf_engine* e, T* out, const T* dev_src, size_t count, hipStream_t st)
{
  H2D_OR_RETURN(small_down(e, 0, dev_src, count, st));
  HIPCHK(e, hipStreamSynchronize(st));
  small_read(e, 0, out, count);
  return BPF_OK;
}

// ------------------------------------------------------------------ device to device
template <class T>
hipError_t copy_d2d(T* dst, const T* src, size_t count, hipStream_t st)
{
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, st);
}

// ------------------------------------------------------------------ pageable host memory
// true when [host, host + bytes) may go to the runtime as it is
bool host_direct_ok(bpf_engine* e, const void* host, size_t bytes)
{
  return e->host_direct || host_reg_find(e, host, bytes) != nullptr;
}

int bounce_ready(bpf_engine* e)
{
  HIPCHK(e, e->h_bounce.reserve(2 * kBounceHalf));
  for (int h = 0; h < 2; ++h)
    if (e->bounce_ev[h] == nullptr)
      HIPCHK(e, hipEventCreateWithFlags(&e->bounce_ev[h], hipEventDisableTiming));
  return BPF_OK;
}

// The way up: on return the source has been read completely; the device has it in stream order on `st`.
int h2d_from_host(bpf_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st)
{
  if (bytes == 0)
    return BPF_OK;
  if (host_direct_ok(e, src, bytes))
  {
    HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return BPF_OK;
  }
  H2D_OR_RETURN(bounce_ready(e));
  const unsigned char* s = static_cast<const unsigned char*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  for (size_t off = 0; off < bytes; off += kBounceHalf)
  {
    const size_t piece = std::min(kBounceHalf, bytes - off);
    const int h = e->bounce_next;
    e->bounce_next ^= 1;
    if (e->bounce_busy[h])
      HIPCHK(e, hipEventSynchronize(e->bounce_ev[h]));  // (the copy that last read this half)
    unsigned char* half = e->h_bounce.p + (size_t)h * kBounceHalf;
    std::memcpy(half, s + off, piece);
    HIPCHK(e, hipMemcpyAsync(d + off, half, piece, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipEventRecord(e->bounce_ev[h], st));
    e->bounce_busy[h] = true;
  }
  return BPF_OK;
}

// the same on the engine's stream, and the device has it when the call returns (where a plain hipMemcpy stood)
int h2d_from_host_sync(bpf_engine* e, void* dst, const void* src, size_t bytes)
{
  H2D_OR_RETURN(h2d_from_host(e, dst, src, bytes, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return BPF_OK;
}

// The way down: piece by piece into the bounce buffer and from there by this thread.  Everything queued on `st`
// before the call is done when it returns, and so is the copy.
int d2h_to_host(bpf_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st)
{
  if (bytes == 0)
    return BPF_OK;
  if (host_direct_ok(e, dst, bytes))
  {
    HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return BPF_OK;
  }
  H2D_OR_RETURN(bounce_ready(e));
  for (int h = 0; h < 2; ++h)
  {
    if (e->bounce_busy[h])
      HIPCHK(e, hipEventSynchronize(e->bounce_ev[h]));  // (an upload that may still be reading this half)
    e->bounce_busy[h] = false;
  }
  unsigned char* d = static_cast<unsigned char*>(dst);
  const unsigned char* s = static_cast<const unsigned char*>(src);
  // two pieces in flight: the copy engine fills one half while this thread empties the other
  size_t issued = 0, taken = 0;
  int h_issue = 0, h_take = 0;
  while (taken < bytes)
  {
    while (issued < bytes && issued - taken < 2 * kBounceHalf)
    {
      const size_t piece = std::min(kBounceHalf, bytes - issued);
      HIPCHK(e, hipMemcpyAsync(e->h_bounce.p + (size_t)h_issue * kBounceHalf, s + issued, piece, hipMemcpyDeviceToHost, st));
      HIPCHK(e, hipEventRecord(e->bounce_ev[h_issue], st));
      issued += piece;
      h_issue ^= 1;
    }
    const size_t piece = std::min(kBounceHalf, bytes - taken);
    HIPCHK(e, hipEventSynchronize(e->bounce_ev[h_take]));
    std::memcpy(d + taken, e->h_bounce.p + (size_t)h_take * kBounceHalf, piece);
    taken += piece;
    h_take ^= 1;
  }
  return BPF_OK;
}
}  // namespace
