// Host helpers shared by every part of the engine: profiling scopes, drand48 jump tables, LUT encoding.  (Copies
// between host and device are host_copy.hpp's: pageable memory never goes to the runtime's copy calls from here.)

// The open-addressing table of n keys: the smallest power of two >= 2 n, at least 1024 (at most half full).  Every
// caller passes an int sample count or a bin total it has held below 2^30, so 2 n < 2^32: the 32-bit product
// `2u * (unsigned)n` of the sample-count sites and the 64-bit one of the bin-list sites were the same number, and the
// result, at most 2^31, fits an unsigned.
unsigned hash_table_size(long long n)
{
  unsigned table = 1024;
  while (table < 2ull * (unsigned long long)n)
    table <<= 1;
  return table;
}

// ------------------------------------------------------------------ profiling helpers
struct ProfScope
{
  bpf_engine* e;
  int idx = -1;
  ProfScope(bpf_engine* eng, int klass) : e(eng)
  {
    if (!e->profiling || e->ev_used >= e->ev_start.size() || !e->times_class(klass))
      return;
    idx = (int)e->ev_used++;
    e->ev_class[idx] = klass;
    (void)hipEventRecord(e->ev_start[idx], e->stream);
  }
  ~ProfScope()
  {
    if (idx >= 0)
      (void)hipEventRecord(e->ev_stop[idx], e->stream);
  }
};

// A kernel launch timed by events attached to the dispatch itself (hipExtLaunchKernelGGL): the elapsed time is the
// kernel's own start-to-end, without the marker packets and launch gap that hipEventRecord around a launch adds
// (~3.5 us), and agrees with the rocprofv3 kernel trace.  A timed dispatch costs the step ~5 us (completion signal
// with timestamps), so in mode 1 (scoring kernels only, used inside bench.py's timed region) every
// kTimedLaunchStride-th launch is timed, starting with the first after bpf_profile_reset; mode 3 times every scoring
// launch (for kernels of a millisecond or more, where 5 us do not show); mode 2 times all classes.  Falls back to a
// plain launch when profiling is off.
constexpr unsigned kTimedLaunchStride = 8;
#define LAUNCH_TIMED(e, klass, kernel, grid, block, lds, ...)                                                         \
  do                                                                                                                  \
  {                                                                                                                   \
    bpf_engine* _e = (e);                                                                                             \
    if (_e->profiling && _e->ev_used < _e->ev_start.size() && _e->times_class(klass) &&                               \
        (_e->profile_all || (_e->timed_launches++ % _e->timed_stride) == 0))                                          \
    {                                                                                                                 \
      const int _idx = (int)_e->ev_used++;                                                                            \
      _e->ev_class[_idx] = (klass);                                                                                   \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, _e->stream, _e->ev_start[_idx], _e->ev_stop[_idx], 0,           \
                            __VA_ARGS__);                                                                             \
    }                                                                                                                 \
    else                                                                                                              \
      hipLaunchKernelGGL(kernel, grid, block, lds, _e->stream, __VA_ARGS__);                                          \
  } while (0)

// ------------------------------------------------------------------ results published in pinned memory
// Waits for what `kernel_name` publishes in pinned host memory (host_poll.hpp): spins up to `ms`, then lets the stream
// drain (a mailbox wait may be running up to its bound) and looks once more.
template <class Ready>
int await_published(bpf_engine* e, Ready&& ready, int ms, const char* kernel_name)
{
  if (spin_until(ready, ms))
    return BPF_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (ready())
    return BPF_OK;
  return e->fail(BPF_ERR_HIP, std::string(kernel_name) + " did not publish its result");
}

// hipFuncAttributeMaxDynamicSharedMemorySize for a kernel that asks for more than the default 64 KB, once per engine
template <class Kernel>
int ensure_dynamic_lds(bpf_engine* e, Kernel* kernel, size_t bytes)
{
  const void* f = reinterpret_cast<const void*>(kernel);
  if (std::find(e->dynamic_lds_set.begin(), e->dynamic_lds_set.end(), f) != e->dynamic_lds_set.end())
    return BPF_OK;
  HIPCHK(e, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  e->dynamic_lds_set.push_back(f);
  return BPF_OK;
}

// BPF_DEBUG: the drivers' debug lines on stderr and the one-block kernels' phase clocks
bool debug_on()
{
  static const bool on = getenv("BPF_DEBUG") != nullptr;
  return on;
}

void lcg_tables(LcgJump& J)
{
  const uint64_t mask = (1ull << 48) - 1;
  uint64_t a = 0x5DEECE66Dull, c = 0xBull;
  for (int j = 0; j < 48; ++j)
  {
    J.A[j] = a;
    J.C[j] = c;
    c = (c * a + c) & mask;  // apply the step twice: x -> a*(a*x + c) + c
    a = (a * a) & mask;
  }
}

uint64_t lcg_skip_host(uint64_t x0, uint64_t n, const LcgJump& J)
{
  const uint64_t mask = (1ull << 48) - 1;
  uint64_t a = 1, c = 0;
  for (int j = 0; n != 0 && j < 48; ++j, n >>= 1)
    if (n & 1)
    {
      a = (a * J.A[j]) & mask;
      c = (c * J.A[j] + J.C[j]) & mask;
    }
  return (a * x0 + c) & mask;
}

int blocks_for(int n, int per_block)
{
  return (n + per_block - 1) / per_block;
}

// ------------------------------------------------------------------ map encoding
int encode_lut(bpf_engine* e, const float* lut)
{
  const int sx = e->map.size_x, sy = e->map.size_y;
  const size_t ncell = (size_t)sx * sy;
  std::unordered_map<uint32_t, int> seen;
  seen.reserve(4096);
  std::vector<float> levels;
  uint32_t last_bits = 0;
  bool have_last = false;
  for (size_t i = 0; i < ncell; ++i)
  {
    uint32_t bits;
    std::memcpy(&bits, &lut[i], 4);
    if (have_last && bits == last_bits)
      continue;
    last_bits = bits;
    have_last = true;
    if (seen.emplace(bits, 0).second)
    {
      levels.push_back(lut[i]);
      if (levels.size() > 8190)
        return e->fail(BPF_ERR_LUT_LEVELS, "distance LUT holds more than 8190 distinct values");
    }
  }
  std::sort(levels.begin(), levels.end());
  for (size_t k = 0; k < levels.size(); ++k)
  {
    uint32_t bits;
    std::memcpy(&bits, &levels[k], 4);
    seen[bits] = (int)k;
  }
  // padded image: a border cell all round, everything outside the map holds the off-map level K;
  // entries are level*8 (byte offset of the level's term in the per-scan table)
  const int tx = e->map.ltx, ty = e->map.lty;
  const uint16_t off_map_level = (uint16_t)(levels.size() * 8);
  std::vector<uint16_t> tiles((size_t)tx * ty * 64, off_map_level);
  for (int j = 0; j < sy; ++j)
  {
    uint32_t prev_bits = 0;
    int prev_idx = -1;
    for (int i = 0; i < sx; ++i)
    {
      uint32_t bits;
      std::memcpy(&bits, &lut[i + (size_t)j * sx], 4);
      if (prev_idx < 0 || bits != prev_bits)
      {
        prev_idx = seen[bits];
        prev_bits = bits;
      }
      const int u = i + 1, v = j + 1;
      tiles[((size_t)(v >> 3) * tx + (u >> 3)) * 64 + ((u & 7) << 3) + (v & 7)] = (uint16_t)(prev_idx * 8);
    }
  }
  HIPCHK(e, e->d_lut_tiles.reserve(tiles.size()));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_lut_tiles.p, tiles.data(), tiles.size() * sizeof(uint16_t)));
  HIPCHK(e, e->d_levels.reserve(levels.size() + 1));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_levels.p, levels.data(), levels.size() * sizeof(float)));
  HIPCHK(e, e->d_lut_f32.reserve(ncell));
  H2D_OR_RETURN(h2d_from_host_sync(e, e->d_lut_f32.p, lut, ncell * sizeof(float)));
  e->h_levels = levels;
  e->h_lut_f32.assign(lut, lut + ncell);
  e->map.lut_tiles = e->d_lut_tiles.p;
  e->map.levels = e->d_levels.p;
  e->map.n_levels = (int)levels.size();
  e->have_lut = true;
  e->map_version++;
  return BPF_OK;
}

int build_lut_device(bpf_engine* e, double max_dist)
{
  if (!e->have_map)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "no 2-D map set");
  if (max_dist == 0.0)
    return BPF_OK;  // occupancy_map.cpp:141-145: leaves the LUT untouched
  const int sx = e->map.size_x, sy = e->map.size_y;
  const size_t ncell = (size_t)sx * sy;
  const int radius = (int)std::floor(max_dist / e->map.resolution);
  HIPCHK(e, e->d_edt_tmp.reserve(ncell));
  HIPCHK(e, e->d_lut_f32.reserve(ncell));
  dim3 grid(blocks_for(sx, 256), sy), block(256);
  hipLaunchKernelGGL(k_edt_rows, grid, block, 0, e->stream, e->d_cells8.p, sx, sy, radius, e->d_edt_tmp.p);
  hipLaunchKernelGGL(k_edt_cols, grid, block, 0, e->stream, e->d_edt_tmp.p, sx, sy, radius, e->map.resolution,
                     max_dist, e->d_lut_f32.p);
  HIPCHK(e, hipGetLastError());
  std::vector<float> lut(ncell);
  H2D_OR_RETURN(d2h_to_host(e, lut.data(), e->d_lut_f32.p, ncell * sizeof(float), e->stream));
  e->map.max_dist = max_dist;
  return encode_lut(e, lut.data());
}
