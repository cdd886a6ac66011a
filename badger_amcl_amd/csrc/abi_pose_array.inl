// C-ABI: Node::publishParticleCloud's poses (node.cpp:335-357) formed on the device -- from the resident set, from the
// rows of a sharded set gathered by the caller's transport, or over the engine's own exchange in one collective call.
// Read-only for the filter: the set, its weights and everything cached about them stay as they were; the rows, the
// gathered rows and the formed poses live in buffers of their own (d_pa_*).
namespace
{
// samples a slice of n samples from global index global_first contributes to the selection first, first + stride, ...:
// the local index of the first one and how many
void pose_selection(long long global_first, long long n, long long first, long long stride, long long* i0_out,
                    long long* n_sel_out)
{
  const long long i0 = global_first >= first ? (stride - (global_first - first) % stride) % stride : first - global_first;
  *i0_out = i0;
  *n_sel_out = i0 < n ? (n - i0 + stride - 1) / stride : 0;
}

// poses 0 .. count-1 from an SoA source into d_pa_out and from there into the caller's memory (complete on return)
int pose_array_form(bpf_engine* e, const double* x, const double* y, const double* th, long long i0, long long stride,
                    int count, double* poses7_out)
{
  if (count == 0)
    return BPF_OK;
  HIPCHK(e, e->d_pa_out.reserve((size_t)7 * (size_t)count));
  hipLaunchKernelGGL(k_pose_array, dim3(blocks_for(count, kPoseBlock)), dim3(kPoseBlock), 0, e->stream, x, y, th, i0,
                     stride, count, e->d_pa_out.p);
  HIPCHK(e, hipGetLastError());
  // a registered destination is written by the copy engine, pageable memory through the bounce buffer
  return d2h_to_host(e, poses7_out, e->d_pa_out.p, (size_t)7 * (size_t)count * sizeof(double), e->stream);
}

// this slice's rows of the selection into d_pa_rows: int64[3][n_sel]
int pose_rows_local(bpf_engine* e, long long i0, long long stride, int n_sel)
{
  if (n_sel == 0)
    return BPF_OK;
  HIPCHK(e, e->d_pa_rows.reserve((size_t)3 * (size_t)n_sel));
  const SampleSet& s = e->sets[e->cur];
  hipLaunchKernelGGL(k_pose_rows, dim3(blocks_for(n_sel, 256)), dim3(256), 0, e->stream, s.x.p, s.y.p, s.th.p, i0,
                     stride, n_sel, e->d_pa_rows.p);
  HIPCHK(e, hipGetLastError());
  return BPF_OK;
}
}  // namespace

int bpf_pf_get_pose_array(bpf_engine* e, int first, int stride, double* poses7_out, int capacity, int* count_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (stride < 1 || first < 0 || !poses7_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose array: first >= 0, stride >= 1 and an output are needed");
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  const int n = e->sample_count;
  const int count = first < n ? (int)(((long long)n - first + stride - 1) / stride) : 0;
  if (capacity < count)
    return e->fail(BPF_ERR_CAPACITY, "pose array: output too small");
  HIPCHK(e, hipSetDevice(e->device));
  const SampleSet& s = e->sets[e->cur];
  const int rc = pose_array_form(e, s.x.p, s.y.p, s.th.p, first, stride, count, poses7_out);
  if (rc != BPF_OK)
    return rc;
  if (count_out)
    *count_out = count;
  return BPF_OK;
}

int bpf_shard_pose_rows_dev(bpf_engine* e, long long global_first, long long first, int stride, void** rows_dev,
                            int* n_rows_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (stride < 1 || first < 0 || global_first < 0 || !rows_dev || !n_rows_out)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose rows: first >= 0, global_first >= 0, stride >= 1, outputs needed");
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  long long i0 = 0, n_sel = 0;
  pose_selection(global_first, e->sample_count, first, stride, &i0, &n_sel);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, e->d_pa_rows.reserve(3));  // an empty selection still hands a pointer of the engine's back
  const int rc = pose_rows_local(e, i0, stride, (int)n_sel);
  if (rc != BPF_OK)
    return rc;
  *rows_dev = e->d_pa_rows.p;
  *n_rows_out = (int)n_sel;
  return BPF_OK;
}

int bpf_pose_array_from_rows_dev(bpf_engine* e, const void* rows_dev, long long row_stride, int n, double* poses7_out,
                                 int capacity)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (n < 0 || row_stride < n || (n > 0 && (!rows_dev || !poses7_out)))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose array from rows: n >= 0, row_stride >= n, rows and an output");
  if (capacity < n)
    return e->fail(BPF_ERR_CAPACITY, "pose array: output too small");
  HIPCHK(e, hipSetDevice(e->device));
  const double* rows = static_cast<const double*>(rows_dev);
  return pose_array_form(e, rows, rows + row_stride, rows + 2 * row_stride, 0, 1, n, poses7_out);
}

int bpf_shard_get_pose_array(bpf_engine* e, int root, long long first, int stride, double* poses7_out, int capacity,
                             int* count_out)
{
  if (!e)
    return BPF_ERR_INVALID_ARGUMENT;
  if (stride < 1 || first < 0)
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose array: first >= 0 and stride >= 1 are needed");
  if (!e->have_pf)
    return e->fail(BPF_ERR_NOT_CONFIGURED, "bpf_pf_create first");
  int rc = shard_step_ready(e);
  if (rc != BPF_OK)
    return rc;
  const int W = e->shard_world, rank = e->shard_rank;
  const bool receives = root < 0 || root == rank;
  if (root < -1 || root >= W || (receives && !poses7_out))
    return e->fail(BPF_ERR_INVALID_ARGUMENT, "pose array: root in [-1, world) and an output on a receiving rank");
  HIPCHK(e, hipSetDevice(e->device));
  ShardExchange X{ e };
  // the local sample counts; every rank derives every rank's first global index and contribution from them
  long long counts[kMailboxMaxWorld] = { 0 }, my_first = 0, n_global = 0;
  rc = shard_gather_counts(e, X, "pose array", counts, &my_first, &n_global);
  if (rc != BPF_OK)
    return rc;
  long long sel[kMailboxMaxWorld] = { 0 }, offs[kMailboxMaxWorld] = { 0 }, my_i0 = 0, at = 0, total = 0;
  for (int r = 0; r < W; ++r)
  {
    long long i0 = 0;
    pose_selection(at, counts[r], first, stride, &i0, &sel[r]);
    if (r == rank)
      my_i0 = i0;
    offs[r] = total;
    total += sel[r];
    at += counts[r];
  }
  if (total >= (1ll << 30))
    return e->fail(BPF_ERR_CAPACITY, "pose array: a selection beyond 2^30 poses");
  const int count = (int)total;
  if (count_out)
    *count_out = count;
  if (count == 0)
    return BPF_OK;  // on every rank alike: no second exchange
  // (mailbox: 3 * count words <= 6 * max_window since max_window >= max_samples; gather checks it all the same)
  rc = pose_rows_local(e, my_i0, stride, (int)sel[rank]);
  if (rc != BPF_OK)
    return rc;
  HIPCHK(e, e->d_pa_rows.reserve(3));
  HIPCHK(e, e->d_pa_gather.reserve((size_t)3 * (size_t)count));
  const long long* src[3] = { e->d_pa_rows.p, e->d_pa_rows.p + sel[rank], e->d_pa_rows.p + 2 * sel[rank] };
  rc = X.gather(src, 3, sel, e->d_pa_gather.p, offs, count);
  if (rc == BPF_OK)
    rc = X.finish();
  if (rc != BPF_OK)
    return rc;
  if (!receives)
    return BPF_OK;
  if (capacity < count)
    return e->fail(BPF_ERR_CAPACITY, "pose array: output too small");
  const double* rows = reinterpret_cast<const double*>(e->d_pa_gather.p);
  return pose_array_form(e, rows, rows + count, rows + 2 * (size_t)count, 0, 1, count, poses7_out);
}
