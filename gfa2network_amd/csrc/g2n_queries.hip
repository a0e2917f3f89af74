// g2n_queries.hip — the queries over a finished, device-resident CSR: graph statistics
// (g2n_csr_stats), component labels and the matrix regrouped by component (g2n_csr_components,
// g2n_csr_split_components_host: g2n_components.hip), hop distances between paths (g2n_csr_path_distances: g2n_dist.hip), weighted ones
// (g2n_csr_path_distances_weighted: g2n_wdist.hip), node-to-node distances (g2n_csr_pair_distances and
// its weighted twin: g2n_pairs.hip), and what a host build returns in place of its
// matrix when a stats / labels / distance / sequence-distance request is set (g2n_host.cpp).
//
// Part of g2n_pipeline.hip's translation unit, included where the host results begin: it uses that
// file's arena and stream helpers (dget, read_dev, scan_excl, shared_context, download) as they are.
#pragma once

namespace g2n {

// ------------------------------------------------------- what the queries share ------
template <int N>
struct Events {  // N events, destroyed with the scope
  hipEvent_t e[N] = {};
  void create() {
    for (auto& x : e) G2N_HIP(hipEventCreate(&x));
  }
  ~Events() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// f(indptr, indices) as int32_t or int64_t arrays
template <class F>
static void with_index_type(int32_t index_width, const void* indptr, const void* indices, F&& f) {
  if (index_width == 4) f((const int32_t*)indptr, (const int32_t*)indices);
  else f((const int64_t*)indptr, (const int64_t*)indices);
}

// f(T{}) with T the element type of a G2N dtype code (declared in g2n_pipeline.hip, whose builds call it too)
template <class F>
static void with_dtype(int dt, F&& f) {
  switch (dt) {
    case G2N_BOOL: f(uint8_t{}); break;
    case G2N_INT8: f(int8_t{}); break;
    case G2N_INT32: f(int32_t{}); break;
    case G2N_FLOAT32: f(float{}); break;
    default: f(double{}); break;
  }
}

// A CSR's description, before anything is read; `who` is the public function the messages name.
// ptrs_ok: the pointers the entry point needs whatever the sizes; entries_ok: those it needs when
// there are entries; need_rows: entries without rows are refused here (a _host entry leaves that to
// the device entry it calls, a distance call of no paths reads nothing).
static void check_csr(const std::string& who, int32_t index_width, uint64_t n, uint64_t nnz, bool ptrs_ok,
                      bool entries_ok, bool need_rows) {
  if (index_width != 4 && index_width != 8) throw Failure(G2N_E_ARG, who + ": index_width must be 4 or 8");
  if (n >= 0x7FFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^31-1 or more nodes");
  if (nnz >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^32-1 or more entries");
  if (!ptrs_ok || (nnz && !entries_ok)) throw Failure(G2N_E_ARG, who + ": null array");
  if (need_rows && n == 0 && nnz) throw Failure(G2N_E_ARG, who + ": entries without rows");
}

static void check_mode(const std::string& who, int32_t mode, bool weighted = false) {
  if (mode != G2N_DIST_MIN && mode != G2N_DIST_MEAN && !(weighted && mode == G2N_DIST_MEAN_FOLD))
    throw Failure(G2N_E_ARG, who + ": unknown mode");
}

// the number of steps, from path_ptr's two ends (path_ptr[0] == 0; what lies between is the device's to check)
static uint64_t path_steps(const std::string& who, int64_t first, int64_t last) {
  if (first != 0 || last < 0) throw Failure(G2N_E_ARG, who + ": path_ptr out of range");
  if ((uint64_t)last >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^32-1 or more steps");
  return (uint64_t)last;
}

// the same of a device path_ptr
static uint64_t path_steps_dev(g2n_context* c, const std::string& who, const int64_t* path_ptr, uint64_t K,
                               const int64_t* path_nodes) {
  int64_t ends[2];
  G2N_HIP(hipMemcpyAsync(&ends[0], path_ptr, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipMemcpyAsync(&ends[1], path_ptr + K, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  const uint64_t steps = path_steps(who, ends[0], ends[1]);
  if (steps && !path_nodes) throw Failure(G2N_E_ARG, who + ": null array");
  return steps;
}

// bytes of the K x K tables of one call, `cell` bytes a cell over all of them (hops: D uint32 = 4, or
// S and C uint64 = 16; weighted: D float64 = 8, or S float64 and C uint64 = 16); 0 = past 2^63
static uint64_t table_bytes(uint64_t K, uint64_t cell) {
  if (K >= (1ull << 29)) return 0;
  return K * K * cell;
}

// an output this library allocates (bytes; ~0 = past 2^63) must fit the device's free memory
static void check_fits(const std::string& who, uint64_t bytes, const std::string& what) {
  size_t f = 0, t = 0;
  G2N_HIP(hipMemGetInfo(&f, &t));
  if (bytes > f) throw Failure(G2N_E_UNSUPPORTED, who + ": " + what + " the device's free memory");
}

// the K x K tables of one call (and the batch's K done words)
static void check_tables(const std::string& who, uint64_t K, uint64_t cell) {
  const uint64_t want = table_bytes(K, cell);
  check_fits(who, K && !want ? ~0ull : want + K * 8, "the K x K tables of " + std::to_string(K) + " paths exceed");
}

// a _host entry point's call on the shared context of `device`: lock, open the call, f(c), trim
template <class F>
static int host_call(int32_t device, F&& f) {
  g2n_context* c = shared_context(device);
  std::lock_guard<std::mutex> lk(c->mu);
  enter_call(c);
  G2N_HIP(hipSetDevice(c->device));
  clear_call_state(c);
  f(c);
  shrink_shared(c);
  return G2N_OK;
}

struct StagedCsr {
  void *indptr, *indices;
  double* values;  // null without values
};

// a host CSR on c's stream (S_STIP / S_STIX, S_WVAL when there are values)
static StagedCsr stage_csr(g2n_context* c, const void* indptr, const void* indices, const double* values,
                           int32_t index_width, uint64_t n, uint64_t nnz) {
  const size_t w = (size_t)index_width;
  StagedCsr d{dbuf(c, S_STIP, (size_t)(n + 1) * w), dbuf(c, S_STIX, (size_t)nnz * w),
              values ? dget<double>(c, S_WVAL, nnz) : nullptr};
  G2N_HIP(hipMemcpyAsync(d.indptr, indptr, (size_t)(n + 1) * w, hipMemcpyHostToDevice, c->stream));
  if (nnz) G2N_HIP(hipMemcpyAsync(d.indices, indices, (size_t)nnz * w, hipMemcpyHostToDevice, c->stream));
  if (nnz && values) G2N_HIP(hipMemcpyAsync(d.values, values, (size_t)nnz * 8, hipMemcpyHostToDevice, c->stream));
  return d;
}

// --------------------------------------------------------- graph statistics ------
// g2n_csr_stats on c's stream (the caller holds c's lock and opened the call).
template <class I>
static void csr_stats_t(g2n_context* c, const I* indptr, const I* indices, uint64_t n, uint64_t nnz, bool directed,
                        StatsOut* so, hipEvent_t* ev) {
  auto* parent = dget<uint32_t>(c, S_STPARENT, n);
  auto* diag = dget<uint8_t>(c, S_STDIAG, n);
  uint32_t* colcnt = directed ? dget<uint32_t>(c, S_STCOL, n) : nullptr;
  const uint64_t long_cap = nnz / kStatsShortRow + 1;
  auto* long_rows = dget<uint32_t>(c, S_STLONG, long_cap);
  const unsigned g = grid_for(n);
  const unsigned gr = (unsigned)std::min<uint64_t>(g, (uint64_t)c->n_cu * 8);
  // ---- degrees (this walk also queues the long rows for both walks)
  G2N_HIP(hipEventRecord(ev[0], c->stream));
  G2N_HIP(hipMemsetAsync(diag, 0, n, c->stream));
  if (colcnt) G2N_HIP(hipMemsetAsync(colcnt, 0, n * sizeof(uint32_t), c->stream));
  const DegOp dop{diag, colcnt};
  hipLaunchKernelGGL((k_rows_short<I, DegOp>), dim3(g), dim3(256), 0, c->stream, indptr, indices, n, nnz, dop, 1,
                     long_rows, long_cap, so);
  hipLaunchKernelGGL((k_rows_long<I, DegOp>), dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices, n, nnz, dop,
                     (const uint32_t*)long_rows, long_cap, so);
  hipLaunchKernelGGL(k_deg_max<I>, dim3(gr), dim3(256), 0, c->stream, indptr, n, nnz, (const uint8_t*)diag,
                     (const uint32_t*)colcnt, so);
  G2N_HIP(hipEventRecord(ev[1], c->stream));
  // ---- components
  const HookOp hop{parent};
  hipLaunchKernelGGL(k_cc_init<I>, dim3(g), dim3(256), 0, c->stream, indptr, indices, n, nnz, parent, so);
  hipLaunchKernelGGL((k_rows_short<I, HookOp>), dim3(g), dim3(256), 0, c->stream, indptr, indices, n, nnz, hop, 0,
                     long_rows, long_cap, so);
  hipLaunchKernelGGL((k_rows_long<I, HookOp>), dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices, n, nnz, hop,
                     (const uint32_t*)long_rows, long_cap, so);
  hipLaunchKernelGGL(k_cc_flatten, dim3(gr), dim3(256), 0, c->stream, parent, n, so);
  G2N_HIP(hipEventRecord(ev[2], c->stream));
}

static StatsOut* stats_out_reset(g2n_context* c) {
  auto* so = dget<StatsOut>(c, S_STOUT, 1);
  G2N_HIP(hipMemsetAsync(so, 0, sizeof(StatsOut), c->stream));
  G2N_HIP(hipMemsetAsync(&so->high_off, 0xFF, sizeof(so->high_off), c->stream));
  return so;
}

static void csr_stats(g2n_context* c, const void* indptr, const void* indices, int32_t index_width, uint64_t n,
                      uint64_t nnz, int32_t directed, g2n_graph_stats* out) {
  std::memset(out, 0, sizeof(*out));
  check_csr("g2n_csr_stats", index_width, n, nnz, !n || indptr, indices, true);
  out->n_nodes = (int64_t)n;
  out->n_entries = (int64_t)nnz;
  if (n == 0) return;
  Events<3> ev;
  ev.create();
  StatsOut* so = stats_out_reset(c);
  with_index_type(index_width, indptr, indices,
                  [&](auto* ip, auto* ix) { csr_stats_t(c, ip, ix, n, nnz, directed != 0, so, ev.e); });
  const StatsOut h = read_dev(c, so);
  if (h.bad) throw Failure(G2N_E_ARG, "g2n_csr_stats: indptr / indices out of range");
  float ms = 0.f;
  G2N_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  out->ms_degree = ms;
  G2N_HIP(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
  out->ms_components = ms;
  out->n_diag = (int64_t)h.n_diag;
  out->n_components = (int64_t)h.n_roots;
  out->max_degree = (int64_t)h.max_degree;
}

int csr_stats_host(const void* indptr, const void* indices, int32_t index_width, uint64_t n, uint64_t nnz,
                   int32_t directed, int32_t device, g2n_graph_stats* out) {
  check_csr("g2n_csr_stats_host", index_width, n, nnz, indptr, indices, false);
  return host_call(device, [&](g2n_context* c) {
    const StagedCsr d = stage_csr(c, indptr, indices, nullptr, index_width, n, nnz);
    csr_stats(c, d.indptr, d.indices, index_width, n, nnz, directed, out);
  });
}

// ------------------------------------------------- components: labels and the split ------
// a call's events: union-find | labels | groups | split between ev[0..4]

template <class I>
static void cc_union_t(g2n_context* c, const I* indptr, const I* indices, uint64_t n, uint64_t nnz, uint32_t* parent,
                       StatsOut* so) {
  const uint64_t long_cap = nnz / kStatsShortRow + 1;
  auto* long_rows = dget<uint32_t>(c, S_STLONG, long_cap);
  const unsigned g = grid_for(n);
  const unsigned gr = (unsigned)std::min<uint64_t>(g, (uint64_t)c->n_cu * 8);
  const HookOp hop{parent};
  hipLaunchKernelGGL(k_cc_init<I>, dim3(g), dim3(256), 0, c->stream, indptr, indices, n, nnz, parent, so);
  hipLaunchKernelGGL((k_rows_short<I, HookOp>), dim3(g), dim3(256), 0, c->stream, indptr, indices, n, nnz, hop, 1,
                     long_rows, long_cap, so);
  hipLaunchKernelGGL((k_rows_long<I, HookOp>), dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices, n, nnz, hop,
                     (const uint32_t*)long_rows, long_cap, so);
  hipLaunchKernelGGL(k_cc_flatten, dim3(gr), dim3(256), 0, c->stream, parent, n, so);
}

// The labels of a device CSR (n > 0) into d_labels (int32, n) on c's stream; returns the number of
// components.  idx (n, or null): the identity, the sort's payload.  ev[0..2] are recorded.
static uint64_t csr_labels(g2n_context* c, const std::string& who, const void* indptr, const void* indices,
                           int32_t index_width, uint64_t n, uint64_t nnz, int32_t* d_labels, uint32_t* idx,
                           StatsOut* so, hipEvent_t* ev) {
  auto* parent = dget<uint32_t>(c, S_STPARENT, n);
  auto* flag = dget<uint32_t>(c, S_CCFLAG, n);
  auto* rank = dget<uint32_t>(c, S_CCRANK, n);
  auto* total = dget<uint32_t>(c, S_CCTOTAL, 1);
  G2N_HIP(hipEventRecord(ev[0], c->stream));
  with_index_type(index_width, indptr, indices, [&](auto* ip, auto* ix) { cc_union_t(c, ip, ix, n, nnz, parent, so); });
  G2N_HIP(hipEventRecord(ev[1], c->stream));
  // the walks checked every offset and index: nothing below runs on a CSR they objected to
  if (read_dev(c, so).bad) throw Failure(G2N_E_ARG, who + ": indptr / indices out of range");
  const unsigned g = grid_for(n);
  hipLaunchKernelGGL(k_cc_roots, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)parent, n, flag);
  scan_excl<uint32_t, uint32_t>(c, flag, rank, n, total);
  hipLaunchKernelGGL(k_cc_labels, dim3(g), dim3(256), 0, c->stream, (const uint32_t*)parent, (const uint32_t*)rank, n,
                     d_labels, idx);
  G2N_HIP(hipEventRecord(ev[2], c->stream));
  const uint64_t k = read_dev(c, total);
  if (k == 0 || k > n) throw Failure(G2N_E_DEVICE, who + ": component count out of range");
  return k;
}

static void components_times(g2n_components_info* info, hipEvent_t* ev, bool split) {
  float ms = 0.f;
  G2N_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  info->ms_union = ms;
  G2N_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
  info->ms_labels = ms;
  if (!split) return;
  G2N_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
  info->ms_group = ms;
  G2N_HIP(hipEventElapsedTime(&ms, ev[3], ev[4]));
  info->ms_split = ms;
}

static void csr_components(g2n_context* c, const std::string& who, const void* indptr, const void* indices,
                           int32_t index_width, uint64_t n, uint64_t nnz, int32_t* d_labels,
                           g2n_components_info* info) {
  std::memset(info, 0, sizeof(*info));
  check_csr(who, index_width, n, nnz, (!n || indptr) && (!n || d_labels), indices, true);
  if (n == 0) return;
  Events<5> ev;
  ev.create();
  StatsOut* so = stats_out_reset(c);
  info->n_components = (int64_t)csr_labels(c, who, indptr, indices, index_width, n, nnz, d_labels, nullptr, so, ev.e);
  components_times(info, ev.e, false);
}

int csr_components_host(const void* indptr, const void* indices, int32_t index_width, uint64_t n, uint64_t nnz,
                        int32_t* labels, int32_t device, g2n_components_info* info) {
  check_csr("g2n_csr_components_host", index_width, n, nnz, indptr && (!n || labels), indices, false);
  return host_call(device, [&](g2n_context* c) {
    const StagedCsr d = stage_csr(c, indptr, indices, nullptr, index_width, n, nnz);
    auto* dl = dget<int32_t>(c, S_CCLABEL, n);
    csr_components(c, "g2n_csr_components_host", d.indptr, d.indices, index_width, n, nnz, dl, info);
    if (n) G2N_HIP(hipMemcpyAsync(labels, dl, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
  });
}

template <class I, int VB>
static void split_copy_t(g2n_context* c, const I* indptr, const I* indices, const void* data, uint64_t n, uint64_t nnz,
                         const uint32_t* perm, const uint32_t* local, const int64_t* pos, void* out_indptr,
                         void* out_indices, void* out_data, StatsOut* so) {
  // the queues of longer rows: at most nnz / kSplitShortRow of them, of which nnz / kSplitHugeRow past the block's share
  const uint64_t long_cap = nnz / kSplitShortRow + 1, huge_cap = nnz / kSplitHugeRow + 1;
  auto* long_rows = dget<uint32_t>(c, S_STLONG, long_cap + huge_cap);
  uint32_t* huge_rows = long_rows + long_cap;
  auto* sq = dget<SplitQueues>(c, S_CCQUEUES, 1);
  G2N_HIP(hipMemsetAsync(sq, 0, sizeof(SplitQueues), c->stream));
  hipLaunchKernelGGL((k_split_short<I, VB>), dim3(grid_for(n + 1)), dim3(256), 0, c->stream, indptr, indices, data, n, nnz,
                     perm, local, pos, (I*)out_indptr, (I*)out_indices, out_data, long_rows, long_cap, huge_rows, huge_cap,
                     sq, so);
  hipLaunchKernelGGL((k_split_long<I, VB>), dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices, data, n, nnz,
                     perm, local, pos, (I*)out_indices, out_data, (const uint32_t*)long_rows, long_cap,
                     (const uint32_t*)huge_rows, huge_cap, (const SplitQueues*)sq, so);
}

int csr_split_components_host(const void* indptr, const void* indices, const void* data, int32_t value_bytes,
                              int32_t index_width, uint64_t n, uint64_t nnz, int32_t* labels, int64_t* perm, int64_t* off,
                              void* out_indptr, void* out_indices, void* out_data, int32_t device,
                              g2n_components_info* info) {
  const std::string who = "g2n_csr_split_components_host";
  std::memset(info, 0, sizeof(*info));
  if (value_bytes != 0 && value_bytes != 1 && value_bytes != 4 && value_bytes != 8)
    throw Failure(G2N_E_ARG, who + ": value_bytes must be 0, 1, 4 or 8");
  check_csr(who, index_width, n, nnz, indptr && off && out_indptr && (!n || (labels && perm)),
            indices && out_indices && (!value_bytes || (data && out_data)), true);
  if (n == 0) {
    off[0] = 0;
    std::memset(out_indptr, 0, (size_t)index_width);
    return G2N_OK;
  }
  return host_call(device, [&](g2n_context* c) {
    const size_t w = (size_t)index_width, vb = (size_t)value_bytes;
    const StagedCsr d = stage_csr(c, indptr, indices, nullptr, index_width, n, nnz);
    void* dval = vb ? dbuf(c, S_CCVAL, (size_t)nnz * vb) : nullptr;
    if (vb && nnz) G2N_HIP(hipMemcpyAsync(dval, data, (size_t)nnz * vb, hipMemcpyHostToDevice, c->stream));
    auto* dl = dget<int32_t>(c, S_CCLABEL, n);
    auto* idx = dget<uint32_t>(c, S_CCIDX, n);
    Events<5> ev;
    ev.create();
    StatsOut* so = stats_out_reset(c);
    const uint64_t k = csr_labels(c, who, d.indptr, d.indices, index_width, n, nnz, dl, idx, so, ev.e);
    info->n_components = (int64_t)k;
    // ---- groups: the nodes ordered by label, each label's first position
    auto* key_s = dget<uint32_t>(c, S_CCKEY, n);
    auto* dperm = dget<uint32_t>(c, S_CCPERM, n);
    auto* doff = dget<int64_t>(c, S_CCOFF, k + 1);
    sort_pairs_u32<uint32_t>(c, (const uint32_t*)dl, key_s, idx, dperm, n, bits_for(k));
    hipLaunchKernelGGL(k_cc_bounds, dim3(grid_for(n)), dim3(256), 0, c->stream, (const uint32_t*)key_s, n, k, doff);
    G2N_HIP(hipEventRecord(ev.e[3], c->stream));
    // ---- split: new row starts, then the copy
    auto* local = dget<uint32_t>(c, S_CCLOCAL, n);
    auto* len = dget<int64_t>(c, S_CCLEN, n + 1);
    auto* pos = dget<int64_t>(c, S_CCPOS, n + 1);
    auto* perm64 = dget<int64_t>(c, S_CCPERM64, n);
    void* oip = dbuf(c, S_CCOIP, (size_t)(n + 1) * w);
    void* oix = dbuf(c, S_CCOIX, (size_t)nnz * w);
    void* oval = vb ? dbuf(c, S_CCOVAL, (size_t)nnz * vb) : nullptr;
    with_index_type(index_width, d.indptr, d.indices, [&](auto* ip, auto* ix) {
      using I = std::remove_cv_t<std::remove_pointer_t<decltype(ip)>>;
      hipLaunchKernelGGL(k_split_rows<I>, dim3(grid_for(n + 1)), dim3(256), 0, c->stream, ip, n, nnz,
                         (const uint32_t*)dperm, (const uint32_t*)key_s, (const int64_t*)doff, k, local, len, perm64, so);
      excl_scan<int64_t>(c, len, pos, n + 1);
      const auto copy = [&](auto vbc) {
        split_copy_t<I, decltype(vbc)::value>(c, ip, ix, dval, n, nnz, dperm, local, pos, oip, oix, oval, so);
      };
      switch (value_bytes) {
        case 0: copy(std::integral_constant<int, 0>{}); break;
        case 1: copy(std::integral_constant<int, 1>{}); break;
        case 4: copy(std::integral_constant<int, 4>{}); break;
        default: copy(std::integral_constant<int, 8>{}); break;
      }
    });
    G2N_HIP(hipEventRecord(ev.e[4], c->stream));
    if (read_dev(c, so).bad) throw Failure(G2N_E_DEVICE, who + ": the split addressed out of range");
    G2N_HIP(hipMemcpyAsync(labels, dl, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipMemcpyAsync(perm, perm64, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipMemcpyAsync(off, doff, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipMemcpyAsync(out_indptr, oip, (size_t)(n + 1) * w, hipMemcpyDeviceToHost, c->stream));
    if (nnz) G2N_HIP(hipMemcpyAsync(out_indices, oix, (size_t)nnz * w, hipMemcpyDeviceToHost, c->stream));
    if (nnz && vb) G2N_HIP(hipMemcpyAsync(out_data, oval, (size_t)nnz * vb, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
    components_times(info, ev.e, true);
  });
}

// ------------------------------------------- distances: what the searches share ------
// The caller's arrays, checked whole on the device before anything is searched or written (values:
// null for hops): the CSR here, the caller's lists — `what` in the message — by the launches of lists(st).
template <class I, class Lists>
static void check_on_device(g2n_context* c, const std::string& who, const I* indptr, const I* indices,
                            const double* values, uint64_t n, uint64_t nnz, DistState* st, const char* what,
                            Lists&& lists) {
  const unsigned gcap = (unsigned)c->n_cu * 8;
  G2N_HIP(hipMemsetAsync(st, 0, sizeof(DistState), c->stream));
  hipLaunchKernelGGL(k_dist_check<I>, dim3(std::min(grid_for(std::max(n, nnz)), gcap)), dim3(256), 0, c->stream, indptr,
                     indices, n, nnz, st);
  if (values && nnz)
    hipLaunchKernelGGL(k_wdist_values, dim3(std::min(grid_for(nnz), gcap)), dim3(256), 0, c->stream, values, nnz, st);
  lists(st);
  if (read_dev(c, st).bad)
    throw Failure(G2N_E_ARG, who + ": indptr / indices / " + what + " out of range" +
                                 (values ? ", or a value that is negative or not finite" : ""));
}

// check_on_device's lists of a path search: the steps' paths into step_path and the nodes' step counts
// into cnt (n + 1, cleared here)
static auto path_lists(g2n_context* c, const int64_t* path_ptr, const int64_t* path_nodes, uint64_t K, uint64_t steps,
                       uint64_t n, uint32_t* step_path, uint32_t* cnt) {
  return [=](DistState* st) {
    G2N_HIP(hipMemsetAsync(cnt, 0, (n + 1) * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_dist_paths_check, dim3(grid_for(K)), dim3(256), 0, c->stream, path_ptr, K, steps, st);
    if (steps)
      hipLaunchKernelGGL(k_dist_steps, dim3(grid_for(steps)), dim3(256), 0, c->stream, path_ptr, path_nodes, K, steps, n,
                         step_path, cnt, st);
  };
}

// One batch's search from the sources already in next (any: there are some), level by level — a
// weighted search's level is its round (g2n_wdist.hip).  collect(L) launches the wide collect of
// level L's frontier, wide(count) the two wide expansions of its count nodes, narrow(budget) the
// one-workgroup kernel for up to budget levels; every launch is counted.  A correct search ends by
// level n (a hop level is at most n - 1, the last improving round too), so a frontier past that, or a
// narrow launch that did not advance within its budget, is a failure, not a reason to go on.
// Returns the deepest level at which anything was found.
template <class Collect, class Wide, class Narrow>
static uint32_t run_frontier(g2n_context* c, const std::string& who, DistState* st, uint64_t n, bool any,
                             int64_t* launches, Collect&& collect, Wide&& wide, Narrow&& narrow) {
  uint64_t L = 0;
  for (bool more = any; more;) {
    if (L > n) throw Failure(G2N_E_DEVICE, who + ": did not converge in n rounds");
    // wide: level L's frontier from next (count, n_long, pending cleared first)
    G2N_HIP(hipMemsetAsync(st, 0, 3 * sizeof(uint32_t), c->stream));
    collect((uint32_t)L);
    ++*launches;
    DistState h = read_dev(c, st);
    if (h.count == 0) break;
    if (h.count > kDistNarrowCap) {
      wide(h.count);
      *launches += 2;
      L++;
      continue;
    }
    // narrow: one workgroup carries it until it empties, overflows or has run its budget
    for (;;) {
      const uint32_t budget = (uint32_t)std::min<uint64_t>(kDistLevelBudget, n + 1 - L);  // (L <= n: >= 1)
      narrow(budget);
      ++*launches;
      h = read_dev(c, st);
      if (h.level <= L || h.level > L + budget) throw Failure(G2N_E_DEVICE, who + ": frontier state");
      L = h.level;
      if (h.pending) break;
      if (h.count == 0) {
        more = false;
        break;
      }
      if (h.count > kDistNarrowCap) throw Failure(G2N_E_DEVICE, who + ": frontier state");
      if (L > n) throw Failure(G2N_E_DEVICE, who + ": did not converge in n rounds");
    }
  }
  const DistState h = read_dev(c, st);
  if (h.bad) throw Failure(G2N_E_ARG, who + ": indptr / indices out of range");
  return h.last_level;
}

// what one search's frontier works in (the arena's S_D* slots); a weighted search has its distances beside it
struct SearchBufs {
  DistState* st;
  unsigned long long* next;
  uint32_t* queue;
  unsigned long long* qmask;
  uint32_t* long_rows;
  uint64_t long_cap;
};

static SearchBufs search_bufs(g2n_context* c, uint64_t n, uint64_t nnz) {
  SearchBufs w{};
  w.st = dget<DistState>(c, S_DSTATE, 1);
  w.next = dget<unsigned long long>(c, S_DNEXT, n);
  w.queue = dget<uint32_t>(c, S_DQUEUE, n);
  w.qmask = dget<unsigned long long>(c, S_DQMASK, n);
  w.long_cap = nnz / kStatsShortRow + 1;
  w.long_rows = dget<uint32_t>(c, S_DLONG, w.long_cap);
  return w;
}

// --------------------------------------------------------- hop searches ------
// what one hop search works in: the seen bits, then what every search does
struct HopBufs : SearchBufs {
  unsigned long long* seen;
};

static HopBufs hop_bufs(g2n_context* c, uint64_t n, uint64_t nnz) {
  auto* seen = dget<unsigned long long>(c, S_DSEEN, n);
  return {search_bufs(c, n, nnz), seen};
}

// n_batches batches of 64 hop searches each.  Per batch seen, next and the state are cleared; seed(k)
// sets batch k's sources in seen / next and returns whether it launched (false: the batch has none);
// collect(L) and narrow(budget) are run_frontier's, over the caller's accumulators.
template <class I, class Seed, class Collect, class Narrow>
static void hop_batches(g2n_context* c, const std::string& who, const I* indptr, const I* indices, uint64_t n,
                        uint64_t nnz, const HopBufs& b, uint64_t n_batches, g2n_dist_info* info, Seed&& seed,
                        Collect&& collect, Narrow&& narrow) {
  const unsigned gcap = (unsigned)c->n_cu * 8;
  int64_t launches = 0, levels = 0;
  for (uint64_t k = 0; k < n_batches; k++) {
    G2N_HIP(hipMemsetAsync(b.seen, 0, n * 8, c->stream));
    G2N_HIP(hipMemsetAsync(b.next, 0, n * 8, c->stream));
    G2N_HIP(hipMemsetAsync(b.st, 0, sizeof(DistState), c->stream));
    const bool any = seed(k);
    launches += any;
    const uint32_t last = run_frontier(
        c, who, b.st, n, any, &launches, collect,
        [&](uint32_t count) {
          hipLaunchKernelGGL(k_dist_expand<I>, dim3(std::min(grid_for(count), gcap)), dim3(256), 0, c->stream, indptr,
                             indices, n, nnz, b.seen, b.next, (const uint32_t*)b.queue, (const unsigned long long*)b.qmask,
                             b.long_rows, b.long_cap, b.st);
          hipLaunchKernelGGL(k_dist_expand_long<I>, dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices, n,
                             nnz, b.seen, b.next, (const uint32_t*)b.queue, (const unsigned long long*)b.qmask,
                             (const uint32_t*)b.long_rows, b.long_cap, b.st);
        },
        narrow);
    levels = std::max<int64_t>(levels, last);
  }
  info->levels = levels;
  info->launches = launches;
  info->batches = (int64_t)n_batches;
}

// A hop search's timed shell: search(indptr, indices) in the CSR's index type, its stream time into ms_bfs
template <class Search>
static void timed_hop_search(g2n_context* c, int32_t index_width, const void* indptr, const void* indices,
                             g2n_dist_info* info, Search&& search) {
  Events<2> ev;
  ev.create();
  G2N_HIP(hipEventRecord(ev.e[0], c->stream));
  with_index_type(index_width, indptr, indices, search);
  G2N_HIP(hipEventRecord(ev.e[1], c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  G2N_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  info->ms_bfs = ms;
}

// --------------------------------------------------------- path distances ------
// g2n_csr_path_distances on c's stream (the caller holds c's lock and opened the call); tables: device.
template <class I>
static void path_distances_t(g2n_context* c, const I* indptr, const I* indices, uint64_t n, uint64_t nnz,
                             const int64_t* path_ptr, const int64_t* path_nodes, uint64_t K, uint64_t steps, bool mean,
                             void* tables, g2n_dist_info* info) {
  const std::string who = "g2n_csr_path_distances";
  auto* st = dget<DistState>(c, S_DSTATE, 1);
  auto* cnt = dget<uint32_t>(c, S_DCNT, n + 1);
  auto* mem_ptr = dget<uint32_t>(c, S_DMPTR, n + 1);
  auto* cursor = dget<uint32_t>(c, S_DCUR, n + 1);
  auto* mem_path = dget<uint32_t>(c, S_DMPATH, steps);
  auto* step_path = dget<uint32_t>(c, S_DSPATH, steps);
  check_on_device(c, who, indptr, indices, (const double*)nullptr, n, nnz, st, "path_ptr / path_nodes",
                  path_lists(c, path_ptr, path_nodes, K, steps, n, step_path, cnt));
  // ---- membership: the steps sorted by node
  scan_excl<uint32_t, uint32_t>(c, cnt, mem_ptr, n + 1);
  G2N_HIP(hipMemcpyAsync(cursor, mem_ptr, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  if (steps)
    hipLaunchKernelGGL(k_dist_fill, dim3(grid_for(steps)), dim3(256), 0, c->stream, path_nodes, steps, n,
                       (const uint32_t*)step_path, cursor, mem_path);
  // ---- tables
  DistAcc acc{mem_ptr, mem_path, nullptr, nullptr, nullptr, nullptr, K, 0};
  if (mean) {
    acc.S = (unsigned long long*)tables;
    acc.C = acc.S + K * K;
    G2N_HIP(hipMemsetAsync(tables, 0, K * K * 16, c->stream));
  } else {
    acc.D = (uint32_t*)tables;
    acc.done = dget<unsigned long long>(c, S_DDONE, K);
    G2N_HIP(hipMemsetAsync(tables, 0xFF, K * K * 4, c->stream));
  }
  const HopBufs b = hop_bufs(c, n, nnz);
  std::vector<int64_t> h_ptr(K + 1);
  G2N_HIP(hipMemcpyAsync(h_ptr.data(), path_ptr, (K + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  const unsigned gn = std::min(grid_for(n), (unsigned)c->n_cu * 8);
  hop_batches(
      c, who, indptr, indices, n, nnz, b, (K + 63) / 64, info,
      [&](uint64_t k) {
        const uint64_t base = k * 64;
        const uint64_t s0 = (uint64_t)h_ptr[base], s1 = (uint64_t)h_ptr[std::min<uint64_t>(base + 64, K)];
        acc.base = (uint32_t)base;
        if (acc.done) G2N_HIP(hipMemsetAsync(acc.done, 0, K * 8, c->stream));
        if (s1 > s0)
          hipLaunchKernelGGL(k_dist_sources, dim3(grid_for(s1 - s0)), dim3(256), 0, c->stream, path_nodes, s0, s1, n,
                             (const uint32_t*)step_path, (uint32_t)base, b.seen, b.next);
        return s1 > s0;
      },
      [&](uint32_t L) {
        hipLaunchKernelGGL(k_dist_collect, dim3(gn), dim3(256), 0, c->stream, b.next, n, L, b.queue, b.qmask, acc, b.st);
      },
      [&](uint32_t budget) {
        hipLaunchKernelGGL(k_dist_narrow<I>, dim3(1), dim3(kDistNarrowTPB), 0, c->stream, indptr, indices, n, nnz, b.seen,
                           b.next, b.queue, b.qmask, acc, b.st, budget);
      });
}

static void path_distances(g2n_context* c, const void* indptr, const void* indices, int32_t index_width, uint64_t n,
                           uint64_t nnz, const int64_t* path_ptr, const int64_t* path_nodes, uint64_t K, int32_t mode,
                           void* tables, g2n_dist_info* info) {
  const std::string who = "g2n_csr_path_distances";
  std::memset(info, 0, sizeof(*info));
  check_mode(who, mode);
  check_csr(who, index_width, n, nnz, !K || (path_ptr && tables && (!n || indptr)), !K || indices, K != 0);
  if (K == 0) return;
  const uint64_t steps = path_steps_dev(c, who, path_ptr, K, path_nodes);
  timed_hop_search(c, index_width, indptr, indices, info, [&](auto* ip, auto* ix) {
    path_distances_t(c, ip, ix, n, nnz, path_ptr, path_nodes, K, steps, mode == G2N_DIST_MEAN, tables, info);
  });
}

// ------------------------------------------------ weighted path distances ------
// B searches a batch, of K wanted: B * n distances must fit what is free (and what the slot already holds)
static uint64_t wdist_batch_width(g2n_context* c, const std::string& who, uint64_t n, uint64_t K) {
  uint64_t B = std::min<uint64_t>(64, K);
  if (n) {
    size_t f = 0, t = 0;
    G2N_HIP(hipMemGetInfo(&f, &t));
    const uint64_t avail = (uint64_t)f + c->bufs[S_WDIST].cap;
    B = std::min<uint64_t>(B, avail / 10 * 8 / (n * 8));  // (the arena adds an eighth to what it is asked for)
    if (B == 0)
      throw Failure(G2N_E_UNSUPPORTED, who + ": the distances of one path over " + std::to_string(n) +
                                           " nodes exceed the device's free memory");
  }
  return B;
}

// One batch's weighted search, from the sources already in dist (0.0) and next (their bits; any: there
// are some): round R expands the nodes that round R - 1 improved (round 0: the sources).  Returns the
// last round that improved a distance.
template <class I>
static uint32_t wdist_search(g2n_context* c, const std::string& who, const I* indptr, const I* indices,
                             const double* values, uint64_t n, uint64_t nnz, uint64_t B, unsigned long long* dist,
                             const SearchBufs& w, bool any, int64_t* launches) {
  const unsigned gcap = (unsigned)c->n_cu * 8;
  const unsigned gn = std::min(grid_for(n), gcap);
  return run_frontier(
      c, who, w.st, n, any, launches,
      [&](uint32_t R) {
        hipLaunchKernelGGL(k_wdist_collect, dim3(gn), dim3(256), 0, c->stream, w.next, n, R, w.queue, w.qmask, w.st);
      },
      [&](uint32_t count) {
        hipLaunchKernelGGL(k_wdist_expand<I>, dim3(std::min(grid_for(count), gcap)), dim3(256), 0, c->stream, indptr,
                           indices, values, n, nnz, (uint32_t)B, dist, w.next, (const uint32_t*)w.queue,
                           (const unsigned long long*)w.qmask, w.long_rows, w.long_cap, w.st);
        hipLaunchKernelGGL(k_wdist_expand_long<I>, dim3(kStatsLongBlocks), dim3(256), 0, c->stream, indptr, indices,
                           values, n, nnz, (uint32_t)B, dist, w.next, (const uint32_t*)w.queue,
                           (const unsigned long long*)w.qmask, (const uint32_t*)w.long_rows, w.long_cap, w.st);
      },
      [&](uint32_t budget) {
        hipLaunchKernelGGL(k_wdist_narrow<I>, dim3(1), dim3(kDistNarrowTPB), 0, c->stream, indptr, indices, values, n,
                           nnz, (uint32_t)B, dist, w.next, w.queue, w.qmask, w.st, budget);
      });
}

// The K searches of one weighted call, B a batch (dist: n * B), batch k from search base(k) on.  Per
// batch dist is filled with inf and next and the state cleared; seed(base, nb) sets the nb searches'
// sources in dist / next and returns whether it launched (false: the batch has none); after the search
// tables(base, nb) launches the batch's part of the caller's tables and returns its launches.  ev: three
// events, ev[0] recorded by the caller before its checks — the first batch's search time holds them.
template <class I, class Base, class Seed, class Tables>
static void wdist_batches(g2n_context* c, const std::string& who, const I* indptr, const I* indices,
                          const double* values, uint64_t n, uint64_t nnz, uint64_t K, uint64_t B,
                          unsigned long long* dist, const SearchBufs& w, g2n_wdist_info* info, hipEvent_t* ev,
                          Base&& base_of, Seed&& seed, Tables&& tables) {
  const unsigned gcap = (unsigned)c->n_cu * 8;
  const uint64_t n_batches = (K + B - 1) / B;
  int64_t launches = 0, rounds = 0;
  double ms_search = 0.0, ms_tables = 0.0;
  for (uint64_t k = 0; k < n_batches; k++) {
    const uint64_t base = base_of(k);
    const uint64_t nb = std::min<uint64_t>(B, K - base);
    if (k) G2N_HIP(hipEventRecord(ev[0], c->stream));
    hipLaunchKernelGGL(k_wdist_fill, dim3(std::min(grid_for(n * B), gcap)), dim3(256), 0, c->stream, dist, n * B,
                       kWDistInf);
    G2N_HIP(hipMemsetAsync(w.next, 0, n * 8, c->stream));
    G2N_HIP(hipMemsetAsync(w.st, 0, sizeof(DistState), c->stream));
    launches++;
    const bool any = seed(base, nb);
    launches += any;
    const uint32_t last = wdist_search(c, who, indptr, indices, values, n, nnz, B, dist, w, any, &launches);
    rounds = std::max<int64_t>(rounds, last);
    G2N_HIP(hipEventRecord(ev[1], c->stream));
    launches += tables(base, nb);
    G2N_HIP(hipEventRecord(ev[2], c->stream));
    G2N_HIP(hipEventSynchronize(ev[2]));
    float ms = 0.f;
    G2N_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ms_search += ms;
    G2N_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    ms_tables += ms;
  }
  info->rounds = rounds;
  info->launches = launches;
  info->batches = (int64_t)n_batches;
  info->ms_search = ms_search;
  info->ms_tables = ms_tables;
}

// A weighted search's shell: search(indptr, indices, ev) in the CSR's index type, ev the three events
// of wdist_batches
template <class Search>
static void weighted_search(g2n_context* c, int32_t index_width, const void* indptr, const void* indices,
                            Search&& search) {
  Events<3> ev;
  ev.create();
  with_index_type(index_width, indptr, indices, [&](auto* ip, auto* ix) { search(ip, ix, ev.e); });
  G2N_HIP(hipStreamSynchronize(c->stream));
}

// g2n_csr_path_distances_weighted on c's stream (the caller holds c's lock and opened the call);
// tables: device.  Nothing is written to the tables before every array has passed its check.
template <class I>
static void wpath_distances_t(g2n_context* c, const I* indptr, const I* indices, const double* values, uint64_t n,
                              uint64_t nnz, const int64_t* path_ptr, const int64_t* path_nodes, uint64_t K,
                              uint64_t steps, int32_t mode, void* tables, g2n_wdist_info* info, hipEvent_t* ev) {
  const std::string who = "g2n_csr_path_distances_weighted";
  const bool mean = mode != G2N_DIST_MIN, fold = mode == G2N_DIST_MEAN_FOLD;
  const SearchBufs w = search_bufs(c, n, nnz);
  G2N_HIP(hipEventRecord(ev[0], c->stream));
  auto* cnt = dget<uint32_t>(c, S_DCNT, n + 1);
  auto* step_path = dget<uint32_t>(c, S_DSPATH, steps);
  check_on_device(c, who, indptr, indices, values, n, nnz, w.st, "path_ptr / path_nodes",
                  path_lists(c, path_ptr, path_nodes, K, steps, n, step_path, cnt));
  // ---- B paths a batch
  const uint64_t B = wdist_batch_width(c, who, n, K);
  auto* dist = dget<unsigned long long>(c, S_WDIST, n * B);
  info->batch_paths = (int64_t)B;
  // ---- tables
  auto* D = (unsigned long long*)tables;
  if (!mean)
    hipLaunchKernelGGL(k_wdist_fill, dim3(std::min(grid_for(K * K), (unsigned)c->n_cu * 8)), dim3(256), 0, c->stream, D,
                       K * K, kWDistInf);
  std::vector<int64_t> h_ptr(K + 1);
  G2N_HIP(hipMemcpyAsync(h_ptr.data(), path_ptr, (K + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  const uint64_t n_batches = (K + B - 1) / B;
  wdist_batches(
      c, who, indptr, indices, values, n, nnz, K, B, dist, w, info, ev,
      // (mean-fold: from the last batch to the first — a row's seeds are the rows below it, k_wdist_mean_fold)
      [&](uint64_t k) { return (fold ? n_batches - 1 - k : k) * B; },
      [&](uint64_t base, uint64_t nb) {
        const uint64_t s0 = (uint64_t)h_ptr[base], s1 = (uint64_t)h_ptr[base + nb];
        if (s1 > s0)
          hipLaunchKernelGGL(k_wdist_sources, dim3(grid_for(s1 - s0)), dim3(256), 0, c->stream, path_nodes, s0, s1, n,
                             (const uint32_t*)step_path, (uint32_t)base, (uint32_t)B, dist, w.next);
        return s1 > s0;
      },
      [&](uint64_t base, uint64_t nb) {  // the batch's rows of the tables
        if (mean) {
          hipLaunchKernelGGL(k_wdist_mean, dim3(grid_for(K * nb)), dim3(256), 0, c->stream, path_ptr, path_nodes, steps,
                             n, K, (const unsigned long long*)dist, (uint32_t)B, (uint32_t)nb, (uint32_t)base,
                             (double*)tables, D + K * K);
          if (fold)
            hipLaunchKernelGGL(k_wdist_mean_fold, dim3(grid_for(K * nb)), dim3(256), 0, c->stream, path_ptr, path_nodes,
                               steps, n, K, (const unsigned long long*)dist, (uint32_t)B, (uint32_t)nb, (uint32_t)base,
                               (double*)tables);
        } else if (steps)
          hipLaunchKernelGGL(k_wdist_min, dim3(grid_for(steps)), dim3(256), 0, c->stream, path_nodes, steps, n,
                             (const uint32_t*)step_path, K, (const unsigned long long*)dist, (uint32_t)B, (uint32_t)nb,
                             (uint32_t)base, D);
        return fold ? 2 : 1;  // (the min table's launch is counted even without steps)
      });
}

static void wpath_distances(g2n_context* c, const void* indptr, const void* indices, int32_t index_width,
                            const double* values, uint64_t n, uint64_t nnz, const int64_t* path_ptr,
                            const int64_t* path_nodes, uint64_t K, int32_t mode, void* tables, g2n_wdist_info* info) {
  const std::string who = "g2n_csr_path_distances_weighted";
  std::memset(info, 0, sizeof(*info));
  info->batch_paths = (int64_t)std::max<uint64_t>(1, std::min<uint64_t>(64, K));
  check_mode(who, mode, true);
  check_csr(who, index_width, n, nnz, !K || (path_ptr && tables && (!n || indptr)), !K || (indices && values), K != 0);
  if (K == 0) return;
  const uint64_t steps = path_steps_dev(c, who, path_ptr, K, path_nodes);
  weighted_search(c, index_width, indptr, indices, [&](auto* ip, auto* ix, hipEvent_t* ev) {
    wpath_distances_t(c, ip, ix, values, n, nnz, path_ptr, path_nodes, K, steps, mode, tables, info, ev);
  });
}

// A distance _host entry's call on the shared context: fits() checks the output against the free
// memory, the CSR is staged (values: null for hops), stage(c) puts the caller's two lists on the device
// (S_DPP / S_DPN) and returns them, search(c, csr, first, second, out) runs on them with the output in
// S_DTAB, and its `bytes` bytes are copied back.
template <class Fits, class Stage, class Search>
static int staged_call(int32_t device, const void* indptr, const void* indices, int32_t index_width,
                       const double* values, uint64_t n, uint64_t nnz, uint64_t bytes, void* out, Fits&& fits,
                       Stage&& stage, Search&& search) {
  return host_call(device, [&](g2n_context* c) {
    fits();
    const StagedCsr d = stage_csr(c, indptr, indices, values, index_width, n, nnz);
    const std::pair<const int64_t*, const int64_t*> lists = stage(c);
    void* dout = dbuf(c, S_DTAB, (size_t)bytes);
    search(c, d, lists.first, lists.second, dout);
    if (bytes) G2N_HIP(hipMemcpyAsync(out, dout, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
  });
}

// The two path _host entries: the paths in S_DPP / S_DPN, the tables `cell` bytes a cell;
// search(c, csr, path_ptr, path_nodes, tables).
template <class Search>
static int distances_host(const std::string& who, const void* indptr, const void* indices, int32_t index_width,
                          const double* values, bool weighted, uint64_t n, uint64_t nnz, const int64_t* path_ptr,
                          const int64_t* path_nodes, uint64_t K, int32_t mode, void* out_tables, int32_t device,
                          Search&& search) {
  check_mode(who, mode, weighted);
  check_csr(who, index_width, n, nnz, indptr && path_ptr && (!K || out_tables), indices && (!weighted || values), false);
  if (path_ptr[K] && !path_nodes) throw Failure(G2N_E_ARG, who + ": path_ptr out of range");
  const uint64_t steps = path_steps(who, path_ptr[0], path_ptr[K]);
  const uint64_t cell = mode != G2N_DIST_MIN ? 16 : weighted ? 8 : 4;
  return staged_call(
      device, indptr, indices, index_width, values, n, nnz, table_bytes(K, cell), out_tables,
      [&] { check_tables(who, K, cell); },
      [&](g2n_context* c) {
        auto* dpp = dget<int64_t>(c, S_DPP, K + 1);
        auto* dpn = dget<int64_t>(c, S_DPN, steps);
        G2N_HIP(hipMemcpyAsync(dpp, path_ptr, (size_t)(K + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (steps) G2N_HIP(hipMemcpyAsync(dpn, path_nodes, (size_t)steps * 8, hipMemcpyHostToDevice, c->stream));
        return std::make_pair((const int64_t*)dpp, (const int64_t*)dpn);
      },
      search);
}

int csr_path_distances_host(const void* indptr, const void* indices, int32_t index_width, uint64_t n, uint64_t nnz,
                            const int64_t* path_ptr, const int64_t* path_nodes, uint64_t K, int32_t mode,
                            void* out_tables, int32_t device, g2n_dist_info* info) {
  return distances_host("g2n_csr_path_distances_host", indptr, indices, index_width, nullptr, false, n, nnz, path_ptr,
                        path_nodes, K, mode, out_tables, device,
                        [&](g2n_context* c, const StagedCsr& d, const int64_t* dpp, const int64_t* dpn, void* dtab) {
                          path_distances(c, d.indptr, d.indices, index_width, n, nnz, dpp, dpn, K, mode, dtab, info);
                        });
}

int csr_path_distances_weighted_host(const void* indptr, const void* indices, int32_t index_width, const double* values,
                                     uint64_t n, uint64_t nnz, const int64_t* path_ptr, const int64_t* path_nodes,
                                     uint64_t K, int32_t mode, void* out_tables, int32_t device, g2n_wdist_info* info) {
  return distances_host("g2n_csr_path_distances_weighted_host", indptr, indices, index_width, values, true, n, nnz,
                        path_ptr, path_nodes, K, mode, out_tables, device,
                        [&](g2n_context* c, const StagedCsr& d, const int64_t* dpp, const int64_t* dpn, void* dtab) {
                          wpath_distances(c, d.indptr, d.indices, index_width, d.values, n, nnz, dpp, dpn, K, mode, dtab,
                                          info);
                        });
}

// ------------------------------------------------ node-to-node distances (g2n_pairs.hip) ------
static void check_pair_call(const std::string& who, int32_t mode, bool weighted, uint64_t n_src, uint64_t n_tgt) {
  if (mode != G2N_PAIR_TABLE && (weighted || mode != G2N_PAIR_SUMS)) throw Failure(G2N_E_ARG, who + ": unknown mode");
  if (n_src >= 0xFFFFFFFFull || n_tgt >= 0xFFFFFFFFull)
    throw Failure(G2N_E_UNSUPPORTED, who + ": 2^32-1 or more sources or targets");
}

// bytes of one call's output — sums: S and C, n_src uint64 each; table: n_src x n_tgt cells of 4 (hops)
// or 8 (weighted) bytes; ~0 = past 2^63
static uint64_t pair_out_bytes(int32_t mode, bool weighted, uint64_t n_src, uint64_t n_tgt) {
  if (mode == G2N_PAIR_SUMS) return n_src * 16;
  if (n_src && n_tgt > (1ull << 60) / n_src) return ~0ull;
  return n_src * n_tgt * (weighted ? 8 : 4);
}

static void check_pair_out(const std::string& who, uint64_t bytes) {
  check_fits(who, bytes, "the distance table exceeds");
}

// check_on_device's lists of a pair search: the targets' occurrences per node into tcnt (n + 1, cleared
// here; null: not wanted)
static auto pair_lists(g2n_context* c, const int64_t* sources, uint64_t n_src, const int64_t* targets, uint64_t n_tgt,
                       uint64_t n, uint32_t* tcnt) {
  return [=](DistState* st) {
    if (tcnt) G2N_HIP(hipMemsetAsync(tcnt, 0, (n + 1) * sizeof(uint32_t), c->stream));
    if (n_src)
      hipLaunchKernelGGL(k_pair_ids, dim3(grid_for(n_src)), dim3(256), 0, c->stream, sources, n_src, n,
                         (uint32_t*)nullptr, st);
    if (n_tgt)
      hipLaunchKernelGGL(k_pair_ids, dim3(grid_for(n_tgt)), dim3(256), 0, c->stream, targets, n_tgt, n, tcnt, st);
  };
}

// g2n_csr_pair_distances on c's stream (the caller holds c's lock and opened the call); out: device.
template <class I>
static void pair_distances_t(g2n_context* c, const I* indptr, const I* indices, uint64_t n, uint64_t nnz,
                             const int64_t* sources, uint64_t n_src, const int64_t* targets, uint64_t n_tgt, bool table,
                             void* out, g2n_dist_info* info) {
  const std::string who = "g2n_csr_pair_distances";
  auto* st = dget<DistState>(c, S_DSTATE, 1);
  auto* tcnt = dget<uint32_t>(c, S_DCNT, n + 1);
  check_on_device(c, who, indptr, indices, (const double*)nullptr, n, nnz, st, "sources / targets",
                  pair_lists(c, sources, n_src, targets, n_tgt, n, tcnt));
  PairAcc acc{};
  acc.n_tgt = n_tgt;
  if (table) {  // the targets' positions sorted by node
    auto* mem_ptr = dget<uint32_t>(c, S_DMPTR, n + 1);
    auto* cursor = dget<uint32_t>(c, S_DCUR, n + 1);
    auto* mem_pos = dget<uint32_t>(c, S_DMPATH, n_tgt);
    scan_excl<uint32_t, uint32_t>(c, tcnt, mem_ptr, n + 1);
    G2N_HIP(hipMemcpyAsync(cursor, mem_ptr, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if (n_tgt)
      hipLaunchKernelGGL(k_pair_fill, dim3(grid_for(n_tgt)), dim3(256), 0, c->stream, targets, n_tgt, n, cursor,
                         mem_pos);
    acc.mem_ptr = mem_ptr;
    acc.mem_pos = mem_pos;
    acc.D = (uint32_t*)out;
    if (n_src && n_tgt) G2N_HIP(hipMemsetAsync(out, 0xFF, n_src * n_tgt * 4, c->stream));
  } else {
    acc.tcnt = tcnt;
    acc.S = (unsigned long long*)out;
    acc.C = acc.S + n_src;
    if (n_src) G2N_HIP(hipMemsetAsync(out, 0, n_src * 16, c->stream));
  }
  const HopBufs b = hop_bufs(c, n, nnz);
  const unsigned gn = std::min(grid_for(n), (unsigned)c->n_cu * 8);
  hop_batches(
      c, who, indptr, indices, n, nnz, b, (n_src + 63) / 64, info,
      [&](uint64_t k) {  // (seeded whenever there are nodes: a batch of -1 ids alone is searched too)
        acc.base = k * 64;
        acc.nb = (uint32_t)std::min<uint64_t>(64, n_src - acc.base);
        if (n)
          hipLaunchKernelGGL(k_pair_sources, dim3(1), dim3(64), 0, c->stream, sources, acc.base, acc.base + acc.nb, n,
                             b.seen, b.next);
        return n != 0;
      },
      [&](uint32_t L) {
        if (table)
          hipLaunchKernelGGL(k_pair_collect<true>, dim3(gn), dim3(256), 0, c->stream, b.next, n, L, b.queue, b.qmask, acc,
                             b.st);
        else
          hipLaunchKernelGGL(k_pair_collect<false>, dim3(gn), dim3(256), 0, c->stream, b.next, n, L, b.queue, b.qmask,
                             acc, b.st);
      },
      [&](uint32_t budget) {
        if (table)
          hipLaunchKernelGGL((k_pair_narrow<I, true>), dim3(1), dim3(kDistNarrowTPB), 0, c->stream, indptr, indices, n,
                             nnz, b.seen, b.next, b.queue, b.qmask, acc, b.st, budget);
        else
          hipLaunchKernelGGL((k_pair_narrow<I, false>), dim3(1), dim3(kDistNarrowTPB), 0, c->stream, indptr, indices, n,
                             nnz, b.seen, b.next, b.queue, b.qmask, acc, b.st, budget);
      });
}

static void pair_distances(g2n_context* c, const void* indptr, const void* indices, int32_t index_width, uint64_t n,
                           uint64_t nnz, const int64_t* sources, uint64_t n_src, const int64_t* targets, uint64_t n_tgt,
                           int32_t mode, void* out, g2n_dist_info* info) {
  const std::string who = "g2n_csr_pair_distances";
  std::memset(info, 0, sizeof(*info));
  check_pair_call(who, mode, false, n_src, n_tgt);
  const bool wants_out = pair_out_bytes(mode, false, n_src, n_tgt) != 0;
  check_csr(who, index_width, n, nnz, (!n_src || sources) && (!n_tgt || targets) && (!wants_out || out) && (!n || indptr),
            indices, true);
  timed_hop_search(c, index_width, indptr, indices, info, [&](auto* ip, auto* ix) {
    pair_distances_t(c, ip, ix, n, nnz, sources, n_src, targets, n_tgt, mode == G2N_PAIR_TABLE, out, info);
  });
}

// g2n_csr_pair_distances_weighted on c's stream; out: device, n_src x n_tgt float64, not written unless
// every array passed its check.
template <class I>
static void wpair_distances_t(g2n_context* c, const I* indptr, const I* indices, const double* values, uint64_t n,
                              uint64_t nnz, const int64_t* sources, uint64_t n_src, const int64_t* targets,
                              uint64_t n_tgt, void* out, g2n_wdist_info* info, hipEvent_t* ev) {
  const std::string who = "g2n_csr_pair_distances_weighted";
  const SearchBufs w = search_bufs(c, n, nnz);
  G2N_HIP(hipEventRecord(ev[0], c->stream));
  check_on_device(c, who, indptr, indices, values, n, nnz, w.st, "sources / targets",
                  pair_lists(c, sources, n_src, targets, n_tgt, n, (uint32_t*)nullptr));
  if (n_src == 0 || n_tgt == 0) return;
  const uint64_t B = wdist_batch_width(c, who, n, n_src);
  auto* dist = dget<unsigned long long>(c, S_WDIST, n * B);
  info->batch_paths = (int64_t)B;
  wdist_batches(
      c, who, indptr, indices, values, n, nnz, n_src, B, dist, w, info, ev, [&](uint64_t k) { return k * B; },
      [&](uint64_t base, uint64_t nb) {
        if (n)
          hipLaunchKernelGGL(k_pair_wsources, dim3(1), dim3(64), 0, c->stream, sources, base, (uint32_t)nb, n,
                             (uint32_t)B, dist, w.next);
        return n != 0;
      },
      [&](uint64_t base, uint64_t nb) {
        hipLaunchKernelGGL(k_pair_wgather, dim3(std::min(grid_for(n_tgt * nb), (unsigned)c->n_cu * 8)), dim3(256), 0,
                           c->stream, targets, n_tgt, n, (const unsigned long long*)dist, (uint32_t)B, (uint32_t)nb, base,
                           (unsigned long long*)out);
        return 1;
      });
}

static void wpair_distances(g2n_context* c, const void* indptr, const void* indices, int32_t index_width,
                            const double* values, uint64_t n, uint64_t nnz, const int64_t* sources, uint64_t n_src,
                            const int64_t* targets, uint64_t n_tgt, void* out, g2n_wdist_info* info) {
  const std::string who = "g2n_csr_pair_distances_weighted";
  std::memset(info, 0, sizeof(*info));
  info->batch_paths = (int64_t)std::max<uint64_t>(1, std::min<uint64_t>(64, n_src));
  check_pair_call(who, G2N_PAIR_TABLE, true, n_src, n_tgt);
  check_csr(who, index_width, n, nnz,
            (!n_src || sources) && (!n_tgt || targets) && (!n_src || !n_tgt || out) && (!n || indptr), indices && values,
            true);
  weighted_search(c, index_width, indptr, indices, [&](auto* ip, auto* ix, hipEvent_t* ev) {
    wpair_distances_t(c, ip, ix, values, n, nnz, sources, n_src, targets, n_tgt, out, info, ev);
  });
}

// The two pair _host entries: the two lists in S_DPN (the sources, then the targets);
// search(c, csr, sources, targets, out).
template <class Search>
static int pairs_host(const std::string& who, const void* indptr, const void* indices, int32_t index_width,
                      const double* values, bool weighted, uint64_t n, uint64_t nnz, const int64_t* sources,
                      uint64_t n_src, const int64_t* targets, uint64_t n_tgt, int32_t mode, void* out, int32_t device,
                      Search&& search) {
  check_pair_call(who, mode, weighted, n_src, n_tgt);
  const uint64_t bytes = pair_out_bytes(mode, weighted, n_src, n_tgt);
  check_csr(who, index_width, n, nnz, indptr && (!n_src || sources) && (!n_tgt || targets) && (!bytes || out),
            indices && (!weighted || values), false);
  return staged_call(
      device, indptr, indices, index_width, values, n, nnz, bytes, out, [&] { check_pair_out(who, bytes); },
      [&](g2n_context* c) {
        auto* ids = dget<int64_t>(c, S_DPN, n_src + n_tgt);
        if (n_src) G2N_HIP(hipMemcpyAsync(ids, sources, (size_t)n_src * 8, hipMemcpyHostToDevice, c->stream));
        if (n_tgt) G2N_HIP(hipMemcpyAsync(ids + n_src, targets, (size_t)n_tgt * 8, hipMemcpyHostToDevice, c->stream));
        return std::make_pair((const int64_t*)ids, (const int64_t*)(ids + n_src));
      },
      search);
}

int csr_pair_distances_host(const void* indptr, const void* indices, int32_t index_width, uint64_t n, uint64_t nnz,
                            const int64_t* sources, uint64_t n_src, const int64_t* targets, uint64_t n_tgt, int32_t mode,
                            void* out, int32_t device, g2n_dist_info* info) {
  return pairs_host("g2n_csr_pair_distances_host", indptr, indices, index_width, nullptr, false, n, nnz, sources, n_src,
                    targets, n_tgt, mode, out, device,
                    [&](g2n_context* c, const StagedCsr& d, const int64_t* ds, const int64_t* dt, void* dout) {
                      pair_distances(c, d.indptr, d.indices, index_width, n, nnz, ds, n_src, dt, n_tgt, mode, dout, info);
                    });
}

int csr_pair_distances_weighted_host(const void* indptr, const void* indices, int32_t index_width, const double* values,
                                     uint64_t n, uint64_t nnz, const int64_t* sources, uint64_t n_src,
                                     const int64_t* targets, uint64_t n_tgt, void* out, int32_t device,
                                     g2n_wdist_info* info) {
  return pairs_host("g2n_csr_pair_distances_weighted_host", indptr, indices, index_width, values, true, n, nnz, sources,
                    n_src, targets, n_tgt, G2N_PAIR_TABLE, out, device,
                    [&](g2n_context* c, const StagedCsr& d, const int64_t* ds, const int64_t* dt, void* dout) {
                      wpair_distances(c, d.indptr, d.indices, index_width, d.values, n, nnz, ds, n_src, dt, n_tgt, dout,
                                      info);
                    });
}

// ------------------------------------------- a host build's result for a request ------
static thread_local const StatsRequest* t_stats_request = nullptr;
void set_stats_request(const StatsRequest* req) { t_stats_request = req; }
static thread_local const LabelsRequest* t_labels_request = nullptr;
void set_labels_request(const LabelsRequest* req) { t_labels_request = req; }
static thread_local const DistRequest* t_dist_request = nullptr;
void set_dist_request(const DistRequest* req) { t_dist_request = req; }
static thread_local const SeqRequest* t_seq_request = nullptr;
void set_seq_request(const SeqRequest* req) { t_seq_request = req; }
static thread_local bool t_last_build = false;
void set_last_build(bool on) { t_last_build = on; }

// A LAST build's stored values before a search: true when one is negative or not finite (the from-file
// weighted calls report it instead of searching: NetworkX's result then depends on its heap's order)
static bool bad_weights(g2n_context* c, const g2n_result& D) {
  if (D.dtype != G2N_FLOAT64) throw Failure(G2N_E_ARG, "weighted distances: the build returned no float64 values");
  if (!D.nnz) return false;
  auto* st = dget<DistState>(c, S_DSTATE, 1);
  G2N_HIP(hipMemsetAsync(st, 0, sizeof(DistState), c->stream));
  hipLaunchKernelGGL(k_wdist_values, dim3(std::min(grid_for((uint64_t)D.nnz), (unsigned)c->n_cu * 8)), dim3(256), 0,
                     c->stream, (const double*)D.data, (uint64_t)D.nnz, st);
  return read_dev(c, st).bad != 0;
}

// H's result as D's scalars, no matrix and no names (a stats or distance request's build)
static void scalars_result(g2n_context* c, const g2n_result& D, HostResult* H) {
  g2n_result& R = H->r;
  std::memcpy(&R, &D, sizeof(g2n_result));
  R.priv_ = H;
  R.err_detail = nullptr;
  R.names_blob = nullptr;
  R.names_offsets = nullptr;
  R.names_bytes = 0;
  R.rows = R.cols = R.indptr = R.indices = R.data = nullptr;
  if (D.err_detail) R.err_detail = (const uint8_t*)download(c, H->detail, D.err_detail, (size_t)D.err_detail_len);
  G2N_HIP(hipStreamSynchronize(c->stream));
}

// The graph path's ASCII decode of node keys after a clean build: true (H's result then carries
// G2N_E_UNICODE, err_line -1, the lowest such node id and its key) when a key has a byte >= 0x80.
static bool ascii_key_check(g2n_context* c, const g2n_result& D, HostResult* H) {
  g2n_result& R = H->r;
  if (!D.names_blob || !D.names_bytes || !D.n_nodes) return false;
  StatsOut* so = stats_out_reset(c);
  const unsigned g = (unsigned)std::min<uint64_t>(grid_for((D.names_bytes + 15) / 16), (uint64_t)c->n_cu * 8);
  hipLaunchKernelGGL(k_high_byte, dim3(g), dim3(256), 0, c->stream, D.names_blob, (uint64_t)D.names_bytes, so);
  hipLaunchKernelGGL(k_high_owner, dim3(1), dim3(64), 0, c->stream, D.names_offsets, (uint64_t)D.n_nodes, so);
  const StatsOut h = read_dev(c, so);
  if (h.high_off == ~0ull) return false;
  if (h.high_id < 0 || h.high_id >= D.n_nodes) throw Failure(G2N_E_DEVICE, "node keys: key lookup failed");
  int64_t span[2];
  G2N_HIP(hipMemcpyAsync(span, D.names_offsets + h.high_id, sizeof(span), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  R.err_detail = (const uint8_t*)download(c, H->detail, D.names_blob + span[0], (size_t)(span[1] - span[0]));
  G2N_HIP(hipStreamSynchronize(c->stream));
  R.err_detail_len = span[1] - span[0];
  R.status = G2N_E_UNICODE;
  R.err_line = -1;
  R.err_index = h.high_id;
  set_last_error("a node key is not ASCII (the graph path decodes node keys as ASCII)");
  return true;
}

// A stats build's result (g2n_stats_from_path): D's CSR stays on the device, the statistics are
// taken from it there, and H receives D's scalars — plus the one key the ASCII check objects to.
static void stats_result(g2n_context* c, const g2n_result& D, HostResult* H, const StatsRequest& q) {
  scalars_result(c, D, H);
  if (D.status != G2N_OK) return;
  if (D.format != G2N_FMT_CSR) throw Failure(G2N_E_ARG, "g2n_stats_from_path: the build returned no CSR");
  csr_stats(c, D.indptr, D.indices, D.index_width, (uint64_t)D.n_nodes, (uint64_t)D.nnz, q.directed, q.out);
  *q.n_paths = D.n_records - D.n_edges - (int64_t)c->last_n_segs;
  if (q.check_ascii) (void)ascii_key_check(c, D, H);
}

// A labels build's result (g2n_components_from_path): D's CSR stays on the device and is labelled
// there; H receives D's scalars, the labels (r.rows: int32, one per node) and the names.
static void labels_result(g2n_context* c, const g2n_result& D, HostResult* H, const LabelsRequest& q) {
  scalars_result(c, D, H);
  if (D.status != G2N_OK) return;
  if (D.format != G2N_FMT_CSR) throw Failure(G2N_E_ARG, "g2n_components_from_path: the build returned no CSR");
  const uint64_t n = (uint64_t)D.n_nodes;
  if (n && (!D.names_blob || !D.names_offsets)) throw Failure(G2N_E_DEVICE, "g2n_components_from_path: no names");
  if (q.check_ascii && ascii_key_check(c, D, H)) return;
  g2n_result& R = H->r;
  auto* dl = dget<int32_t>(c, S_CCLABEL, n);
  csr_components(c, "g2n_components_from_path", D.indptr, D.indices, D.index_width, n, (uint64_t)D.nnz, dl, q.info);
  R.rows = download(c, H->rows, dl, (size_t)n * 4);
  if (n) {
    const int64_t* offs = (const int64_t*)download(c, H->offs, D.names_offsets, (size_t)(n + 1) * sizeof(int64_t));
    G2N_HIP(hipStreamSynchronize(c->stream));
    R.names_blob = (const uint8_t*)download(c, H->blob, D.names_blob, (size_t)offs[n]);
    R.names_offsets = offs;
    R.names_bytes = D.names_bytes;
  }
  G2N_HIP(hipStreamSynchronize(c->stream));
}

// What a distance or sequence-distance build's result begins with: H receives D's scalars; false = the
// result is complete (the build failed, or the ASCII check objected to a key).  D's CSR and names stay
// on the device — the names are downloaded too when names_if_high and one has a byte >= 0x80.
static bool names_on_device(g2n_context* c, const g2n_result& D, HostResult* H, const std::string& who,
                            bool check_ascii, bool names_if_high) {
  scalars_result(c, D, H);
  if (D.status != G2N_OK) return false;
  if (D.format != G2N_FMT_CSR) throw Failure(G2N_E_ARG, who + ": the build returned no CSR");
  const uint64_t n = (uint64_t)D.n_nodes;
  if (n && (!D.names_blob || !D.names_offsets)) throw Failure(G2N_E_DEVICE, who + ": no names");
  if (check_ascii && ascii_key_check(c, D, H)) return false;
  if (names_if_high && n && D.names_bytes) {
    StatsOut* so = stats_out_reset(c);
    const unsigned g = (unsigned)std::min<uint64_t>(grid_for((D.names_bytes + 15) / 16), (uint64_t)c->n_cu * 8);
    hipLaunchKernelGGL(k_high_byte, dim3(g), dim3(256), 0, c->stream, D.names_blob, (uint64_t)D.names_bytes, so);
    if (read_dev(c, so).high_off != ~0ull) {
      g2n_result& R = H->r;
      const int64_t* offs = (const int64_t*)download(c, H->offs, D.names_offsets, (size_t)(n + 1) * sizeof(int64_t));
      G2N_HIP(hipStreamSynchronize(c->stream));
      R.names_blob = (const uint8_t*)download(c, H->blob, D.names_blob, (size_t)offs[n]);
      R.names_offsets = offs;
      R.names_bytes = D.names_bytes;
      G2N_HIP(hipStreamSynchronize(c->stream));
    }
  }
  return true;
}

struct NameTable {
  const KsEntry* table;  // over the names' own blob: ids = node ids
  uint64_t mask;
  unsigned long long* flags;  // S_DFLAG, two words: [0] becomes non-zero when a key is oriented, [1] the caller's
};

// the orientation flag and the key table over the names' own blob, launched on c's stream
static NameTable name_table(g2n_context* c, const g2n_result& D) {
  const uint64_t n = (uint64_t)D.n_nodes;
  auto* flags = dget<unsigned long long>(c, S_DFLAG, 2);
  G2N_HIP(hipMemsetAsync(flags, 0, 8, c->stream));
  if (n)
    hipLaunchKernelGGL(k_key_oriented, dim3(std::min(grid_for(n), (unsigned)c->n_cu * 8)), dim3(256), 0, c->stream,
                       D.names_blob, D.names_offsets, n, (uint32_t*)flags);
  uint64_t cap = 1024;
  while (cap < 2 * n) cap *= 2;
  auto* table = dget<KsEntry>(c, S_DKS, cap);
  G2N_HIP(hipMemsetAsync(table, 0xFF, cap * sizeof(KsEntry), c->stream));
  if (n)
    hipLaunchKernelGGL(k_ks_insert, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, D.names_blob, D.names_offsets, n,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const int64_t*)nullptr, (uint64_t)0,
                       (uint64_t)0, table, cap - 1, (uint8_t*)nullptr, (int64_t*)nullptr, (uint32_t*)nullptr, 1);
  return {table, cap - 1, flags};
}

// A distance build's result (g2n_distances_from_path): the names go into a key table over their own
// blob, the request's step names are looked up in it in one launch, and g2n_csr_path_distances runs
// on the ids.
static void dist_result(g2n_context* c, const g2n_result& D, HostResult* H, const DistRequest& q) {
  const std::string who = q.pairs ? "g2n_pair_distances_from_path" : "g2n_distances_from_path";
  *q.oriented = 0;
  *q.missing_step = -1;
  const bool weighted = q.winfo != nullptr;
  if (weighted) {
    *q.bad_weight = 0;
    std::memset(q.winfo, 0, sizeof(*q.winfo));
  }
  if (!names_on_device(c, D, H, who, q.check_ascii, q.names_if_high)) return;
  const uint64_t n = (uint64_t)D.n_nodes;
  if (q.n_steps >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^32-1 or more steps");
  if (weighted && bad_weights(c, D)) {  // the graph is refused as a whole, before any step is looked up
    *q.bad_weight = 1;
    return;
  }
  // (a pair request: the source's steps are the sources, the target's the targets — g2n_pair_distances_from_path)
  const uint64_t n_a = q.n_source_steps, n_b = q.n_steps - q.n_source_steps;
  const uint64_t cell = q.mode != G2N_DIST_MIN ? 16 : weighted ? 8 : 4;
  if (q.pairs) {
    check_pair_call(who, q.mode, weighted, n_a, n_b);
    check_pair_out(who, pair_out_bytes(q.mode, weighted, n_a, n_b));
  } else {
    check_tables(who, q.K, cell);
  }
  Events<2> ev;
  ev.create();
  G2N_HIP(hipEventRecord(ev.e[0], c->stream));
  // ---- the orientation flag, the key table, and the steps looked up in it
  const NameTable nt = name_table(c, D);
  G2N_HIP(hipMemsetAsync(nt.flags + 1, 0xFF, 8, c->stream));  // the first missing source step
  const uint64_t sbytes = (uint64_t)q.step_offs[q.n_steps];
  auto* sblob = dget<uint8_t>(c, S_DSBLOB, sbytes + 16);
  auto* soffs = dget<int64_t>(c, S_DSOFFS, q.n_steps + 1);
  auto* ids = dget<uint32_t>(c, S_DIDS, q.n_steps);
  auto* fresh = dget<uint32_t>(c, S_DCUR, q.n_steps);  // (scratch: path_distances_t takes the slot afterwards)
  auto* dpp = dget<int64_t>(c, S_DPP, q.K + 1);
  auto* dpn = dget<int64_t>(c, S_DPN, q.n_steps);
  if (sbytes) G2N_HIP(hipMemcpyAsync(sblob, q.step_blob, sbytes, hipMemcpyHostToDevice, c->stream));
  G2N_HIP(hipMemcpyAsync(soffs, q.step_offs, (q.n_steps + 1) * 8, hipMemcpyHostToDevice, c->stream));
  G2N_HIP(hipMemcpyAsync(dpp, q.path_ptr, (q.K + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (q.n_steps) {
    hipLaunchKernelGGL(k_ks_lookup, dim3(grid_for(q.n_steps, 256)), dim3(256), 0, c->stream, (const uint8_t*)sblob,
                       (const int64_t*)soffs, q.n_steps, nt.table, nt.mask, D.names_blob, ids, fresh);
    hipLaunchKernelGGL(k_dist_resolved, dim3(grid_for(q.n_steps)), dim3(256), 0, c->stream, (const uint32_t*)ids,
                       q.n_steps, q.n_source_steps, dpn, nt.flags + 1);
  }
  G2N_HIP(hipEventRecord(ev.e[1], c->stream));
  unsigned long long h[2];
  G2N_HIP(hipMemcpyAsync(h, nt.flags, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  *q.oriented = (uint32_t)h[0] != 0;
  float ms = 0.f;
  G2N_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  if (h[1] != ~0ull) {
    *q.missing_step = (int64_t)h[1];
    if (!weighted) {
      std::memset(q.info, 0, sizeof(*q.info));
      q.info->ms_resolve = ms;
    }
    return;
  }
  const uint64_t tbytes = q.pairs ? pair_out_bytes(q.mode, weighted, n_a, n_b) : table_bytes(q.K, cell);
  void* dtab = dbuf(c, S_DTAB, (size_t)tbytes);
  if (q.pairs && weighted) {
    wpair_distances(c, D.indptr, D.indices, D.index_width, (const double*)D.data, n, (uint64_t)D.nnz, dpn, n_a,
                    dpn + n_a, n_b, dtab, q.winfo);
  } else if (q.pairs) {
    pair_distances(c, D.indptr, D.indices, D.index_width, n, (uint64_t)D.nnz, dpn, n_a, dpn + n_a, n_b, q.mode, dtab,
                   q.info);
    q.info->ms_resolve = ms;
  } else if (weighted) {
    wpath_distances(c, D.indptr, D.indices, D.index_width, (const double*)D.data, n, (uint64_t)D.nnz, dpp, dpn, q.K,
                    q.mode, dtab, q.winfo);
  } else {
    path_distances(c, D.indptr, D.indices, D.index_width, n, (uint64_t)D.nnz, dpp, dpn, q.K, q.mode, dtab, q.info);
    q.info->ms_resolve = ms;
  }
  if (tbytes && q.tables) G2N_HIP(hipMemcpyAsync(q.tables, dtab, (size_t)tbytes, hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
}

// The end of a sequence search: cell [0][1] of the K = 2 table (device) and what the search reported
template <class T>
static void seq_search_end(g2n_context* c, const T* dtab, T* cell, g2n_seq_info* info, int64_t levels, int64_t launches,
                           int64_t batches, double ms) {
  T tab[4];
  G2N_HIP(hipMemcpyAsync(tab, dtab, sizeof(tab), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  *cell = tab[1];
  info->levels = levels;
  info->launches = launches;
  info->batches = batches;
  info->ms_bfs = ms;
}

// A sequence-distance build's result (g2n_seq_distance_from_path): the S records of the staged
// input in[0, len) give the two lists of node ids (g2n_seq.hip), their names looked up in the key
// table, and g2n_csr_path_distances searches the lists as K = 2.
static void seq_result(g2n_context* c, const g2n_result& D, HostResult* H, const SeqRequest& q, const uint8_t* in,
                       uint64_t len) {
  const std::string who = "g2n_seq_distance_from_path";
  *q.oriented = 0;
  if (q.wdist) {
    *q.wdist = __builtin_inf();
    *q.bad_weight = 0;
  } else {
    *q.dist = kDistUnreached;
  }
  std::memset(q.info, 0, sizeof(*q.info));
  *q.hits = g2n_seq_hits();
  if (!names_on_device(c, D, H, who, q.check_ascii, q.names_if_high)) return;
  if (q.wdist && bad_weights(c, D)) {  // the graph is refused as a whole, before any sequence is matched
    *q.bad_weight = 1;
    return;
  }
  const uint64_t n = (uint64_t)D.n_nodes;
  const uint64_t n_s = c->last_n_segs;
  if (n_s >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^32-1 or more S lines");
  Events<3> ev;
  ev.create();
  const unsigned gcap = (unsigned)c->n_cu * 8;
  // ---- the line starts "S\t": the one pass over every byte
  auto* st = dget<SeqState>(c, S_QSTATE, 1);
  auto* lines = dget<uint64_t>(c, S_QLINES, n_s);
  G2N_HIP(hipMemsetAsync(st, 0, sizeof(SeqState), c->stream));
  G2N_HIP(hipEventRecord(ev.e[0], c->stream));
  if (len)
    hipLaunchKernelGGL(k_seq_lines, dim3(std::min(grid_for((len + 15) / 16), gcap)), dim3(256), 0, c->stream, in, len,
                       n_s, lines, st);
  G2N_HIP(hipEventRecord(ev.e[1], c->stream));
  const NameTable nt = name_table(c, D);
  if (read_dev(c, st).n_lines != n_s)
    throw Failure(G2N_E_DEVICE, who + ": the S lines found differ from the build's count");
  // ---- the queries: one holding a tab or a newline equals no field; the bytes past the first 16
  // are read on the device only by k_seq_compare
  SeqQuery sq{};
  uint64_t qoff[2] = {0, 0}, qbytes = 0;
  for (int k = 0; k < 2; k++) {
    const uint8_t* s = q.seq[k];
    const uint64_t m = q.len[k];
    const bool never = m && (std::memchr(s, '\t', m) || std::memchr(s, '\n', m));
    sq.m[k] = never ? kSeqNoQuery : m;
    if (never) continue;
    if (m) std::memcpy(sq.head[k], s, (size_t)std::min<uint64_t>(m, kSeqHead));
    if (m > kSeqHead) {
      qoff[k] = qbytes;
      qbytes += (m + 15) & ~15ull;
    }
  }
  auto* dq = dget<uint8_t>(c, S_QBYTES, qbytes);
  for (int k = 0; k < 2; k++)
    if (sq.m[k] != kSeqNoQuery && sq.m[k] > kSeqHead)
      G2N_HIP(hipMemcpyAsync(dq + qoff[k], q.seq[k], (size_t)sq.m[k], hipMemcpyHostToDevice, c->stream));
  // ---- one lane per S line, the long candidates' remaining bytes, the node lists
  auto* node_of = dget<uint32_t>(c, S_QNODE, n_s);
  auto* fpos = dget<uint64_t>(c, S_QFPOS, n_s);
  auto* flags = dget<uint32_t>(c, S_QFLAG, n_s);
  auto* last = dget<unsigned long long>(c, S_QLAST, n);
  auto* cand = dget<uint32_t>(c, S_QCAND, 2 * n_s);
  auto* ids = dget<uint32_t>(c, S_QIDS, 2 * n_s);
  G2N_HIP(hipMemsetAsync(last, 0, n * 8, c->stream));
  SeqState h{};
  if (n_s) {
    hipLaunchKernelGGL(k_seq_classify, dim3(grid_for(n_s, 256)), dim3(256), 0, c->stream, in, len,
                       (const uint64_t*)lines, n_s, nt.table, nt.mask, D.names_blob, n, sq, node_of, fpos, flags, last,
                       cand, cand + n_s, st);
    h = read_dev(c, st);
    if (h.bad) throw Failure(G2N_E_DEVICE, who + ": an S name is no node");
    for (int k = 0; k < 2; k++)
      if (sq.m[k] != kSeqNoQuery && sq.m[k] > kSeqHead && h.cand[k])
        hipLaunchKernelGGL(k_seq_compare, dim3(std::min<unsigned>(h.cand[k], gcap)), dim3(256), 0, c->stream, in, len,
                           (const uint8_t*)(dq + qoff[k]), sq.m[k], kSeqCand << k, (const uint32_t*)(cand + k * n_s),
                           (uint64_t)h.cand[k], (const uint64_t*)fpos, flags);
    hipLaunchKernelGGL(k_seq_nodes, dim3(grid_for(n_s, 256)), dim3(256), 0, c->stream, (const uint64_t*)lines, n_s,
                       (const uint32_t*)node_of, (const uint32_t*)flags, (const unsigned long long*)last, ids, ids + n_s,
                       st);
    h = read_dev(c, st);
  }
  G2N_HIP(hipEventRecord(ev.e[2], c->stream));
  unsigned long long oriented = 0;
  G2N_HIP(hipMemcpyAsync(&oriented, nt.flags, 8, hipMemcpyDeviceToHost, c->stream));
  // ---- the two lists, ascending (the appends' order is arbitrary)
  std::vector<uint32_t> got[2];
  for (int k = 0; k < 2; k++) {
    if (h.hits[k] > n_s) throw Failure(G2N_E_DEVICE, who + ": node list overflow");
    got[k].resize(h.hits[k]);
    if (h.hits[k])
      G2N_HIP(hipMemcpyAsync(got[k].data(), ids + k * n_s, (size_t)h.hits[k] * 4, hipMemcpyDeviceToHost, c->stream));
  }
  G2N_HIP(hipStreamSynchronize(c->stream));
  *q.oriented = (uint32_t)oriented != 0;
  std::vector<int64_t> pn;
  for (int k = 0; k < 2; k++) {
    std::sort(got[k].begin(), got[k].end());
    q.hits->ids[k].assign(got[k].begin(), got[k].end());
    pn.insert(pn.end(), got[k].begin(), got[k].end());
  }
  float ms_scan = 0.f, ms_match = 0.f;
  G2N_HIP(hipEventElapsedTime(&ms_scan, ev.e[0], ev.e[1]));
  G2N_HIP(hipEventElapsedTime(&ms_match, ev.e[1], ev.e[2]));
  q.info->n_s_lines = (int64_t)n_s;
  q.info->n_with_seq = (int64_t)h.n_with_seq;
  q.info->candidates_a = (int64_t)h.cand[0];
  q.info->candidates_b = (int64_t)h.cand[1];
  q.info->ms_scan = ms_scan;
  q.info->ms_match = ms_match;
  // ---- the listed nodes' keys (A's, then B's)
  const uint64_t T = pn.size();
  auto* dpn = dget<int64_t>(c, S_DPN, T);
  std::vector<int64_t>& noffs = q.hits->name_offs;
  noffs.assign(T + 1, 0);
  if (T) {
    auto* dlens = dget<int64_t>(c, S_QNLEN, T);
    auto* doffs = dget<int64_t>(c, S_QNOFF, T + 1);
    G2N_HIP(hipMemcpyAsync(dpn, pn.data(), T * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_seq_hit_lens, dim3(grid_for(T, 256)), dim3(256), 0, c->stream, (const int64_t*)dpn, T, n,
                       D.names_offsets, dlens);
    G2N_HIP(hipMemcpyAsync(noffs.data() + 1, dlens, T * 8, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < T; i++) {
      if (noffs[i + 1] < 0 || noffs[i + 1] > D.names_bytes) throw Failure(G2N_E_DEVICE, who + ": key length out of range");
      noffs[i + 1] += noffs[i];
    }
    const uint64_t nbytes = (uint64_t)noffs[T];
    auto* dblob = dget<uint8_t>(c, S_QNBLOB, nbytes);
    q.hits->names.resize(nbytes);
    G2N_HIP(hipMemcpyAsync(doffs, noffs.data(), (T + 1) * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_seq_hit_names, dim3(grid_for(T, 256)), dim3(256), 0, c->stream, (const int64_t*)dpn, T, n,
                       D.names_offsets, D.names_blob, (const int64_t*)doffs, dblob);
    if (nbytes) G2N_HIP(hipMemcpyAsync(q.hits->names.data(), dblob, nbytes, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
  }
  if (got[0].empty() || got[1].empty()) return;  // nothing to search
  // ---- the search: K = 2, cell [0][1]
  const int64_t pp[3] = {0, (int64_t)got[0].size(), (int64_t)pn.size()};
  auto* dpp = dget<int64_t>(c, S_DPP, 3);
  G2N_HIP(hipMemcpyAsync(dpp, pp, sizeof(pp), hipMemcpyHostToDevice, c->stream));
  if (q.wdist) {  // the same over the LAST build's values: cell [0][1] as a double
    auto* wtab = dget<double>(c, S_DTAB, 4);
    g2n_wdist_info wi;
    wpath_distances(c, D.indptr, D.indices, D.index_width, (const double*)D.data, n, (uint64_t)D.nnz, dpp, dpn, 2,
                    G2N_DIST_MIN, wtab, &wi);
    seq_search_end(c, wtab, q.wdist, q.info, wi.rounds, wi.launches, wi.batches, wi.ms_search + wi.ms_tables);
    return;
  }
  auto* dtab = dget<uint32_t>(c, S_DTAB, 4);
  g2n_dist_info di;
  path_distances(c, D.indptr, D.indices, D.index_width, n, (uint64_t)D.nnz, dpp, dpn, 2, G2N_DIST_MIN, dtab, &di);
  seq_search_end(c, dtab, q.dist, q.info, di.levels, di.launches, di.batches, di.ms_bfs);
}

}  // namespace g2n
