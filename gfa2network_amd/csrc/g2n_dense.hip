// g2n_dense.hip — convert --matrix x.csv / x.npy (gfa2network/utils.py:87-96): the dense documents numpy writes
// from A.toarray() — np.savetxt(dest, dense, delimiter=",", fmt="%.6g") and np.save(dest, dense) — rendered from
// the CSR in byte ranges, the dense array never held.  Included by g2n_pipeline.hip behind g2n_queries.hip, whose
// helpers (with_index_type, with_dtype, host_call, check_csr) and the arena it uses as they are.
//
// The csv document.  A row of n_cols cells is "c,c,...,c\n": a cell that is not stored is "0" and every cell
// carries one separator (',' or the row's '\n'), so a row without entries is 2 * n_cols bytes and a stored entry
// whose text has L bytes adds extra = L - 1.  With X = the exclusive scan of extra over the entries in CSR order:
//   row i starts at       R(i) = 2 * n_cols * i + X[indptr[i]]
//   entry k of row i, column c, starts at   E(k) = 2 * (n_cols * i + c) + X[k]   and ends at E(k) + 1 + X[k+1] - X[k]
//   the document holds    2 * n_cols * n_rows + X[nnz]   bytes
// R and E ascend (rows sorted, no duplicates), and a byte p outside every entry's text is '0' when p - X[j] is
// even and a separator when odd, j = the first entry that starts at or behind p (2 * (...) is even, so the parity of
// X[j] is that of E(j)): ',' at even distance behind an entry's end, '0' at even distance from a row's start.
//
// The chosen constants (tests/test_gpu_dense_shapes.py is keyed to them):
//   kDnTile = 4096   bytes of the document per render block, aligned in the document: 256 threads x one 16-byte
//                    store.  A tile holds at most kDnTile / 2 entries and kDnTile / 2 + 1 row ends; the LDS stage
//                    is the tile and one packed word per entry, 12.3 KiB, so the block count per CU is bounded by
//                    its waves, not by LDS.
//
// D1  k_dn_rows      indptr is a non-decreasing map of the rows into [0, nnz] (else the call is refused)
//     k_dn_fmt       one thread per entry: its column is in range, ascends unless the entry opens a row (else the
//                    writer declines: numpy's toarray() adds duplicates), '%.6g' of the value (g6fmt.h) into its
//                    16-byte slot — text, zeros, the length in byte 15 — with one store, extra[k] = L - 1;
//                    scan_excl -> X (nnz + 1 entries)
// D2  k_dn_text      k_gx_text's scheme per tile of [b0, b1): wave 0 finds the row and the entry at the tile's first
//                    byte, wave 1 those at its end (the row bounded by X[nnz] first, then 64 probes a step on R
//                    and E); the tile's entries put their text
//                    and a word (offset, length) in LDS; every thread fills the background of its 16 bytes — one
//                    constant store when no entry touches them —; the tile's rows put their '\n'; aligned 16-byte
//                    stores.  All positions 64-bit.
// D3  k_dn_scatter   the .npy body (the C-order array): the band is cleared (hipMemsetAsync) and the entries of the
//                    rows it touches store their value where the cell lies in it; -0.0 as +0.0 and a signalling NaN
//                    quieted (toarray() adds each value to 0), True as byte 1.
// No atomics, no loop over a row: as the JSON and GEXF paths.
#pragma once

#include "g6fmt.h"

namespace g2n {

constexpr uint32_t kDnTile = 4096;
constexpr uint32_t kDnTpb = kDnTile / 16;      // 256
constexpr uint32_t kDnMaxEnt = kDnTile / 2;    // entries that start inside one tile, plus one that reaches into it

struct DnFlags {
  uint32_t bad;       // indptr / indices out of range
  uint32_t declined;  // a row's columns do not ascend strictly
};

// the CSR on the device and the csv positions
template <class I>
struct DnDoc {
  const I* indptr;
  const I* indices;
  const uint64_t* X;   // nnz + 1
  const uint4* slots;  // nnz
  uint64_t n_rows, n_cols, nnz;
  uint64_t x_total;  // X[nnz]: R(i) lies in [2 * n_cols * i, 2 * n_cols * i + x_total]
};

// ------------------------------------------------------------------ D1 ----
template <class I>
__global__ void __launch_bounds__(kTPB) k_dn_rows(const I* __restrict__ indptr, uint64_t n_rows, uint64_t nnz,
                                                  DnFlags* __restrict__ fl) {
  const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i > n_rows) return;
  const I v = indptr[i];
  bool bad = v < 0 || (uint64_t)v > nnz;
  if (i == 0) bad |= v != 0;
  if (i == n_rows) bad |= (uint64_t)v != nnz;
  else bad |= indptr[i + 1] < v;
  if (bad) fl->bad = 1;
}

// what dense[i, j] += v leaves in a cleared cell
__device__ inline uint8_t dn_cell(uint8_t v, int is_bool) { return is_bool ? (uint8_t)(v != 0) : v; }
__device__ inline int8_t dn_cell(int8_t v, int) { return v; }
__device__ inline int32_t dn_cell(int32_t v, int) { return v; }
__device__ inline float dn_cell(float v, int) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  if (!(b << 1)) b = 0;
  else if ((b & 0x7F800000u) == 0x7F800000u && (b & 0x007FFFFFu)) b |= 0x00400000u;
  __builtin_memcpy(&v, &b, 4);
  return v;
}
__device__ inline double dn_cell(double v, int) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  if (!(b << 1)) b = 0;
  else if ((b & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (b & 0x000FFFFFFFFFFFFFull)) b |= 0x0008000000000000ull;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

// kFmt: the csv's slots and extras; without: the checks alone (.npy)
template <class I, class T, bool kFmt>
__global__ void __launch_bounds__(kTPB) k_dn_fmt(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                 const T* __restrict__ data, uint64_t n_rows, uint64_t n_cols,
                                                 uint64_t nnz, int is_bool, uint4* __restrict__ slots,
                                                 uint8_t* __restrict__ extra, DnFlags* __restrict__ fl) {
  const uint64_t k = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (k > nnz) return;
  if (k == nnz) {
    if (kFmt) extra[k] = 0;  // the scan's last item: X[nnz] = the sum
    return;
  }
  const I c = indices[k];
  if (c < 0 || (uint64_t)c >= n_cols) fl->bad = 1;
  if (k && c <= indices[k - 1]) {  // must open a row: some indptr[i] == k
    uint64_t lo = 0, hi = n_rows + 1;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if ((uint64_t)indptr[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    if (lo > n_rows || (uint64_t)indptr[lo] != k) fl->declined = 1;
  }
  if (kFmt) {
    const T v = dn_cell(data[k], is_bool);  // (a stored -0.0 prints as "0": the dense cell is 0 + v)
    alignas(16) uint8_t text[16];
    const uint32_t len = g6_format((double)v, text);
    slots[k] = *(const uint4*)text;
    extra[k] = (uint8_t)(len - 1);
  }
}

// ------------------------------------------------------------------ D2 ----
// the first q in [lo, hi) with pred(q), hi when there is none; pred ascends (false .. true).  Called by every lane
// of one wave: 64 probes a step.
template <class P>
__device__ inline uint64_t dn_wave_first(uint64_t lo, uint64_t hi, P pred) {
  const uint32_t lane = threadIdx.x & 63u;
  while (hi - lo > 64) {
    const uint64_t step = (hi - lo) / 64;  // probes lo + (l + 1) * step - 1 < hi
    const uint64_t q = lo + (lane + 1) * step - 1;
    const unsigned long long b = __ballot(pred(q));
    if (!b) {
      lo += 64 * step;
    } else {
      const uint32_t f = (uint32_t)__builtin_ctzll(b);
      hi = lo + (f + 1) * step - 1;  // pred holds there
      lo += (uint64_t)f * step;
    }
  }
  const uint64_t q = lo + lane;
  const unsigned long long b = __ballot(q < hi && pred(q));
  return b ? lo + (uint32_t)__builtin_ctzll(b) : hi;
}

template <class I>
__device__ inline uint64_t dn_row_start(const DnDoc<I>& D, uint64_t i) {
  return 2 * D.n_cols * i + D.X[(uint64_t)D.indptr[i]];
}

// the row that holds byte p: the last i with R(i) <= p.  R(i) - 2 * n_cols * i lies in [0, x_total], which bounds
// the row from both sides before anything is probed: one step of 64 probes wherever the extras of the whole
// document are shorter than 62 rows.  Called by every lane of one wave.
template <class I>
__device__ inline uint64_t dn_row_of(const DnDoc<I>& D, uint64_t p) {
  const uint64_t rb = 2 * D.n_cols;
  const uint64_t a = p > D.x_total ? (p - D.x_total) / rb : 0;  // row >= a
  const uint64_t b = p / rb;                                    // row <= b
  uint64_t sh = b + 2 < D.n_rows ? b + 2 : D.n_rows;
  uint64_t sl = a + 1 < sh ? a + 1 : sh;
  return dn_wave_first(sl, sh, [&](uint64_t i) { return dn_row_start(D, i) > p; }) - 1;
}

template <class I>
__global__ void __launch_bounds__(kDnTpb) k_dn_text(DnDoc<I> D, uint64_t b0, uint64_t b1, uint8_t* __restrict__ out) {
  __shared__ uint4 tile4[kDnTile / 16];
  __shared__ uint32_t pk[kDnMaxEnt + 1];  // per entry of the tile: (offset in the tile + 16) << 4 | length
  __shared__ uint64_t s_i[2], s_k[2];
  __shared__ uint32_t s_par;
  uint8_t* tile = (uint8_t*)tile4;
  const uint64_t t0 = (b0 / kDnTile + blockIdx.x) * kDnTile;
  const uint64_t lo = t0 > b0 ? t0 : b0;
  const uint64_t hi = t0 + kDnTile < b1 ? t0 + kDnTile : b1;  // lo < hi: the grid covers [b0, b1)
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  if (wave == 0) {  // the row that holds byte lo, the first entry that ends behind it
    const uint64_t i0 = dn_row_of(D, lo);
    const uint64_t base = 2 * D.n_cols * i0 + 1;
    const uint64_t k0 = dn_wave_first((uint64_t)D.indptr[i0], (uint64_t)D.indptr[i0 + 1], [&](uint64_t k) {
      return base + 2 * (uint64_t)D.indices[k] + D.X[k + 1] > lo;
    });
    if (tid == 0) s_i[0] = i0, s_k[0] = k0;
  } else if (wave == 1) {  // the row that holds byte hi - 1, the first entry that starts at or behind hi
    const uint64_t i1 = dn_row_of(D, hi - 1);
    const uint64_t base = 2 * D.n_cols * i1;
    const uint64_t k1 = dn_wave_first((uint64_t)D.indptr[i1], (uint64_t)D.indptr[i1 + 1], [&](uint64_t k) {
      return base + 2 * (uint64_t)D.indices[k] + D.X[k] >= hi;
    });
    if ((tid & 63u) == 0) s_i[1] = i1, s_k[1] = k1, s_par = (uint32_t)(D.X[k1] & 1u);
  }
  __syncthreads();
  const uint64_t i0 = s_i[0], i1 = s_i[1], k0 = s_k[0];
  uint32_t ne = (uint32_t)(s_k[1] > k0 ? s_k[1] - k0 : 0);
  if (ne > kDnMaxEnt + 1) ne = kDnMaxEnt + 1;  // (never: entries lie two bytes apart at least)
  // ---- the entries: text and packed word
  for (uint32_t j = tid; j < ne; j += kDnTpb) {
    const uint64_t k = k0 + j;
    uint64_t ra = i0, rb = i1;  // the last row in [i0, i1] with indptr[row] <= k
    while (ra < rb) {
      const uint64_t mid = (ra + rb + 1) >> 1;
      if ((uint64_t)D.indptr[mid] <= k) ra = mid;
      else rb = mid - 1;
    }
    const uint64_t e = 2 * (D.n_cols * ra + (uint64_t)D.indices[k]) + D.X[k];
    const int64_t s = (int64_t)(e - t0);  // >= -12
    const uint4 slot4 = D.slots[k];
    uint8_t text[16];
    __builtin_memcpy(text, &slot4, 16);
    const uint32_t len = text[15] < 14 ? text[15] : 13;
    for (uint32_t b = 0; b < len; b++) {
      const int64_t p = s + b;
      if (p >= 0 && p < (int64_t)kDnTile) tile[p] = text[b];
    }
    pk[j] = ((uint32_t)(s + 16) << 4) | len;
  }
  __syncthreads();
  // ---- the background of this thread's 16 bytes
  {
    const uint32_t c0 = tid * 16u, c1 = c0 + 16u;
    uint32_t ja = 0, jb = ne;  // the first entry that starts at or behind c0
    while (ja < jb) {
      const uint32_t mid = (ja + jb) >> 1;
      if ((pk[mid] >> 4) < c0 + 16u) ja = mid + 1;
      else jb = mid;
    }
    uint32_t j = ja, pos = c0;
    if (j) {
      const uint32_t w = pk[j - 1];
      const uint32_t end = (w >> 4) + (w & 15u);  // + 16
      if (end > pos + 16u) pos = end - 16u;
    }
    const uint32_t nxt0 = j < ne ? (pk[j] >> 4) - 16u : 0xFFFFFFFFu;
    if (pos == c0 && nxt0 >= c1) {  // no entry touches the chunk: one of two constants
      const uint32_t par = j < ne ? (nxt0 & 1u) : s_par;
      const uint32_t w = par ? 0x302C302Cu : 0x2C302C30u;  // ",0,0" : "0,0," (little endian)
      tile4[tid] = make_uint4(w, w, w, w);
    } else {
      while (pos < c1) {
        const uint32_t nxt = j < ne ? (pk[j] >> 4) - 16u : 0xFFFFFFFFu;
        const uint32_t par = j < ne ? (nxt & 1u) : s_par;
        const uint32_t stop = nxt < c1 ? nxt : c1;
        for (; pos < stop; pos++) tile[pos] = ((pos ^ par) & 1u) ? ',' : '0';
        if (nxt >= c1) break;
        pos = nxt + (pk[j] & 15u);
        j++;
      }
    }
  }
  __syncthreads();
  // ---- the rows' ends
  for (uint64_t i = i0 + tid; i <= i1; i += kDnTpb) {
    const uint64_t nl = dn_row_start(D, i + 1) - 1;  // (row n_rows starts at the document's end)
    if (nl >= t0 && nl < t0 + kDnTile) tile[nl - t0] = '\n';
  }
  __syncthreads();
  const uint64_t a = t0 + (uint64_t)tid * 16u;
  if (a >= lo && a + 16 <= hi) {
    *(uint4*)(out + (a - b0)) = tile4[tid];  // (the caller places out so that the document's 16-byte words are aligned)
  } else {
    for (uint64_t p = a < lo ? lo : a; p < a + 16 && p < hi; p++) out[p - b0] = tile[p - t0];
  }
}

// ------------------------------------------------------------------ D3 ----
// entries [ka, kb) — those of rows [r0, r1], the rows the band [b0, b1) of the body touches — into out[p - b0]
template <class I, class T>
__global__ void __launch_bounds__(kTPB) k_dn_scatter(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                     const T* __restrict__ data, uint64_t n_cols, uint64_t r0, uint64_t r1,
                                                     uint64_t ka, uint64_t kb, int is_bool, uint64_t b0, uint64_t b1,
                                                     uint8_t* __restrict__ out) {
  const uint64_t k = ka + (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (k >= kb) return;
  uint64_t ra = r0, rb = r1;  // the last row in [r0, r1] with indptr[row] <= k
  while (ra < rb) {
    const uint64_t mid = (ra + rb + 1) >> 1;
    if ((uint64_t)indptr[mid] <= k) ra = mid;
    else rb = mid - 1;
  }
  const uint64_t p = (n_cols * ra + (uint64_t)indices[k]) * sizeof(T);
  const T v = dn_cell(data[k], is_bool);
  if (p >= b0 && p + sizeof(T) <= b1 && ((p - b0) % sizeof(T)) == 0) {
    *(T*)(out + (p - b0)) = v;  // (out is placed so that the body's cells are aligned)
  } else {
    uint8_t raw[sizeof(T)];
    __builtin_memcpy(raw, &v, sizeof(T));
    for (uint32_t b = 0; b < sizeof(T); b++)
      if (p + b >= b0 && p + b < b1) out[p + b - b0] = raw[b];
  }
}

// ------------------------------------------------------------------ the driver ----
constexpr uint64_t kDnDefaultBand = 16ull << 20;  // bytes of the document per band (two on the device, two pinned)

struct DnPlan {  // one matrix staged and checked on c's stream
  int kind, dtype, index_width;
  uint64_t n_rows, n_cols, nnz, w;  // w: the dtype's bytes
  void *indptr, *indices, *data;
  uint4* slots;
  uint64_t* X;
  uint64_t total;  // bytes of the body
  bool declined;
};

// the entries of a host CSR: indptr[n_rows]
uint64_t dense_host_nnz(const std::string& who, const void* indptr, int32_t index_width, uint64_t n_rows) {
  if (!indptr) throw Failure(G2N_E_ARG, who + ": null array");
  if (index_width != 4 && index_width != 8) throw Failure(G2N_E_ARG, who + ": index_width must be 4 or 8");
  if (n_rows >= 0x7FFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^31-1 or more rows");
  const int64_t v = index_width == 4 ? (int64_t)((const int32_t*)indptr)[n_rows] : ((const int64_t*)indptr)[n_rows];
  if (v < 0) throw Failure(G2N_E_ARG, who + ": indptr out of range");
  return (uint64_t)v;
}

static void dense_check_args(const std::string& who, int32_t kind, const void* indptr, const void* indices,
                             int32_t index_width, const void* data, int32_t dtype, uint64_t n_rows, uint64_t n_cols,
                             uint64_t nnz) {
  if (kind != 0 && kind != 1) throw Failure(G2N_E_ARG, who + ": kind must be 0 (csv) or 1 (npy)");
  if (dtype < G2N_BOOL || dtype > G2N_FLOAT64) throw Failure(G2N_E_ARG, who + ": unknown dtype");
  check_csr(who, index_width, n_rows, nnz, indptr != nullptr, indices && data, false);
  if (n_rows == 0 || n_cols == 0) throw Failure(G2N_E_ARG, who + ": an empty shape");
  if (n_cols >= 0x7FFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, who + ": 2^31-1 or more columns");
}

// uploads the CSR, runs D1 (csv: with the slots and the scan), reads the flags and the document's length
static DnPlan dense_plan(g2n_context* c, const std::string& who, int32_t kind, const void* indptr, const void* indices,
                         int32_t index_width, const void* data, int32_t dtype, uint64_t n_rows, uint64_t n_cols,
                         uint64_t nnz) {
  DnPlan P{};
  P.kind = kind, P.dtype = dtype, P.index_width = index_width;
  P.n_rows = n_rows, P.n_cols = n_cols, P.nnz = nnz, P.w = dtype_size(dtype);
  const size_t iw = (size_t)index_width;
  P.indptr = dbuf(c, S_DNIP, (n_rows + 1) * iw);
  P.indices = dbuf(c, S_DNIX, nnz * iw);
  P.data = dbuf(c, S_DNVAL, nnz * P.w);
  auto* fl = dget<DnFlags>(c, S_DNFLAG, 1);
  G2N_HIP(hipMemcpyAsync(P.indptr, indptr, (n_rows + 1) * iw, hipMemcpyHostToDevice, c->stream));
  if (nnz) {
    G2N_HIP(hipMemcpyAsync(P.indices, indices, nnz * iw, hipMemcpyHostToDevice, c->stream));
    G2N_HIP(hipMemcpyAsync(P.data, data, nnz * P.w, hipMemcpyHostToDevice, c->stream));
  }
  G2N_HIP(hipMemsetAsync(fl, 0, sizeof(DnFlags), c->stream));
  uint8_t* extra = nullptr;
  if (kind == 0) {
    P.slots = dget<uint4>(c, S_DNSLOT, nnz);
    extra = dget<uint8_t>(c, S_DNEXTRA, nnz + 1);
    P.X = dget<uint64_t>(c, S_DNX, nnz + 1);
  }
  with_index_type(index_width, P.indptr, P.indices, [&](auto* ip, auto* ix) {
    using I = std::remove_cv_t<std::remove_pointer_t<decltype(ip)>>;
    hipLaunchKernelGGL(k_dn_rows<I>, dim3(grid_for(n_rows + 1)), dim3(kTPB), 0, c->stream, ip, n_rows, nnz, fl);
    with_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      if (kind == 0)
        hipLaunchKernelGGL((k_dn_fmt<I, T, true>), dim3(grid_for(nnz + 1)), dim3(kTPB), 0, c->stream, ip, ix,
                           (const T*)P.data, n_rows, n_cols, nnz, (int)(dtype == G2N_BOOL), P.slots, extra, fl);
      else
        hipLaunchKernelGGL((k_dn_fmt<I, T, false>), dim3(grid_for(nnz + 1)), dim3(kTPB), 0, c->stream, ip, ix,
                           (const T*)P.data, n_rows, n_cols, nnz, (int)(dtype == G2N_BOOL), (uint4*)nullptr,
                           (uint8_t*)nullptr, fl);
    });
  });
  if (kind == 0) scan_excl<uint8_t, uint64_t>(c, extra, P.X, nnz + 1);
  const DnFlags h = read_dev(c, fl);
  if (h.bad) throw Failure(G2N_E_ARG, who + ": indptr / indices out of range");
  P.declined = h.declined != 0;
  P.total = kind == 0 ? 2 * n_cols * n_rows + read_dev(c, P.X + nnz) : n_rows * n_cols * P.w;
  return P;
}

// bytes [b0, b1) of P's body (b0 < b1 <= P.total) rendered on stream s at dev + (b0 & 15); returns that address.
// dev holds b1 - b0 + 16 bytes; h_indptr: the host's indptr (the .npy band's entries).
static uint8_t* dense_render(g2n_context* c, const DnPlan& P, const void* h_indptr, uint64_t b0, uint64_t b1,
                             uint8_t* dev, hipStream_t s) {
  uint8_t* out = dev + (b0 & 15u);
  with_index_type(P.index_width, P.indptr, P.indices, [&](auto* ip, auto* ix) {
    using I = std::remove_cv_t<std::remove_pointer_t<decltype(ip)>>;
    if (P.kind == 0) {
      const DnDoc<I> D{ip, ix, P.X, P.slots, P.n_rows, P.n_cols, P.nnz, P.total - 2 * P.n_cols * P.n_rows};
      const uint64_t tiles = (b1 - 1) / kDnTile - b0 / kDnTile + 1;
      hipLaunchKernelGGL(k_dn_text<I>, dim3((unsigned)tiles), dim3(kDnTpb), 0, s, D, b0, b1, out);
      return;
    }
    G2N_HIP(hipMemsetAsync(out, 0, b1 - b0, s));
    const uint64_t row_bytes = P.n_cols * P.w;
    const uint64_t r0 = b0 / row_bytes, r1 = (b1 - 1) / row_bytes;
    const auto* hp = (const I*)h_indptr;
    const uint64_t ka = (uint64_t)hp[r0], kb = (uint64_t)hp[r1 + 1];
    if (kb <= ka) return;
    with_dtype(P.dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_dn_scatter<I, T>), dim3(grid_for(kb - ka)), dim3(kTPB), 0, s, ip, ix, (const T*)P.data,
                         P.n_cols, r0, r1, ka, kb, (int)(P.dtype == G2N_BOOL), b0, b1, out);
    });
  });
  return out;
}

static void dense_info(const DnPlan& P, uint64_t band, g2n_dense_info* info) {
  info->doc_bytes = P.total;
  info->tile_bytes = kDnTile;
  info->band_bytes = band;
  info->bands = band ? (P.total + band - 1) / band : 0;
  info->declined = P.declined ? 1 : 0;
}

int dense_range(int32_t kind, const void* indptr, const void* indices, int32_t index_width, const void* data,
                int32_t dtype, uint64_t n_rows, uint64_t n_cols, uint64_t nnz, int32_t device, uint64_t b0, uint64_t b1,
                uint8_t* out, g2n_dense_info* info) {
  const std::string who = "g2n_dense_range";
  dense_check_args(who, kind, indptr, indices, index_width, data, dtype, n_rows, n_cols, nnz);
  return host_call(device, [&](g2n_context* c) {
    const DnPlan P = dense_plan(c, who, kind, indptr, indices, index_width, data, dtype, n_rows, n_cols, nnz);
    dense_info(P, 0, info);
    if (P.declined) return;
    if (b0 > b1 || b1 > P.total) throw Failure(G2N_E_ARG, who + ": the range lies outside the document");
    if (b0 == b1) return;
    if (!out) throw Failure(G2N_E_ARG, who + ": null output");
    check_fits(who, b1 - b0 + 16, "the range exceeds");
    auto* dev = dget<uint8_t>(c, S_DNBAND0, b1 - b0 + 16);
    const uint8_t* at = dense_render(c, P, indptr, b0, b1, dev, c->stream);
    G2N_HIP(hipMemcpyAsync(out, at, b1 - b0, hipMemcpyDeviceToHost, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
  });
}

// write(2) of all n bytes; errno on failure
static int dense_write_all(int fd, const uint8_t* p, size_t n) {
  while (n) {
    const ssize_t r = ::write(fd, p, n);
    if (r < 0) {
      if (errno == EINTR) continue;
      return errno;
    }
    p += r;
    n -= (size_t)r;
  }
  return 0;
}

// g2n_dense_last_times: where the calling thread's last g2n_write_dense spent its time
static thread_local double t_dense_ms[5] = {0, 0, 0, 0, 0};  // plan, render, copy, write, total
void dense_last_times(double out[5]) {
  for (int i = 0; i < 5; i++) out[i] = t_dense_ms[i];
}

int write_dense(const char* path, int32_t kind, const void* head, size_t head_len, const void* indptr,
                const void* indices, int32_t index_width, const void* data, int32_t dtype, uint64_t n_rows,
                uint64_t n_cols, uint64_t nnz, uint64_t band_bytes, int32_t device, g2n_dense_info* info) {
  const std::string who = "g2n_write_dense";
  dense_check_args(who, kind, indptr, indices, index_width, data, dtype, n_rows, n_cols, nnz);
  if (band_bytes % kDnTile) throw Failure(G2N_E_ARG, who + ": band_bytes must be a multiple of the tile");
  struct Pinned {  // the two host bands, the copy stream and its events
    uint8_t* h[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipEvent_t render0[2] = {nullptr, nullptr}, rendered[2] = {nullptr, nullptr};
    hipEvent_t copy0[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    int fd = -1;
    ~Pinned() {
      if (copy) (void)hipStreamSynchronize(copy);
      for (auto& p : h)
        if (p) (void)hipHostFree(p);
      for (auto* ev : {render0, rendered, copy0, copied})
        for (int s = 0; s < 2; s++)
          if (ev[s]) (void)hipEventDestroy(ev[s]);
      if (copy) (void)hipStreamDestroy(copy);
      if (fd >= 0) ::close(fd);
    }
  };
  for (auto& t : t_dense_ms) t = 0;
  return host_call(device, [&](g2n_context* c) {
    const double t_start = now_ms();
    const DnPlan P = dense_plan(c, who, kind, indptr, indices, index_width, data, dtype, n_rows, n_cols, nnz);
    t_dense_ms[0] = now_ms() - t_start;
    uint64_t band = band_bytes;
    if (!band) {  // what the CSR and its slots leave of the free memory, in two bands; kDnDefaultBand at most
      size_t f = 0, t = 0;
      G2N_HIP(hipMemGetInfo(&f, &t));
      band = std::min<uint64_t>(kDnDefaultBand, (uint64_t)f / 4 / kDnTile * kDnTile);
      if (band < kDnTile) throw Failure(G2N_E_NOMEM, who + ": no device memory left for a band");
    }
    band = std::min<uint64_t>(band, (P.total + kDnTile - 1) / kDnTile * kDnTile);
    dense_info(P, band, info);
    if (P.declined) return;
    Pinned H;
    H.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (H.fd < 0) {
      const int err = errno;
      throw Failure(G2N_E_IO, std::string(path) + ": " + std::strerror(err));
    }
    if (head_len) {
      if (const int err = dense_write_all(H.fd, (const uint8_t*)head, head_len))
        throw Failure(G2N_E_IO, std::string(path) + ": " + std::strerror(err));
    }
    uint8_t* dev[2] = {dget<uint8_t>(c, S_DNBAND0, band + 16), dget<uint8_t>(c, S_DNBAND1, band + 16)};
    for (auto& p : H.h) G2N_HIP(hipHostMalloc((void**)&p, band, hipHostMallocDefault));
    G2N_HIP(hipStreamCreateWithFlags(&H.copy, hipStreamNonBlocking));
    for (auto* ev : {H.render0, H.rendered, H.copy0, H.copied})  // (timed: g2n_dense_last_times)
      for (int s = 0; s < 2; s++) G2N_HIP(hipEventCreate(&ev[s]));
    // band b renders into dev[b & 1] on the pipeline's stream once the copy of band b - 2 has left it, is copied to
    // H.h[b & 1] on the copy stream once band b - 2 was written from there, and is written while band b + 1 copies
    const uint64_t n_bands = info->bands;
    auto issue = [&](uint64_t b) {
      const int s = (int)(b & 1u);
      const uint64_t p0 = b * band, p1 = std::min(P.total, p0 + band);
      if (b >= 2) G2N_HIP(hipStreamWaitEvent(c->stream, H.copied[s], 0));
      G2N_HIP(hipEventRecord(H.render0[s], c->stream));
      const uint8_t* at = dense_render(c, P, indptr, p0, p1, dev[s], c->stream);  // (p0 is a multiple of 16)
      G2N_HIP(hipEventRecord(H.rendered[s], c->stream));
      G2N_HIP(hipStreamWaitEvent(H.copy, H.rendered[s], 0));
      G2N_HIP(hipEventRecord(H.copy0[s], H.copy));
      G2N_HIP(hipMemcpyAsync(H.h[s], at, p1 - p0, hipMemcpyDeviceToHost, H.copy));
      G2N_HIP(hipEventRecord(H.copied[s], H.copy));
    };
    if (n_bands) issue(0);
    for (uint64_t b = 0; b < n_bands; b++) {
      const int s = (int)(b & 1u);
      if (b + 1 < n_bands) issue(b + 1);  // (its host band was written in the last iteration)
      G2N_HIP(hipEventSynchronize(H.copied[s]));
      float ms = 0.f;
      G2N_HIP(hipEventElapsedTime(&ms, H.render0[s], H.rendered[s]));
      t_dense_ms[1] += ms;
      G2N_HIP(hipEventElapsedTime(&ms, H.copy0[s], H.copied[s]));
      t_dense_ms[2] += ms;
      const double t_write = now_ms();
      const uint64_t p0 = b * band, p1 = std::min(P.total, p0 + band);
      if (const int err = dense_write_all(H.fd, H.h[s], p1 - p0))
        throw Failure(G2N_E_IO, std::string(path) + ": " + std::strerror(err));
      t_dense_ms[3] += now_ms() - t_write;
    }
    G2N_HIP(hipStreamSynchronize(c->stream));
    const int fd = H.fd;
    H.fd = -1;
    if (::close(fd) != 0) {
      const int err = errno;
      throw Failure(G2N_E_IO, std::string(path) + ": " + std::strerror(err));
    }
    t_dense_ms[4] = now_ms() - t_start;
  });
}

}  // namespace g2n
