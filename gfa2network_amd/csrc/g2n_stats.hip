// g2n_stats.hip — graph statistics over a device-resident CSR structure (g2n_csr_stats): what the
// reference's compute_stats reads off a NetworkX graph (gfa2network/analysis.py:33-65), as integer
// work on indptr / indices.  The values are never read.
//
// Components: a lock-free union-find over parent[] (parent[x] <= x always, so no cycle can form).
//   k_cc_init     parent[i] = the row's first neighbour when it is smaller than i, else i (no atomics)
//   k_rows_short / k_rows_long <HookOp>
//                 every stored (u, v): find both roots with path halving (plain loads and stores,
//                 served by the caches) and, only when they differ, hook the larger root under the
//                 smaller with one compare-and-swap; a lost race continues from the value the swap
//                 returned.  A thread carries its row's last known root from entry to entry: an
//                 entry whose column already points at it costs one load.
//   k_cc_flatten  parent[i] = its root; roots counted (one atomic per block)
//   The partition into sets, and so the count, does not depend on how the races resolve.  Nothing
//   iterates to a fixed point: the work per entry is a few loads once the trees are shallow, whatever
//   the graph's diameter.
// Degrees: row lengths from indptr; one walk over the entries marks the rows that hold their own index
//   and, for a directed graph, counts each column's occurrences with a scattered atomic histogram;
//   k_deg_max then reduces the maximum and the diagonal count (one atomic each per block).
// Rows longer than kStatsShortRow entries are queued by the first walk and walked by a block each.
// Every index read from the caller's arrays is range-checked before it addresses anything: a bad
// indptr / indices sets StatsOut::bad and is skipped (the call then fails with G2N_E_ARG).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g2n {

constexpr uint32_t kStatsShortRow = 64;    // rows up to this many entries are walked by one thread
constexpr uint32_t kStatsLongBlocks = 1024;  // blocks that share the queue of longer rows

struct StatsOut {
  unsigned long long max_degree, n_diag, n_roots, high_off;
  unsigned int bad, n_long;
  long long high_id;
};

// parent[] is read and halved with plain loads and stores (wavefront scope: one access each, never
// merged or hoisted by the compiler), served by the caches.  A stale value is an older one, and every
// value parent[x] ever held is an ancestor-or-self of x, so a stale read only lengthens a walk; what
// decides a hook is the compare-and-swap, which executes on the word itself.
__device__ inline uint32_t uf_ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ inline void uf_st(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// x's root, halving the path on the way.  Only non-roots are stored to, with one of their ancestors:
// a hook's compare-and-swap expects parent[r] == r, which never holds again for a non-root.
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_ld(parent + x);
    if (p == x) return x;
    const uint32_t g = uf_ld(parent + p);
    if (g == p) return p;
    uf_st(parent + x, g);
    x = g;
  }
}

__device__ inline uint32_t uf_find_ro(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_ld(parent + x);
    if (p == x) return x;
    x = p;
  }
}

// Joins v's set with the set of ru, an ancestor-or-self of the row (its last known root), and returns
// the row's new last known root.  parent[v] == ru — the usual case once a row's first entry has
// been joined — costs the one load and touches no root's word.
__device__ inline uint32_t uf_link(uint32_t* parent, uint32_t ru, uint32_t v) {
  if (uf_ld(parent + v) == ru) return ru;
  ru = uf_find(parent, ru);
  uint32_t rv = uf_find(parent, v);
  while (ru != rv) {
    const uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    ru = uf_find(parent, old);  // hi was hooked meanwhile: go on from where it points now
    rv = uf_find(parent, lo);
  }
  return ru;
}

// state: what a thread carries from one entry of a row to the next (begin(row) before the first)
struct HookOp {
  uint32_t* parent;
  __device__ inline uint32_t begin(uint32_t row) const { return row; }
  __device__ inline void entry(uint32_t row, uint32_t col, uint32_t& root) const {
    if (col != row) root = uf_link(parent, root, col);
  }
};

struct DegOp {
  uint8_t* diag;      // 1: the row holds its own index (racing stores of the same value)
  uint32_t* colcnt;   // directed: occurrences of each index as a column; else null
  __device__ inline uint32_t begin(uint32_t) const { return 0; }
  __device__ inline void entry(uint32_t row, uint32_t col, uint32_t&) const {
    if (col == row) diag[row] = 1;
    if (colcnt) atomicAdd(colcnt + col, 1u);
  }
};

// [b, e) of row i, or false (StatsOut::bad set) when indptr is not a non-decreasing map into [0, nnz]
template <class I>
__device__ inline bool row_range(const I* __restrict__ indptr, uint64_t i, uint64_t nnz, uint64_t* b, uint64_t* e,
                                 StatsOut* so) {
  const int64_t lo = (int64_t)indptr[i], hi = (int64_t)indptr[i + 1];
  if (lo < 0 || hi < lo || (uint64_t)hi > nnz) {
    so->bad = 1u;
    return false;
  }
  *b = (uint64_t)lo;
  *e = (uint64_t)hi;
  return true;
}

template <class I>
__global__ void __launch_bounds__(256) k_cc_init(const I* __restrict__ indptr, const I* __restrict__ indices, uint64_t n,
                                                 uint64_t nnz, uint32_t* __restrict__ parent, StatsOut* so) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t p = (uint32_t)i;
  uint64_t b, e;
  if (row_range(indptr, i, nnz, &b, &e, so) && e > b) {
    const uint64_t c = (uint64_t)indices[b];
    if (c < i) p = (uint32_t)c;  // (c >= n is not below i; the walks report it)
  }
  parent[i] = p;
}

// One thread per row of at most kStatsShortRow entries.  collect: longer rows are queued in long_rows
// (capacity nnz / kStatsShortRow + 1: there cannot be more) for k_rows_long.
template <class I, class Op>
__global__ void __launch_bounds__(256) k_rows_short(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                    uint64_t n, uint64_t nnz, Op op, int collect,
                                                    uint32_t* __restrict__ long_rows, uint64_t long_cap, StatsOut* so) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t b, e;
  if (!row_range(indptr, i, nnz, &b, &e, so)) return;
  if (e - b > kStatsShortRow) {
    if (collect) {
      const unsigned int k = atomicAdd(&so->n_long, 1u);
      if (k < long_cap) long_rows[k] = (uint32_t)i;
      else so->bad = 1u;
    }
    return;
  }
  uint32_t state = op.begin((uint32_t)i);
  for (uint64_t j = b; j < e; j++) {
    const uint64_t c = (uint64_t)indices[j];
    if (c >= n) {
      so->bad = 1u;
      continue;
    }
    op.entry((uint32_t)i, (uint32_t)c, state);
  }
}

template <class I, class Op>
__global__ void __launch_bounds__(256) k_rows_long(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                   uint64_t n, uint64_t nnz, Op op,
                                                   const uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                   StatsOut* so) {
  uint64_t n_long = so->n_long;
  if (n_long > long_cap) n_long = long_cap;
  for (uint64_t w = blockIdx.x; w < n_long; w += gridDim.x) {
    const uint64_t i = long_rows[w];
    if (i >= n) continue;
    uint64_t b, e;
    if (!row_range(indptr, i, nnz, &b, &e, so)) continue;
    uint32_t state = op.begin((uint32_t)i);
    for (uint64_t j = b + threadIdx.x; j < e; j += 256) {
      const uint64_t c = (uint64_t)indices[j];
      if (c >= n) {
        so->bad = 1u;
        continue;
      }
      op.entry((uint32_t)i, (uint32_t)c, state);
    }
  }
}

__device__ inline unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(v, o, 64);
    v = x > v ? x : v;
  }
  return v;
}
__device__ inline unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(v, o, 64);
    v = x < v ? x : v;
  }
  return v;
}
__device__ inline unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// degree of row i = its length + (directed: its column count; else: 1 if it holds i)
template <class I>
__global__ void __launch_bounds__(256) k_deg_max(const I* __restrict__ indptr, uint64_t n, uint64_t nnz,
                                                 const uint8_t* __restrict__ diag, const uint32_t* __restrict__ colcnt,
                                                 StatsOut* so) {
  __shared__ unsigned long long red[2][4];
  unsigned long long mx = 0, nd = 0;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    uint64_t b, e;
    if (!row_range(indptr, i, nnz, &b, &e, so)) continue;
    const unsigned long long d = (e - b) + (colcnt ? (unsigned long long)colcnt[i] : (unsigned long long)diag[i]);
    mx = d > mx ? d : mx;
    nd += diag[i];
  }
  mx = wave_max(mx);
  nd = wave_sum(nd);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx;
    red[1][threadIdx.x >> 6] = nd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      mx = red[0][w] > mx ? red[0][w] : mx;
      nd += red[1][w];
    }
    if (mx) atomicMax(&so->max_degree, mx);
    if (nd) atomicAdd(&so->n_diag, nd);
  }
}

__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t* __restrict__ parent, uint64_t n, StatsOut* so) {
  __shared__ unsigned long long red[4];
  unsigned long long roots = 0;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const uint32_t r = uf_find_ro(parent, (uint32_t)i);
    roots += r == (uint32_t)i;
    if (r != (uint32_t)i) uf_st(parent + i, r);
  }
  roots = wave_sum(roots);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    roots = red[0] + red[1] + red[2] + red[3];
    if (roots) atomicAdd(&so->n_roots, roots);
  }
}

// The lowest offset of a byte >= 0x80 in blob[0, len) (StatsOut::high_off, ~0 before: none): the node
// keys the reference's graph path decodes as ASCII (builders.py:155-162).  blob is 16-byte aligned.
__global__ void __launch_bounds__(256) k_high_byte(const uint8_t* __restrict__ blob, uint64_t len, StatsOut* so) {
  unsigned long long best = ~0ull;
  const uint64_t stride = (uint64_t)gridDim.x * 256 * 16;
  for (uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16; p < len && best == ~0ull; p += stride) {
    if (p + 16 <= len) {
      const uint4 v = *reinterpret_cast<const uint4*>(blob + p);
      const uint32_t w[4] = {v.x & 0x80808080u, v.y & 0x80808080u, v.z & 0x80808080u, v.w & 0x80808080u};
      for (int q = 0; q < 4; q++)
        if (w[q]) {
          best = p + 4 * q + ((uint32_t)__builtin_ctz(w[q]) >> 3);
          break;
        }
    } else {
      for (uint64_t j = p; j < len; j++)
        if (blob[j] & 0x80u) {
          best = j;
          break;
        }
    }
  }
  best = wave_min(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&so->high_off, best);
}

// the key that holds blob offset high_off: the last id whose start is <= it (empty keys share a start)
__global__ void k_high_owner(const int64_t* __restrict__ offs, uint64_t n, StatsOut* so) {
  if (blockIdx.x || threadIdx.x) return;
  const long long off = (long long)so->high_off;
  uint64_t lo = 0, hi = n;  // first id in [0, n] whose start is > off
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (offs[mid] <= off) lo = mid + 1;
    else hi = mid;
  }
  so->high_id = (long long)lo - 1;
}

}  // namespace g2n
