// g2n_components.hip — which node is in which connected component, and the matrix regrouped by
// component (g2n_csr_components, g2n_csr_split_components_host), over a device-resident CSR.
//
// The union-find is g2n_stats.hip's, as it is: k_cc_init, k_rows_short / k_rows_long <HookOp>,
// k_cc_flatten.  It hooks the larger root under the smaller, so after the flatten parent[i] is the
// smallest index of i's component, whatever way the races went.  Numbering the roots in index order
// is therefore scipy.sparse.csgraph.connected_components' numbering (and that of
// nx.connected_components over nodes in first-touch order), the same on every run.
//
// Labels   k_cc_roots    flag[i] = parent[i] == i
//          k_scan_excl   rank[] (g2n_scan.hip); its total is the number of components k
//          k_cc_labels   label[i] = rank[parent[i]] (int32); idx[i] = i for the sort
// Groups   sort_pairs_u32 (g2n_sort.hip) key = label, payload = index, ceil(bits(k) / 8) stable
//          passes: perm = the nodes ordered by label, index order kept inside a component
//          (np.argsort(labels, kind="stable")), and the labels in that order
//          k_cc_bounds   off[j] = the first position of label j in the sorted order, off[k] = n: each
//          label's boundary is written by the one position that sees it, no atomics (one giant
//          component would send every node to one address)
// Split    k_split_rows  new row p is old row perm[p]: its length, and local[perm[p]] = p - off[label]
//          — the node's index inside its own component (inv[perm[p]] = p folded into it: nothing
//          else reads inv), one scattered 4-byte store per node instead of three dependent gathers
//          per entry
//          k_scan_excl   new row starts, 64-bit
//          k_split_short one thread per new row of at most kSplitShortRow entries: out_indptr[p], and
//          the row's entries copied in stored order with col -> local[col]; values copied by item
//          size 1, 4 or 8, or skipped.  Longer rows are queued: up to kSplitHugeRow entries in
//          one queue, past it in another.
//          k_split_long  one block per row of the first queue, coalesced; then every block takes
//          its stripes of each row of the second (a star's hub is copied by the whole grid, not by
//          one block).
// Every stored (u, v) has both ends in one component, so the split is a permutation of the whole
// matrix: component j is rows [off[j], off[j + 1]) of it, its columns already local.
// indptr / indices were range-checked whole by the union-find walks before any of the split's
// kernels runs (the host reads StatsOut::bad in between); the split's kernels check again what they
// address with, as every kernel here does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2n_stats.hip"

namespace g2n {

constexpr uint32_t kSplitShortRow = 64;    // rows up to this many entries are copied by one thread
constexpr uint32_t kSplitHugeRow = 4096;   // ... up to this many by one block, longer ones by the whole grid

struct SplitQueues {
  unsigned int n_long, n_huge;
};

__global__ void __launch_bounds__(256) k_cc_roots(const uint32_t* __restrict__ parent, uint64_t n,
                                                  uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = parent[i] == (uint32_t)i ? 1u : 0u;
}

// parent is flattened: parent[i] is a root below n, whose rank is its component's number
__global__ void __launch_bounds__(256) k_cc_labels(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rank,
                                                   uint64_t n, int32_t* __restrict__ label, uint32_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = parent[i];
  label[i] = r < n ? (int32_t)rank[r] : 0;
  if (idx) idx[i] = (uint32_t)i;
}

// key_s: the labels in sorted order (every label 0..k-1 occurs: a root carries its own)
__global__ void __launch_bounds__(256) k_cc_bounds(const uint32_t* __restrict__ key_s, uint64_t n, uint64_t k,
                                                   int64_t* __restrict__ off) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t lab = key_s[p];
  if (lab < k && (p == 0 || key_s[p - 1] != lab)) off[lab] = (int64_t)p;
  if (p == n - 1) off[k] = (int64_t)n;
}

// one thread per new row p in [0, n]: len[p] (len[n] = 0, the scan's last start is the total),
// local[] and the 64-bit copy of perm the caller receives
template <class I>
__global__ void __launch_bounds__(256) k_split_rows(const I* __restrict__ indptr, uint64_t n, uint64_t nnz,
                                                    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key_s,
                                                    const int64_t* __restrict__ off, uint64_t k,
                                                    uint32_t* __restrict__ local, int64_t* __restrict__ len,
                                                    int64_t* __restrict__ perm64, StatsOut* so) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  if (p == n) {
    len[n] = 0;
    return;
  }
  const uint64_t u = perm[p];
  const uint32_t lab = key_s[p];
  int64_t l = 0;
  if (u >= n || lab >= k) {
    so->bad = 1u;
  } else {
    local[u] = (uint32_t)((int64_t)p - off[lab]);
    uint64_t b, e;
    if (row_range(indptr, u, nnz, &b, &e, so)) l = (int64_t)(e - b);
  }
  len[p] = l;
  perm64[p] = (int64_t)u;
}

template <int VB>
__device__ inline void split_value(const void* __restrict__ in, void* __restrict__ out, uint64_t s, uint64_t d) {
  if constexpr (VB == 1) ((uint8_t*)out)[d] = ((const uint8_t*)in)[s];
  if constexpr (VB == 4) ((uint32_t*)out)[d] = ((const uint32_t*)in)[s];
  if constexpr (VB == 8) ((uint64_t*)out)[d] = ((const uint64_t*)in)[s];
}

// entry s of the old matrix to position d of the new one (d < nnz: pos is the scan of the checked lengths)
template <class I, int VB>
__device__ inline void split_entry(const I* __restrict__ indices, const void* __restrict__ data, uint64_t n, uint64_t nnz,
                                   const uint32_t* __restrict__ local, I* __restrict__ out_indices,
                                   void* __restrict__ out_data, uint64_t s, uint64_t d, StatsOut* so) {
  const uint64_t c = (uint64_t)indices[s];
  if (c >= n || d >= nnz) {
    so->bad = 1u;
    return;
  }
  out_indices[d] = (I)local[c];
  split_value<VB>(data, out_data, s, d);
}

template <class I, int VB>
__global__ void __launch_bounds__(256) k_split_short(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                     const void* __restrict__ data, uint64_t n, uint64_t nnz,
                                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ local,
                                                     const int64_t* __restrict__ pos, I* __restrict__ out_indptr,
                                                     I* __restrict__ out_indices, void* __restrict__ out_data,
                                                     uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                     uint32_t* __restrict__ huge_rows, uint64_t huge_cap,
                                                     SplitQueues* sq, StatsOut* so) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  out_indptr[p] = (I)pos[p];
  if (p == n) return;
  const uint64_t u = perm[p];
  uint64_t b, e;
  if (u >= n || !row_range(indptr, u, nnz, &b, &e, so)) return;
  if (e - b > kSplitShortRow) {
    const bool huge = e - b > kSplitHugeRow;
    const unsigned int q = atomicAdd(huge ? &sq->n_huge : &sq->n_long, 1u);
    if (q < (huge ? huge_cap : long_cap)) (huge ? huge_rows : long_rows)[q] = (uint32_t)p;
    else so->bad = 1u;
    return;
  }
  const uint64_t d = (uint64_t)pos[p];
  for (uint64_t j = b; j < e; j++)
    split_entry<I, VB>(indices, data, n, nnz, local, out_indices, out_data, j, d + (j - b), so);
}

// entries [b + first, e) of new row p in steps of `step`, this thread's share
template <class I, int VB>
__device__ inline void split_stripes(const I* __restrict__ indptr, const I* __restrict__ indices,
                                     const void* __restrict__ data, uint64_t n, uint64_t nnz,
                                     const uint32_t* __restrict__ perm, const uint32_t* __restrict__ local,
                                     const int64_t* __restrict__ pos, I* __restrict__ out_indices,
                                     void* __restrict__ out_data, uint64_t p, uint64_t first, uint64_t step, StatsOut* so) {
  if (p >= n) return;
  const uint64_t u = perm[p];
  uint64_t b, e;
  if (u >= n || !row_range(indptr, u, nnz, &b, &e, so)) return;
  const uint64_t d = (uint64_t)pos[p];
  for (uint64_t j = b + first; j < e; j += step)
    split_entry<I, VB>(indices, data, n, nnz, local, out_indices, out_data, j, d + (j - b), so);
}

template <class I, int VB>
__global__ void __launch_bounds__(256) k_split_long(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                    const void* __restrict__ data, uint64_t n, uint64_t nnz,
                                                    const uint32_t* __restrict__ perm, const uint32_t* __restrict__ local,
                                                    const int64_t* __restrict__ pos, I* __restrict__ out_indices,
                                                    void* __restrict__ out_data, const uint32_t* __restrict__ long_rows,
                                                    uint64_t long_cap, const uint32_t* __restrict__ huge_rows,
                                                    uint64_t huge_cap, const SplitQueues* sq, StatsOut* so) {
  const uint64_t n_long = sq->n_long < long_cap ? sq->n_long : long_cap;
  const uint64_t n_huge = sq->n_huge < huge_cap ? sq->n_huge : huge_cap;
  for (uint64_t w = blockIdx.x; w < n_long; w += gridDim.x)
    split_stripes<I, VB>(indptr, indices, data, n, nnz, perm, local, pos, out_indices, out_data, long_rows[w], threadIdx.x,
                         256, so);
  for (uint64_t w = 0; w < n_huge; w++)
    split_stripes<I, VB>(indptr, indices, data, n, nnz, perm, local, pos, out_indices, out_data, huge_rows[w],
                         (uint64_t)blockIdx.x * 256 + threadIdx.x, (uint64_t)gridDim.x * 256, so);
}

}  // namespace g2n
