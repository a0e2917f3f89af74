// g2n_pairs.hip — node-to-node distances over a device-resident CSR (g2n_csr_pair_distances): what
// the reference's genome_distance(G, A, B, method="mean") takes from |A| x |B| calls of NetworkX's
// shortest_path_length (gfa2network/analysis.py:142-159), as ceil(|A| / 64) bit-parallel searches.
//
// Sources and targets are two int64 id lists, in list order, duplicates kept, -1 = no node (a source
// that reaches nothing, a target nothing reaches).  Bit b of batch k is SOURCE OCCURRENCE 64 * k + b
// — not a path.  The search is g2n_dist.hip's, unchanged (seen / next, k_dist_expand /
// k_dist_expand_long, the frontier_* skeleton); only what happens when v enters the frontier at level
// L with the new bits B differs:
//   G2N_PAIR_SUMS   C[i] += tcnt[v], S[i] += L * tcnt[v] for every bit i of B, tcnt[v] = how often v
//                   stands in the targets.  With a large target list every discovered node is a
//                   target, so the 64 global counters are not touched per node: a workgroup stages
//                   its counts in LDS (64-bit counters, ds_add_u64 — a count is below 2^32 and a
//                   level below 2^31, so neither they nor L * count can wrap) and flushes once.
//                   wide    within one collect launch L is constant: 64 counts, S += L * count, at
//                           most one global atomic pair per non-zero bit and block.
//                   narrow  S and C of the 64 bits stay in LDS over all the levels of a launch
//                           (1 KB beside the 56 KB of queues) and are flushed when it leaves —
//                           frontier empty, queue overflow or budget spent alike.
//   G2N_PAIR_TABLE  D[base + i][t] = L for every bit i of B and every position t at which v stands
//                   in the targets (a counting sort of the positions by node: k_pair_ids, the
//                   existing scan, k_pair_fill).  (v, bit) is discovered once, so each cell is
//                   written once, by one thread.
// Weighted table: g2n_wdist.hip's batch search with every source occurrence as a one-step path
//   (k_pair_wsources); once a batch has converged k_pair_wgather copies D[base + b][t] =
//   dist[targets[t] * B + b] — d_b(v) as Dijkstra returns it, bit for bit, +inf where not reached.
//   There is no weighted sum: a float sum's order is the contract, and the host folds the table.
// Every id read from the caller's lists is range-checked before it addresses anything (k_pair_ids,
// DistState::bad -> G2N_E_ARG), and again where it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2n_wdist.hip"

namespace g2n {

// ids[0, count): -1 is no node, anything else outside [0, n) is refused; cnt (null: not wanted)
// counts a node's occurrences
__global__ void __launch_bounds__(256) k_pair_ids(const int64_t* __restrict__ ids, uint64_t count, uint64_t n,
                                                  uint32_t* __restrict__ cnt, DistState* st) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const int64_t v = ids[t];
  if (v == -1) return;
  if (v < 0 || (uint64_t)v >= n) {
    st->bad = 1u;
    return;
  }
  if (cnt) atomicAdd(cnt + v, 1u);
}

// the targets' positions sorted by node: mem_pos[mem_ptr[v] .. mem_ptr[v + 1]) = the t with targets[t] == v
__global__ void __launch_bounds__(256) k_pair_fill(const int64_t* __restrict__ targets, uint64_t n_tgt, uint64_t n,
                                                   uint32_t* __restrict__ cursor, uint32_t* __restrict__ mem_pos) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tgt) return;
  const int64_t v = targets[t];
  if (v < 0 || (uint64_t)v >= n) return;
  const uint32_t p = atomicAdd(cursor + v, 1u);
  if (p < n_tgt) mem_pos[p] = (uint32_t)t;
}

// the sources of one batch, occurrences [i0, i1) with i1 - i0 <= 64: level 0's discoveries
__global__ void __launch_bounds__(64) k_pair_sources(const int64_t* __restrict__ sources, uint64_t i0, uint64_t i1,
                                                     uint64_t n, unsigned long long* __restrict__ seen,
                                                     unsigned long long* __restrict__ next) {
  const uint64_t i = i0 + threadIdx.x;
  if (i >= i1) return;
  const int64_t v = sources[i];
  if (v < 0 || (uint64_t)v >= n) return;
  const unsigned long long m = 1ull << (i - i0);
  atomicOr(seen + v, m);
  atomicOr(next + v, m);
}

struct PairAcc {
  const uint32_t* tcnt;      // sums: n + 1, a node's occurrences in the targets
  const uint32_t* mem_ptr;   // table: n + 1
  const uint32_t* mem_pos;   // table: n_tgt positions, by node
  uint32_t* D;               // table: n_src x n_tgt
  unsigned long long* S;     // sums: n_src each
  unsigned long long* C;
  uint64_t n_tgt;
  uint64_t base;             // the batch's first source occurrence
  uint32_t nb;               // its occurrences (<= 64)
  // table: v entered the frontier at level L with the new bits B
  __device__ inline void cells(uint32_t v, unsigned long long B, uint32_t L) const {
    const uint32_t b = mem_ptr[v], e = mem_ptr[v + 1];
    for (uint32_t q = b; q < e && q < n_tgt; q++) {
      const uint64_t t = mem_pos[q];
      if (t >= n_tgt) continue;
      unsigned long long bits = B;
      while (bits) {
        const uint32_t i = (uint32_t)__builtin_ctzll(bits);
        bits &= bits - 1;
        if (i < nb) D[(base + i) * n_tgt + t] = L;
      }
    }
  }
  // sums: m target occurrences at v for every bit of B, into a workgroup's 64 LDS counters
  static __device__ inline void stage(unsigned long long* s_c, unsigned long long B, unsigned long long m) {
    while (B) {
      const uint32_t i = (uint32_t)__builtin_ctzll(B);
      B &= B - 1;
      atomicAdd(s_c + i, m);
    }
  }
  // ... and a workgroup's counters of bit i = threadIdx.x into the call's (after a __syncthreads())
  __device__ inline void flush(unsigned long long sum, unsigned long long cnt) const {
    const uint32_t i = threadIdx.x;
    if (i >= nb || !cnt) return;
    atomicAdd(C + base + i, cnt);
    if (sum) atomicAdd(S + base + i, sum);
  }
};

template <bool kTable>
__global__ void __launch_bounds__(256) k_pair_collect(unsigned long long* __restrict__ next, uint64_t n, uint32_t L,
                                                      uint32_t* __restrict__ queue,
                                                      unsigned long long* __restrict__ qmask, PairAcc acc,
                                                      DistState* st) {
  __shared__ unsigned long long s_c[64];
  if (!kTable) {
    if (threadIdx.x < 64) s_c[threadIdx.x] = 0;
    __syncthreads();
  }
  frontier_collect(next, n, L, queue, qmask, st, [&](uint32_t v, unsigned long long B, uint32_t lv) {
    if (kTable) {
      acc.cells(v, B, lv);
    } else {
      const uint32_t m = acc.tcnt[v];
      if (m) PairAcc::stage(s_c, B, m);
    }
  });
  if (!kTable) {
    __syncthreads();
    if (threadIdx.x < 64) acc.flush(s_c[threadIdx.x] * L, s_c[threadIdx.x]);
  }
}

template <class I, bool kTable>
__global__ void __launch_bounds__(kDistNarrowTPB) k_pair_narrow(const I* __restrict__ indptr,
                                                                const I* __restrict__ indices, uint64_t n, uint64_t nnz,
                                                                unsigned long long* __restrict__ seen,
                                                                unsigned long long* __restrict__ next,
                                                                uint32_t* __restrict__ queue,
                                                                unsigned long long* __restrict__ qmask, PairAcc acc,
                                                                DistState* st, uint32_t budget) {
  __shared__ unsigned long long s_s[64], s_c[64];
  if (!kTable) {
    if (threadIdx.x < 64) s_s[threadIdx.x] = s_c[threadIdx.x] = 0;
    __syncthreads();
  }
  // (every thread leaves frontier_narrow at the same point: its exits test workgroup-uniform values)
  frontier_narrow(
      indptr, n, nnz, next, queue, qmask, st, budget,
      [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        dist_relax_row(indices, n, b, e, 0u, 1u, m, seen, st, push);
      },
      [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        dist_relax_row(indices, n, b, e, threadIdx.x, kDistNarrowTPB, m, seen, st, push);
      },
      [&](uint32_t v, unsigned long long B, uint32_t L) {
        if (kTable) {
          acc.cells(v, B, L);
        } else {
          const unsigned long long m = acc.tcnt[v];
          if (m) {
            PairAcc::stage(s_c, B, m);
            PairAcc::stage(s_s, B, m * L);
          }
        }
      });
  if (!kTable) {
    __syncthreads();
    if (threadIdx.x < 64) acc.flush(s_s[threadIdx.x], s_c[threadIdx.x]);
  }
}

// weighted: the sources of one batch, occurrences [i0, i0 + nb) as the bits of dist's B columns
__global__ void __launch_bounds__(64) k_pair_wsources(const int64_t* __restrict__ sources, uint64_t i0, uint32_t nb,
                                                      uint64_t n, uint32_t B, unsigned long long* __restrict__ dist,
                                                      unsigned long long* __restrict__ next) {
  const uint32_t b = threadIdx.x;
  if (b >= nb || b >= B) return;
  const int64_t v = sources[i0 + b];
  if (v < 0 || (uint64_t)v >= n) return;
  atomicMin(dist + (uint64_t)v * B + b, 0ull);
  atomicOr(next + v, 1ull << b);
}

// weighted, after the batch's nb <= B searches have converged: D[i0 + b][t] = d_b(targets[t]), the
// float64's bits (+inf: not reached, or no node)
__global__ void __launch_bounds__(256) k_pair_wgather(const int64_t* __restrict__ targets, uint64_t n_tgt, uint64_t n,
                                                      const unsigned long long* __restrict__ dist, uint32_t B,
                                                      uint32_t nb, uint64_t i0, unsigned long long* __restrict__ D) {
  const uint64_t stride = (uint64_t)gridDim.x * 256, cells = n_tgt * nb;
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += stride) {
    const uint64_t t = k / nb;
    const uint32_t b = (uint32_t)(k % nb);
    const int64_t v = targets[t];
    D[(i0 + b) * n_tgt + t] = (v < 0 || (uint64_t)v >= n) ? kWDistInf : dist[(uint64_t)v * B + b];
  }
}

}  // namespace g2n
