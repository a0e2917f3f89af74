// g2n_wdist.hip — weighted shortest-path distances between paths over a device-resident CSR
// (g2n_csr_path_distances_weighted): what the reference's distance helpers take from NetworkX's
// multi_source_dijkstra_path_length(G, nodes, weight="weight") on a graph built with a weight_tag.
// Every stored entry k of row u is an edge u -> indices[k] of length values[k] (float64, finite,
// >= 0; repeated (u, v) are parallel edges, an explicit zero is an edge of length 0).
//
// d_i(v) = the smallest left-to-right float64 sum ((0.0 + w1) + w2) + ... over the walks from a step
//   of path i to v.  IEEE addition is monotone (a <= b implies a + w <= b + w), so that minimum is
//   the one fixed point of d(v) = min(d(v), d(u) + w(u, v)) below the start values — what Dijkstra
//   returns, bit for bit, in whatever order the relaxations run.
// State of a batch of B <= 64 paths: dist[v * B + b], the float64's bit pattern (non-negative
//   doubles order as unsigned integers; +inf = kWDistInf = not reached), and one mask word next[v]:
//   the paths whose distance at v improved since v was last expanded.  Both are written by
//   device-scope atomics only and read, inside a kernel, through an atomic's return or a relaxed
//   agent-scope load (g2n_dist.hip: an L1 line another CU rewrote stays stale).
// Expanding u with mask m, for every bit b of m: du = dist[u][b]; for every stored (u, v, w):
//   t = du + w; old = atomicMin(dist[v][b], bits(t)); t < old -> atomicOr(next + v, bit b).  The
//   comparison is strict: a zero-length cycle improves nothing and is not queued again.  The bit is
//   set after the minimum, the word is taken before du is read, so the expansion that follows an
//   improvement reads it (or a later one).
// Rounds: round r expands every node whose word was set in round r - 1 (round 0: the sources).  A
//   node whose shortest walk has h edges is final after round h at the latest (induction over h, as
//   for synchronous Bellman-Ford; a value read in mid-round is only lower), so the last round that
//   improves anything is at most n - 1.  The host counts the rounds and fails past n.
//   wide    k_wdist_collect (every non-zero word of next is taken and queued), k_wdist_expand /
//           k_wdist_expand_long (a row past kStatsShortRow entries by a block).
//   narrow  k_wdist_narrow: at most kDistNarrowCap queued nodes — ONE workgroup carries the search
//           from round to round with both queues in LDS, for up to kDistLevelBudget rounds a
//           launch; it leaves when the frontier empties, when a queue would overflow (after the
//           round's expansion: dist / next are complete, the wide collect rebuilds the frontier
//           from next) or when the budget is spent (the frontier goes back to queue / qmask).
//   Both regimes are g2n_dist.hip's frontier_* templates with this file's row bodies.
//   No workgroup waits on another; every loop runs over a row, a queue, a mask's bits or a budget.
// Tables, once a batch has converged: D[i][j] = min over the steps of j (atomicMin on the bit
//   patterns, one thread per step: the minimum does not depend on the order); S[i][j] / C[i][j] by
//   one thread per cell that walks path j's steps in order — the sum's order is the contract.
// Every index read from the caller's arrays is range-checked before it addresses anything, and the
// values are checked whole before anything is searched (DistState::bad -> G2N_E_ARG).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2n_dist.hip"

namespace g2n {

constexpr unsigned long long kWDistInf = 0x7FF0000000000000ull;  // +inf: not reached

// every value finite and >= 0 (-0.0 is 0): one pass, before anything is searched
__global__ void __launch_bounds__(256) k_wdist_values(const double* __restrict__ values, uint64_t nnz, DistState* st) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  uint32_t bad = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
    const double w = values[j];
    bad |= !(w >= 0.0 && w < __longlong_as_double((long long)kWDistInf));  // (a NaN fails both)
  }
  if (bad) st->bad = 1u;
}

__global__ void __launch_bounds__(256) k_wdist_fill(unsigned long long* __restrict__ p, uint64_t count,
                                                    unsigned long long x) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) p[i] = x;
}

// the sources of one batch, steps [s0, s1) of paths [base, base + B): distance 0.0, round 0's frontier
__global__ void __launch_bounds__(256) k_wdist_sources(const int64_t* __restrict__ path_nodes, uint64_t s0, uint64_t s1,
                                                       uint64_t n, const uint32_t* __restrict__ step_path,
                                                       uint32_t base, uint32_t B, unsigned long long* __restrict__ dist,
                                                       unsigned long long* __restrict__ next) {
  const uint64_t s = s0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= s1) return;
  const int64_t v = path_nodes[s];
  const uint32_t b = step_path[s] - base;
  if (v < 0 || (uint64_t)v >= n || b >= B) return;
  atomicMin(dist + (uint64_t)v * B + b, 0ull);
  atomicOr(next + v, 1ull << b);
}

// wide: every node whose word in next is set joins round R's frontier (queue capacity n)
__global__ void __launch_bounds__(256) k_wdist_collect(unsigned long long* __restrict__ next, uint64_t n, uint32_t R,
                                                       uint32_t* __restrict__ queue,
                                                       unsigned long long* __restrict__ qmask, DistState* st) {
  frontier_collect(next, n, R, queue, qmask, st, [](uint32_t, unsigned long long, uint32_t) {});
}

// dist[v][b] = min(dist[v][b], du + w); true when it improved (strictly)
__device__ inline bool wdist_min(unsigned long long* dist, uint64_t v, uint32_t B, uint32_t b, double du, double w) {
  const unsigned long long t = (unsigned long long)__double_as_longlong(du + w);
  unsigned long long* p = dist + v * B + b;
  if (t >= mask_ld(p)) return false;  // (dist only falls: what fails against an older value fails now)
  return t < atomicMin(p, t);
}

// u's distances of the bits of m, for one thread: du[] is not kept — a short row is walked once per bit
template <class I, class F>
__device__ inline void wdist_row(const I* __restrict__ indices, const double* __restrict__ values, uint64_t n,
                                 uint64_t b, uint64_t e, uint64_t u, unsigned long long m, uint32_t B,
                                 unsigned long long* dist, DistState* st, F&& improved) {
  while (m) {
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1;
    if (bit >= B) continue;
    const unsigned long long db = mask_ld(dist + u * B + bit);
    if (db >= kWDistInf) continue;
    const double du = __longlong_as_double((long long)db);
    for (uint64_t j = b; j < e; j++) {
      const uint64_t c = (uint64_t)indices[j];
      if (c >= n) {
        st->bad = 1u;
        continue;
      }
      if (wdist_min(dist, c, B, bit, du, values[j])) improved(c, bit);
    }
  }
}

template <class I>
__global__ void __launch_bounds__(256) k_wdist_expand(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                      const double* __restrict__ values, uint64_t n, uint64_t nnz,
                                                      uint32_t B, unsigned long long* __restrict__ dist,
                                                      unsigned long long* __restrict__ next,
                                                      const uint32_t* __restrict__ queue,
                                                      const unsigned long long* __restrict__ qmask,
                                                      uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                      DistState* st) {
  frontier_expand(indptr, n, nnz, queue, qmask, long_rows, long_cap, st,
                  [&](uint64_t u, uint64_t b, uint64_t e, unsigned long long m) {
                    wdist_row(indices, values, n, b, e, u, m, B, dist, st,
                              [&](uint64_t c, uint32_t bit) { atomicOr(next + c, 1ull << bit); });
                  });
}

// a long row by the block: u's distances once into LDS, then an entry per thread and every bit of m
template <class I, class F>
__device__ inline void wdist_long_row(const I* __restrict__ indices, const double* __restrict__ values, uint64_t n,
                                      uint64_t b, uint64_t e, uint64_t u, unsigned long long m, uint32_t B,
                                      unsigned long long* dist, DistState* st, unsigned long long* s_du, uint32_t tpb,
                                      F&& improved) {
  if (threadIdx.x < 64)
    s_du[threadIdx.x] = (threadIdx.x < B && ((m >> threadIdx.x) & 1ull)) ? mask_ld(dist + u * B + threadIdx.x)
                                                                           : kWDistInf;
  __syncthreads();
  for (uint64_t j = b + threadIdx.x; j < e; j += tpb) {
    const uint64_t c = (uint64_t)indices[j];
    if (c >= n) {
      st->bad = 1u;
      continue;
    }
    const double w = values[j];
    unsigned long long bits = m;
    while (bits) {
      const uint32_t bit = (uint32_t)__builtin_ctzll(bits);
      bits &= bits - 1;
      const unsigned long long db = s_du[bit];
      if (db >= kWDistInf) continue;
      if (wdist_min(dist, c, B, bit, __longlong_as_double((long long)db), w)) improved(c, bit);
    }
  }
  __syncthreads();  // (s_du is the next row's)
}

template <class I>
__global__ void __launch_bounds__(256) k_wdist_expand_long(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                           const double* __restrict__ values, uint64_t n, uint64_t nnz,
                                                           uint32_t B, unsigned long long* __restrict__ dist,
                                                           unsigned long long* __restrict__ next,
                                                           const uint32_t* __restrict__ queue,
                                                           const unsigned long long* __restrict__ qmask,
                                                           const uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                           DistState* st) {
  __shared__ unsigned long long s_du[64];
  frontier_expand_long(indptr, n, nnz, queue, qmask, long_rows, long_cap, st,
                       [&](uint64_t u, uint64_t b, uint64_t e, unsigned long long m) {
                         wdist_long_row(indices, values, n, b, e, u, m, B, dist, st, s_du, 256u,
                                        [&](uint64_t c, uint32_t bit) { atomicOr(next + c, 1ull << bit); });
                       });
}

// narrow (frontier_narrow, g2n_dist.hip): a level is a round; a queued node is one whose distance
// improved for some path, so nothing is accumulated when its word is taken
template <class I>
__global__ void __launch_bounds__(kDistNarrowTPB) k_wdist_narrow(const I* __restrict__ indptr,
                                                                 const I* __restrict__ indices,
                                                                 const double* __restrict__ values, uint64_t n,
                                                                 uint64_t nnz, uint32_t B,
                                                                 unsigned long long* __restrict__ dist,
                                                                 unsigned long long* __restrict__ next,
                                                                 uint32_t* __restrict__ queue,
                                                                 unsigned long long* __restrict__ qmask, DistState* st,
                                                                 uint32_t budget) {
  __shared__ unsigned long long s_du[64];
  frontier_narrow(
      indptr, n, nnz, next, queue, qmask, st, budget,
      [&](uint64_t u, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        wdist_row(indices, values, n, b, e, u, m, B, dist, st, [&](uint64_t c, uint32_t bit) { push(c, 1ull << bit); });
      },
      [&](uint64_t u, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        wdist_long_row(indices, values, n, b, e, u, m, B, dist, st, s_du, kDistNarrowTPB,
                       [&](uint64_t c, uint32_t bit) { push(c, 1ull << bit); });
      },
      [](uint32_t, unsigned long long, uint32_t) {});
}

// min, after the batch's nb <= B searches have converged: step s of path j lowers D[base + b][j] to
// d_b(its node) — bit patterns of non-negative doubles, D starts as kWDistInf
__global__ void __launch_bounds__(256) k_wdist_min(const int64_t* __restrict__ path_nodes, uint64_t steps, uint64_t n,
                                                   const uint32_t* __restrict__ step_path, uint64_t K,
                                                   const unsigned long long* __restrict__ dist, uint32_t B, uint32_t nb,
                                                   uint32_t base, unsigned long long* __restrict__ D) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= steps) return;
  const int64_t v = path_nodes[s];
  const uint64_t j = step_path[s];
  if (v < 0 || (uint64_t)v >= n || j >= K) return;
  for (uint32_t b = 0; b < nb; b++) {
    const unsigned long long d = dist[(uint64_t)v * B + b];
    unsigned long long* cell = D + (uint64_t)(base + b) * K + j;
    if (d < mask_ld(cell)) atomicMin(cell, d);  // (a cell only falls; the load spares the path's one cell most of its steps)
  }
}

// mean: cell (base + b, j) by one thread, path j's steps in order, left to right from 0.0
__global__ void __launch_bounds__(256) k_wdist_mean(const int64_t* __restrict__ path_ptr,
                                                    const int64_t* __restrict__ path_nodes, uint64_t steps, uint64_t n,
                                                    uint64_t K, const unsigned long long* __restrict__ dist, uint32_t B,
                                                    uint32_t nb, uint32_t base, double* __restrict__ S,
                                                    unsigned long long* __restrict__ C) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= K * nb) return;
  const uint32_t b = (uint32_t)(t % nb);
  const uint64_t j = t / nb;
  const int64_t lo = path_ptr[j], hi = path_ptr[j + 1];
  double sum = 0.0;
  unsigned long long cnt = 0;
  if (lo >= 0 && lo <= hi && (uint64_t)hi <= steps)
    for (int64_t s = lo; s < hi; s++) {
      const int64_t v = path_nodes[s];
      if (v < 0 || (uint64_t)v >= n) continue;
      const unsigned long long d = dist[(uint64_t)v * B + b];
      if (d >= kWDistInf) continue;
      sum += __longlong_as_double((long long)d);
      cnt++;
    }
  S[(uint64_t)(base + b) * K + j] = sum;
  C[(uint64_t)(base + b) * K + j] = cnt;
}

// mean-fold (G2N_DIST_MEAN_FOLD), after the batch's k_wdist_mean: cell (i = base + b, j > i) by one
// thread again, the same walk over path j's steps — but from the seed S[j][i], the total over path
// i's steps of d_j, which row j's own k_wdist_mean wrote (path j is in this batch, or in a later one:
// the batches run from the last to the first).  The seeds are cells below the diagonal, the results
// cells above it: no cell this kernel reads is one it writes.  C is not touched.
__global__ void __launch_bounds__(256) k_wdist_mean_fold(const int64_t* __restrict__ path_ptr,
                                                         const int64_t* __restrict__ path_nodes, uint64_t steps,
                                                         uint64_t n, uint64_t K,
                                                         const unsigned long long* __restrict__ dist, uint32_t B,
                                                         uint32_t nb, uint32_t base, double* S) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= K * nb) return;
  const uint32_t b = (uint32_t)(t % nb);
  const uint64_t j = t / nb, i = (uint64_t)base + b;
  if (j <= i) return;
  const int64_t lo = path_ptr[j], hi = path_ptr[j + 1];
  double sum = S[j * K + i];
  if (lo >= 0 && lo <= hi && (uint64_t)hi <= steps)
    for (int64_t s = lo; s < hi; s++) {
      const int64_t v = path_nodes[s];
      if (v < 0 || (uint64_t)v >= n) continue;
      const unsigned long long d = dist[(uint64_t)v * B + b];
      if (d >= kWDistInf) continue;
      sum += __longlong_as_double((long long)d);
    }
  S[i * K + j] = sum;
}

}  // namespace g2n
