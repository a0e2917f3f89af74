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
//           from round to round with both queues in LDS, for up to kWDistRoundBudget rounds a
//           launch; it leaves when the frontier empties, when a queue would overflow (after the
//           round's expansion: dist / next are complete, the wide collect rebuilds the frontier
//           from next) or when the budget is spent (the frontier goes back to queue / qmask).
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
constexpr uint32_t kWDistRoundBudget = 8192;                     // rounds one k_wdist_narrow launch may run

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
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += stride) {
    if (!mask_ld(next + v)) continue;
    const unsigned long long m = atomicExch(next + v, 0ull);
    if (!m) continue;
    const uint32_t k = atomicAdd(&st->count, 1u);
    if (k >= n) continue;  // (cannot be: a node is taken once)
    queue[k] = (uint32_t)v;
    qmask[k] = m;
    if (k == 0) {
      st->level = R;
      st->last_level = R;
    }
  }
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
  uint64_t count = st->count;
  if (count > n) count = n;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += stride) {
    const uint64_t u = queue[k];
    if (u >= n) continue;
    uint64_t b, e;
    if (!dist_row(indptr, u, nnz, &b, &e, st)) continue;
    if (e - b > kStatsShortRow) {
      const uint32_t w = atomicAdd(&st->n_long, 1u);
      if (w < long_cap) long_rows[w] = (uint32_t)k;
      else st->bad = 1u;
      continue;
    }
    wdist_row(indices, values, n, b, e, u, qmask[k], B, dist, st,
              [&](uint64_t c, uint32_t bit) { atomicOr(next + c, 1ull << bit); });
  }
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
  uint64_t n_long = st->n_long, count = st->count;
  if (n_long > long_cap) n_long = long_cap;
  if (count > n) count = n;
  for (uint64_t w = blockIdx.x; w < n_long; w += gridDim.x) {  // (everything up to the row is the block's: no thread leaves alone)
    const uint64_t k = long_rows[w];
    if (k >= count) continue;
    const uint64_t u = queue[k];
    if (u >= n) continue;
    uint64_t b, e;
    if (!dist_row(indptr, u, nnz, &b, &e, st)) continue;
    wdist_long_row(indices, values, n, b, e, u, qmask[k], B, dist, st, s_du, 256u,
                   [&](uint64_t c, uint32_t bit) { atomicOr(next + c, 1ull << bit); });
  }
}

// narrow: one workgroup, from the collected frontier in queue / qmask (st->count <= kDistNarrowCap
// nodes of round st->level) until the frontier empties (count = 0), a queue would overflow (pending
// = 1: next holds round `level`'s frontier, uncollected) or `budget` rounds have run (the frontier
// is written back to queue / qmask).
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
  __shared__ unsigned long long qm[2][kDistNarrowCap];
  __shared__ uint32_t qv[2][kDistNarrowCap];
  __shared__ uint32_t s_long[kDistNarrowCap];  // frontier slots whose row the whole block walks
  __shared__ unsigned long long s_du[64];
  __shared__ uint32_t s_cnt[2], s_nlong, s_over;
  const uint32_t tid = threadIdx.x;
  uint32_t cnt = st->count, R = st->level, cur = 0;
  if (cnt > kDistNarrowCap || budget == 0) return;  // (the host launches it only below the cap)
  for (uint32_t k = tid; k < cnt; k += kDistNarrowTPB) {
    qv[0][k] = queue[k];
    qm[0][k] = qmask[k];
  }
  if (tid == 0) {
    s_cnt[0] = s_cnt[1] = 0;
    s_nlong = 0;
    s_over = 0;
  }
  __syncthreads();
  for (uint32_t it = 0;; it++) {
    const uint32_t nx = cur ^ 1u;
    // the thread that finds next[c] zero queues c (one per node and round)
    auto improved = [&](uint64_t c, uint32_t bit) {
      if (atomicOr(next + c, 1ull << bit)) return;
      const uint32_t p = atomicAdd(&s_cnt[nx], 1u);
      if (p < kDistNarrowCap) qv[nx][p] = (uint32_t)c;
      else s_over = 1u;
    };
    // ---- expand round R's frontier: short rows by a thread each, longer ones by the block
    for (uint32_t k = tid; k < cnt; k += kDistNarrowTPB) {
      const uint64_t u = qv[cur][k];
      uint64_t b, e;
      if (u >= n || !dist_row(indptr, u, nnz, &b, &e, st)) continue;
      if (e - b > kStatsShortRow) {
        s_long[atomicAdd(&s_nlong, 1u)] = k;  // (at most cnt <= kDistNarrowCap of them)
        continue;
      }
      wdist_row(indices, values, n, b, e, u, qm[cur][k], B, dist, st, improved);
    }
    __syncthreads();
    const uint32_t nl = s_nlong;
    for (uint32_t w = 0; w < nl; w++) {
      const uint32_t k = s_long[w];
      const uint64_t u = qv[cur][k];
      uint64_t b, e;
      if (!dist_row(indptr, u, nnz, &b, &e, st)) continue;  // (the same answer in every thread)
      wdist_long_row(indices, values, n, b, e, u, qm[cur][k], B, dist, st, s_du, kDistNarrowTPB, improved);
    }
    __syncthreads();
    // every atomic of the round has returned: dist / next are complete for round R + 1
    const uint32_t ncnt = s_cnt[nx], over = s_over;
    R++;
    if (over) {
      if (tid == 0) {
        st->count = 0;
        st->pending = 1u;
        st->level = R;
      }
      return;
    }
    if (ncnt == 0) {
      if (tid == 0) {
        st->count = 0;
        st->pending = 0;
        st->level = R;
        st->last_level = R - 1;
      }
      return;
    }
    // ---- collect round R + 1: take each queued node's word
    for (uint32_t k = tid; k < ncnt; k += kDistNarrowTPB) qm[nx][k] = atomicExch(next + qv[nx][k], 0ull);
    if (tid == 0) {
      s_cnt[cur] = 0;
      s_nlong = 0;
    }
    __syncthreads();
    cur = nx;
    cnt = ncnt;
    if (it + 1 >= budget) {
      for (uint32_t k = tid; k < cnt; k += kDistNarrowTPB) {
        queue[k] = qv[cur][k];
        qmask[k] = qm[cur][k];
      }
      if (tid == 0) {
        st->count = cnt;
        st->pending = 0;
        st->level = R;
        st->last_level = R;
      }
      return;
    }
  }
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

}  // namespace g2n
