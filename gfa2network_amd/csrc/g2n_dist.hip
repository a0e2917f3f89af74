// g2n_dist.hip — hop distances between paths over a device-resident CSR structure
// (g2n_csr_path_distances): what the reference's genome_distance_matrix takes from one NetworkX
// multi-source Dijkstra per path (gfa2network/analysis.py), as a bit-parallel breadth-first search.
// Every edge weighs 1 there, so Dijkstra is BFS.  The values are never read.
//
// Membership, node -> paths: a counting sort of the steps by node (k_dist_steps histogram, the
//   existing scan, k_dist_fill).  A repeated (node, path) stays: it is the multiplicity mean needs.
// Search: the paths are taken 64 at a time; bit b of a node's word in seen / next is path
//   64 * batch + b.  Expanding frontier node u with mask m, every stored (u, v):
//   old = atomicOr(seen + v, m); nw = m & ~old; atomicOr(next + v, nw) when nw — each (v, bit) is
//   discovered exactly once, at its true level.  seen / next are written by device-scope atomics
//   only and read, inside a kernel, through an atomic's return or a relaxed agent-scope load (an
//   L1 line another CU rewrote stays stale).
//   wide    k_dist_collect: one pass over all n words of next — a non-zero word is taken (exchanged
//           for 0), queued with its mask and accumulated; k_dist_expand / k_dist_expand_long walk
//           the queue's rows (a row past kStatsShortRow entries by a block).  The host reads the
//           state after every collect.
//   narrow  k_dist_narrow: at most kDistNarrowCap frontier nodes — ONE workgroup carries the search
//           from level to level with both queues in LDS and a __syncthreads() between the phases,
//           for up to kDistLevelBudget levels per launch: a chain's million levels cost a launch
//           and a read-back per budget, not per level.  The thread whose atomicOr finds next[v]
//           zero queues v (one per node and level).  A queue that would overflow ends the launch
//           after the level's expansion: seen / next are complete then, and the wide collect
//           rebuilds the frontier from next.
//   The two regimes' walks, queues and hand-over are the frontier_* templates below, which the
//   weighted search (g2n_wdist.hip) runs with its own row bodies and the node-to-node search
//   (g2n_pairs.hip) with its own accumulation; the host's loop over them is run_frontier
//   (g2n_queries.hip).
// Accumulation, when v enters the frontier at level L with new bits B, for v's membership entries j:
//   min   todo = B & ~done[j] (one load); if any, the bits the atomicOr on done[j] newly set store L
//         into D[i][j] — each cell is written once, by one thread.
//   mean  C[i][j] += 1, S[i][j] += L for every bit i of B (64-bit atomics).
// Every index read from the caller's arrays is range-checked before it addresses anything
// (DistState::bad; the call then fails with G2N_E_ARG).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2n_stats.hip"

namespace g2n {

constexpr uint32_t kDistNarrowCap = 2048;     // frontier nodes one workgroup carries (2 LDS queues: 56 KB)
constexpr uint32_t kDistLevelBudget = 8192;   // levels one k_dist_narrow launch may run
constexpr uint32_t kDistNarrowTPB = 256;
constexpr uint32_t kDistUnreached = 0xFFFFFFFFu;

struct DistState {
  uint32_t count;       // frontier nodes in queue / qmask (collected, not expanded yet)
  uint32_t n_long;      // rows queued for k_dist_expand_long
  uint32_t pending;     // 1: next holds level `level`'s discoveries, uncollected (a narrow queue overflowed)
  uint32_t level;       // the frontier's level
  uint32_t last_level;  // the deepest level at which a node was discovered
  uint32_t bad;
};

__device__ inline unsigned long long mask_ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class I>
__device__ inline bool dist_row(const I* __restrict__ indptr, uint64_t i, uint64_t nnz, uint64_t* b, uint64_t* e,
                                DistState* st) {
  const int64_t lo = (int64_t)indptr[i], hi = (int64_t)indptr[i + 1];
  if (lo < 0 || hi < lo || (uint64_t)hi > nnz) {
    st->bad = 1u;
    return false;
  }
  *b = (uint64_t)lo;
  *e = (uint64_t)hi;
  return true;
}

// the whole structure once, before anything is searched (a search reads only the rows it reaches)
template <class I>
__global__ void __launch_bounds__(256) k_dist_check(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                    uint64_t n, uint64_t nnz, DistState* st) {
  const uint64_t stride = (uint64_t)gridDim.x * 256, t0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0;
  for (uint64_t i = t0; i < n; i += stride) {
    const int64_t lo = (int64_t)indptr[i], hi = (int64_t)indptr[i + 1];
    bad |= lo < 0 || hi < lo || (uint64_t)hi > nnz;
  }
  for (uint64_t j = t0; j < nnz; j += stride) {
    const int64_t c = (int64_t)indices[j];
    bad |= c < 0 || (uint64_t)c >= n;
  }
  if (t0 == 0 && n) bad |= (int64_t)indptr[0] < 0;
  if (bad) st->bad = 1u;
}

// path_ptr is a non-decreasing map of [0, K] into [0, steps] (path_ptr[0] == 0 and path_ptr[K] ==
// steps are the host's to check: it read them)
__global__ void __launch_bounds__(256) k_dist_paths_check(const int64_t* __restrict__ path_ptr, uint64_t K,
                                                          uint64_t steps, DistState* st) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int64_t lo = path_ptr[k], hi = path_ptr[k + 1];
  if (lo < 0 || hi < lo || (uint64_t)hi > steps) st->bad = 1u;
}

// step s: its path (the last k with path_ptr[k] <= s < path_ptr[k + 1]) and its node's count
__global__ void __launch_bounds__(256) k_dist_steps(const int64_t* __restrict__ path_ptr,
                                                    const int64_t* __restrict__ path_nodes, uint64_t K, uint64_t steps,
                                                    uint64_t n, uint32_t* __restrict__ step_path,
                                                    uint32_t* __restrict__ cnt, DistState* st) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= steps) return;
  uint64_t lo = 0, hi = K;  // first k in [0, K] whose start is > s
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (path_ptr[mid] <= (int64_t)s) lo = mid + 1;
    else hi = mid;
  }
  step_path[s] = (uint32_t)(lo ? lo - 1 : 0);
  const int64_t v = path_nodes[s];
  if (v == -1) return;  // a step that is no node: never reached, no source
  if (v < 0 || (uint64_t)v >= n) {
    st->bad = 1u;
    return;
  }
  atomicAdd(cnt + v, 1u);
}

// looked-up steps (k_ks_lookup: ~0u = no such key) as path_nodes; *missing = the lowest unknown
// step below n_src (~0 before: none)
__global__ void __launch_bounds__(256) k_dist_resolved(const uint32_t* __restrict__ ids, uint64_t steps, uint64_t n_src,
                                                       int64_t* __restrict__ path_nodes, unsigned long long* missing) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= steps) return;
  const uint32_t id = ids[s];
  path_nodes[s] = id == ~0u ? -1 : (int64_t)id;
  if (id == ~0u && s < n_src) atomicMin(missing, (unsigned long long)s);
}

__global__ void __launch_bounds__(256) k_dist_fill(const int64_t* __restrict__ path_nodes, uint64_t steps, uint64_t n,
                                                   const uint32_t* __restrict__ step_path,
                                                   uint32_t* __restrict__ cursor, uint32_t* __restrict__ mem_path) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= steps) return;
  const int64_t v = path_nodes[s];
  if (v < 0 || (uint64_t)v >= n) return;
  const uint32_t p = atomicAdd(cursor + v, 1u);
  if (p < steps) mem_path[p] = step_path[s];
}

// the sources of one batch, steps [s0, s1) of paths [base, base + 64): level 0's discoveries
__global__ void __launch_bounds__(256) k_dist_sources(const int64_t* __restrict__ path_nodes, uint64_t s0, uint64_t s1,
                                                      uint64_t n, const uint32_t* __restrict__ step_path, uint32_t base,
                                                      unsigned long long* __restrict__ seen,
                                                      unsigned long long* __restrict__ next) {
  const uint64_t s = s0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= s1) return;
  const int64_t v = path_nodes[s];
  const uint32_t b = step_path[s] - base;
  if (v < 0 || (uint64_t)v >= n || b >= 64u) return;
  const unsigned long long m = 1ull << b;
  const unsigned long long old = atomicOr(seen + v, m);
  if (!(old & m)) atomicOr(next + v, m);
}

struct DistAcc {
  const uint32_t* mem_ptr;    // n + 1
  const uint32_t* mem_path;
  unsigned long long* done;   // min: K words of the batch
  uint32_t* D;                // min: K x K, else null
  unsigned long long* S;      // mean: K x K each
  unsigned long long* C;
  uint64_t K;
  uint32_t base;              // the batch's first path
  // v entered the frontier at level L with the new bits B
  __device__ inline void node(uint32_t v, unsigned long long B, uint32_t L) const {
    const uint32_t b = mem_ptr[v], e = mem_ptr[v + 1];
    for (uint32_t q = b; q < e; q++) {
      const uint64_t j = mem_path[q];
      if (j >= K) continue;
      if (D) {
        unsigned long long todo = B & ~mask_ld(done + j);
        if (!todo) continue;
        todo &= ~atomicOr(done + j, todo);
        while (todo) {
          const uint32_t i = (uint32_t)__builtin_ctzll(todo);
          todo &= todo - 1;
          D[(uint64_t)(base + i) * K + j] = L;
        }
      } else {
        unsigned long long bits = B;
        while (bits) {
          const uint32_t i = (uint32_t)__builtin_ctzll(bits);
          bits &= bits - 1;
          const uint64_t cell = (uint64_t)(base + i) * K + j;
          atomicAdd(C + cell, 1ull);
          if (L) atomicAdd(S + cell, (unsigned long long)L);
        }
      }
    }
  }
};

// ---- the frontier skeleton: what the hop search and the weighted one (g2n_wdist.hip) share.  A
// search supplies its row bodies as callables (inlined: a lambda of the kernel that calls); the walk
// over the queue, the long-row hand-off, the LDS queues and the hand-over to the host live here.

// wide: every node whose word in next is set joins level L's frontier (queue capacity n); the taker
// of the word calls taken(v, bits, L)
template <class Taken>
__device__ __forceinline__ void frontier_collect(unsigned long long* __restrict__ next, uint64_t n, uint32_t L,
                                                 uint32_t* __restrict__ queue, unsigned long long* __restrict__ qmask,
                                                 DistState* st, Taken&& taken) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += stride) {
    if (!mask_ld(next + v)) continue;
    const unsigned long long B = atomicExch(next + v, 0ull);
    if (!B) continue;
    const uint32_t k = atomicAdd(&st->count, 1u);
    if (k >= n) continue;  // (cannot be: a node is taken once)
    queue[k] = (uint32_t)v;
    qmask[k] = B;
    if (k == 0) {
      st->level = L;
      st->last_level = L;
    }
    taken((uint32_t)v, B, L);
  }
}

// wide: queue[0, count) by a thread per node — short_row(u, b, e, mask) for a row of at most
// kStatsShortRow entries, a longer one goes to long_rows (its slot in the queue)
template <class I, class Short>
__device__ __forceinline__ void frontier_expand(const I* __restrict__ indptr, uint64_t n, uint64_t nnz,
                                                const uint32_t* __restrict__ queue,
                                                const unsigned long long* __restrict__ qmask,
                                                uint32_t* __restrict__ long_rows, uint64_t long_cap, DistState* st,
                                                Short&& short_row) {
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
    short_row(u, b, e, qmask[k]);
  }
}

// wide: long_rows by a block per row — long_row(u, b, e, mask), the whole block together (everything
// up to the row is the block's: no thread leaves alone, a row body may use __syncthreads())
template <class I, class Long>
__device__ __forceinline__ void frontier_expand_long(const I* __restrict__ indptr, uint64_t n, uint64_t nnz,
                                                     const uint32_t* __restrict__ queue,
                                                     const unsigned long long* __restrict__ qmask,
                                                     const uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                     DistState* st, Long&& long_row) {
  uint64_t n_long = st->n_long, count = st->count;
  if (n_long > long_cap) n_long = long_cap;
  if (count > n) count = n;
  for (uint64_t w = blockIdx.x; w < n_long; w += gridDim.x) {
    const uint64_t k = long_rows[w];
    if (k >= count) continue;
    const uint64_t u = queue[k];
    if (u >= n) continue;
    uint64_t b, e;
    if (!dist_row(indptr, u, nnz, &b, &e, st)) continue;
    long_row(u, b, e, qmask[k]);
  }
}

// narrow: one workgroup of kDistNarrowTPB threads, from the collected frontier in queue / qmask
// (st->count <= kDistNarrowCap nodes of level st->level) until the frontier empties (count = 0), a
// queue would overflow (pending = 1: next holds level `level`'s discoveries, uncollected) or `budget`
// levels have run (the frontier is written back to queue / qmask).
//   short_row(u, b, e, mask, push) by one thread, long_row(u, b, e, mask, push) by the block (the same
//   arguments in every thread).  push(c, bits) sets bits in next[c]; the thread that found the word
//   zero queues c for the next level (one per node and level).
//   taken(v, bits, L): v's word was taken — it is in level L's frontier with those bits.
template <class I, class Short, class Long, class Taken>
__device__ __forceinline__ void frontier_narrow(const I* __restrict__ indptr, uint64_t n, uint64_t nnz,
                                                unsigned long long* __restrict__ next, uint32_t* __restrict__ queue,
                                                unsigned long long* __restrict__ qmask, DistState* st, uint32_t budget,
                                                Short&& short_row, Long&& long_row, Taken&& taken) {
  __shared__ unsigned long long qm[2][kDistNarrowCap];
  __shared__ uint32_t qv[2][kDistNarrowCap];
  __shared__ uint32_t s_long[kDistNarrowCap];  // frontier slots whose row the whole block walks
  __shared__ uint32_t s_cnt[2], s_nlong, s_over;
  const uint32_t tid = threadIdx.x;
  uint32_t cnt = st->count, L = st->level, cur = 0;
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
    auto push = [&](uint64_t c, unsigned long long bits) {
      if (atomicOr(next + c, bits)) return;  // queued by the thread that found the word zero
      const uint32_t p = atomicAdd(&s_cnt[nx], 1u);
      if (p < kDistNarrowCap) qv[nx][p] = (uint32_t)c;
      else s_over = 1u;
    };
    // ---- expand level L: short rows by a thread each, longer ones by the block
    for (uint32_t k = tid; k < cnt; k += kDistNarrowTPB) {
      const uint64_t u = qv[cur][k];
      uint64_t b, e;
      if (u >= n || !dist_row(indptr, u, nnz, &b, &e, st)) continue;
      if (e - b > kStatsShortRow) {
        s_long[atomicAdd(&s_nlong, 1u)] = k;  // (at most cnt <= kDistNarrowCap of them)
        continue;
      }
      short_row(u, b, e, qm[cur][k], push);
    }
    __syncthreads();
    const uint32_t nl = s_nlong;
    for (uint32_t w = 0; w < nl; w++) {
      const uint32_t k = s_long[w];
      const uint64_t u = qv[cur][k];
      uint64_t b, e;
      if (!dist_row(indptr, u, nnz, &b, &e, st)) continue;  // (the same answer in every thread)
      long_row(u, b, e, qm[cur][k], push);
    }
    __syncthreads();
    // every atomic of the level has returned: the search's state and next are complete for level L + 1
    const uint32_t ncnt = s_cnt[nx], over = s_over;
    L++;
    if (over) {
      if (tid == 0) {
        st->count = 0;
        st->pending = 1u;
        st->level = L;
      }
      return;
    }
    if (ncnt == 0) {
      if (tid == 0) {
        st->count = 0;
        st->pending = 0;
        st->level = L;
        st->last_level = L - 1;
      }
      return;
    }
    // ---- collect level L + 1: take each queued node's word
    for (uint32_t k = tid; k < ncnt; k += kDistNarrowTPB) {
      const uint32_t v = qv[nx][k];
      const unsigned long long B = atomicExch(next + v, 0ull);
      qm[nx][k] = B;
      taken(v, B, L);
    }
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
        st->level = L;
        st->last_level = L;
      }
      return;
    }
  }
}

// ---- the hop search's kernels over the skeleton

__global__ void __launch_bounds__(256) k_dist_collect(unsigned long long* __restrict__ next, uint64_t n, uint32_t L,
                                                      uint32_t* __restrict__ queue,
                                                      unsigned long long* __restrict__ qmask, DistAcc acc,
                                                      DistState* st) {
  frontier_collect(next, n, L, queue, qmask, st,
                   [&](uint32_t v, unsigned long long B, uint32_t lv) { acc.node(v, B, lv); });
}

// entries [b, e) from b + first by step: the paths of m not yet seen at an entry's column are its
// discoveries — found(c, those bits)
template <class I, class F>
__device__ __forceinline__ void dist_relax_row(const I* __restrict__ indices, uint64_t n, uint64_t b, uint64_t e,
                                               uint32_t first, uint32_t step, unsigned long long m,
                                               unsigned long long* seen, DistState* st, F&& found) {
  for (uint64_t j = b + first; j < e; j += step) {
    const uint64_t c = (uint64_t)indices[j];
    if (c >= n) {
      st->bad = 1u;
      continue;
    }
    const unsigned long long nw = m & ~atomicOr(seen + c, m);
    if (nw) found(c, nw);
  }
}

template <class I>
__global__ void __launch_bounds__(256) k_dist_expand(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                     uint64_t n, uint64_t nnz, unsigned long long* __restrict__ seen,
                                                     unsigned long long* __restrict__ next,
                                                     const uint32_t* __restrict__ queue,
                                                     const unsigned long long* __restrict__ qmask,
                                                     uint32_t* __restrict__ long_rows, uint64_t long_cap, DistState* st) {
  const auto found = [&](uint64_t c, unsigned long long nw) { atomicOr(next + c, nw); };
  frontier_expand(indptr, n, nnz, queue, qmask, long_rows, long_cap, st,
                  [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m) {
                    dist_relax_row(indices, n, b, e, 0u, 1u, m, seen, st, found);
                  });
}

template <class I>
__global__ void __launch_bounds__(256) k_dist_expand_long(const I* __restrict__ indptr, const I* __restrict__ indices,
                                                          uint64_t n, uint64_t nnz,
                                                          unsigned long long* __restrict__ seen,
                                                          unsigned long long* __restrict__ next,
                                                          const uint32_t* __restrict__ queue,
                                                          const unsigned long long* __restrict__ qmask,
                                                          const uint32_t* __restrict__ long_rows, uint64_t long_cap,
                                                          DistState* st) {
  const auto found = [&](uint64_t c, unsigned long long nw) { atomicOr(next + c, nw); };
  frontier_expand_long(indptr, n, nnz, queue, qmask, long_rows, long_cap, st,
                       [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m) {
                         dist_relax_row(indices, n, b, e, threadIdx.x, 256u, m, seen, st, found);
                       });
}

template <class I>
__global__ void __launch_bounds__(kDistNarrowTPB) k_dist_narrow(const I* __restrict__ indptr,
                                                                const I* __restrict__ indices, uint64_t n, uint64_t nnz,
                                                                unsigned long long* __restrict__ seen,
                                                                unsigned long long* __restrict__ next,
                                                                uint32_t* __restrict__ queue,
                                                                unsigned long long* __restrict__ qmask, DistAcc acc,
                                                                DistState* st, uint32_t budget) {
  frontier_narrow(
      indptr, n, nnz, next, queue, qmask, st, budget,
      [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        dist_relax_row(indices, n, b, e, 0u, 1u, m, seen, st, push);
      },
      [&](uint64_t, uint64_t b, uint64_t e, unsigned long long m, auto& push) {
        dist_relax_row(indices, n, b, e, threadIdx.x, kDistNarrowTPB, m, seen, st, push);
      },
      [&](uint32_t v, unsigned long long B, uint32_t L) { acc.node(v, B, L); });
}

// keys [offs[i], offs[i + 1]) of blob: *flag = 1 when one ends in ":+" or ":-" (the reference's
// _warn_directed_bidirected reads node keys that way)
__global__ void __launch_bounds__(256) k_key_oriented(const uint8_t* __restrict__ blob,
                                                      const int64_t* __restrict__ offs, uint64_t n, uint32_t* flag) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t b = offs[i], e = offs[i + 1];
    if (b < 0 || e - b < 2) continue;
    const uint8_t s = blob[e - 1];
    if (blob[e - 2] == ':' && (s == '+' || s == '-')) *flag = 1u;
  }
}

}  // namespace g2n
