// g2n_seq.hip — which nodes carry a given sequence, straight from the S records of the staged input
// (g2n_seq_distance_from_path): what the reference's sequence_distance takes from a dict over every
// node's `sequence` attribute (gfa2network/analysis.py:96-108) after a graph build with
// store_seq=True (parser.py:135-163, builders.py:164-189).  No sequence byte is copied or brought
// to the host; the two node lists then go to g2n_csr_path_distances as K = 2.
//
// The sequence of an S record (fields cut at '\t', the line at '\n' only: a '\r' stays):
//   fewer than 3 fields: none.  third = fields[2]: when int(third) raises (CPython's int(bytes), the
//   grammar of pylit.h's py_int_literal) the sequence is third — b"" and b"*" included.  Otherwise
//   it is fields[3] when that exists and is not tag-shaped (first ':' at index 2, second at 4:
//   split(b":", 2) gives parts of lengths 2, 1, any), else none.
// The sequence of a node: that of the last S record of its name, in file order, that has one.
//
//   k_seq_lines     the only pass over every byte: 16-byte loads, the offsets of the line starts
//                   "S\t" appended to a list (one atomic per wave; the list's order is arbitrary,
//                   file order is the offsets').  Its capacity is the build's S-line count.
//   k_seq_classify  one lane per S line, work proportional to the name and the short fields: the
//                   name's node id from the key table over the names blob, the sequence field's
//                   start f, last[node] = max(offset + 1) over the records that have a sequence,
//                   and for each query (m bytes) a candidate when f + m is the input's end or a
//                   '\t' / '\n' and the first min(m, 16) bytes match.  A query holds no '\t' or
//                   '\n' (the host never launches for one that does), so all m bytes matching with
//                   a terminator behind them is exactly the field: its end is never searched for.
//   k_seq_compare   m > 16 only: one workgroup per candidate compares bytes [16, m).
//   k_seq_nodes     one lane per S line: a match counts when last[node] is its own line; the node
//                   ids are appended to the query's list (a node has one last line: no duplicates).
// Nothing outside [0, len) is addressed: the 16 bytes after len are never data nor a terminator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2n_keyset.hip"
#include "pylit.h"

namespace g2n {

constexpr uint32_t kSeqHead = 16;           // query bytes k_seq_classify compares itself
constexpr uint64_t kSeqNoQuery = ~0ull;     // a query that can match no field
constexpr uint32_t kSeqHas = 1u;            // flags: the record has a sequence
constexpr uint32_t kSeqCand = 2u;           // flags: << q, a candidate (after k_seq_compare: a match) of query q

struct SeqState {
  uint32_t n_lines;     // "S\t" line starts found (past the list's capacity: counted, not stored)
  uint32_t n_with_seq;  // records that have a sequence
  uint32_t cand[2];     // candidates of each query
  uint32_t hits[2];     // node ids appended for each query
  uint32_t bad;         // an S name that is no node
};

struct SeqQuery {
  uint64_t m[2];               // length, or kSeqNoQuery
  uint8_t head[2][kSeqHead];   // its first min(m, 16) bytes
};

// Appends of a wave's lanes with one atomic: the slot of this lane (pred) in the list *counter
// counts; every lane of the wave must call it.
__device__ inline uint32_t seq_wave_slot(bool pred, uint32_t* counter) {
  const unsigned long long b = __ballot(pred);
  if (b == 0) return 0;
  const int lane = (int)(threadIdx.x & 63u);
  const int leader = __ffsll((long long)b) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(b));
  base = (uint32_t)__shfl((int)base, leader, 64);
  return base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256) k_seq_lines(const uint8_t* __restrict__ in, uint64_t len, uint64_t cap,
                                                   uint64_t* __restrict__ lines, SeqState* st) {
  const uint64_t n_chunks = (len + 15) / 16;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  const int lane = (int)(threadIdx.x & 63u);
  // (a wave's lanes run the same trips: the shuffles need them all)
  for (uint64_t w0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); w0 < n_chunks; w0 += stride) {
    const uint64_t pos = (w0 + (uint64_t)lane) * 16;
    const uint4 v = pos < len ? load16(in, pos, len) : make_uint4(0, 0, 0, 0);
    uint32_t prev_b = (uint32_t)__shfl_up((int)(v.w >> 24), 1, 64);
    uint32_t next_b = (uint32_t)__shfl_down((int)(v.x & 0xFFu), 1, 64);
    if (lane == 0) prev_b = pos == 0 ? (uint32_t)'\n' : (uint32_t)in[pos - 1];
    if (lane == 63) next_b = pos + 16 < len ? (uint32_t)in[pos + 16] : 0u;
    const uint32_t valid = pos >= len ? 0u : (len - pos >= 16 ? 0xFFFFu : ((1u << (uint32_t)(len - pos)) - 1u));
    const uint32_t nl = mask16(v, 0x0A0A0A0Au) & valid;
    const uint32_t start = ((nl << 1) | (prev_b == '\n' ? 1u : 0u)) & valid;
    const uint32_t tab = mask16(v, 0x09090909u) & valid;  // (bytes past len load as 0: no tab)
    const uint32_t tab_next = (tab >> 1) | (next_b == '\t' ? 0x8000u : 0u);
    uint32_t hit = start & mask16(v, 0x53535353u) & tab_next;
    // slots: the lanes' counts scanned over the wave, one atomic for the total
    const uint32_t cnt = (uint32_t)__popc(hit);
    uint32_t incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    if (total == 0) continue;
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(&st->n_lines, total);
    base = (uint32_t)__shfl((int)base, 63, 64);
    uint64_t slot = (uint64_t)base + incl - cnt;
    while (hit) {
      const uint32_t b = (uint32_t)__builtin_ctz(hit);
      hit &= hit - 1;
      if (slot < cap) lines[slot] = pos + b;
      slot++;
    }
  }
}

// int(bytes) acceptance (pylit.h py_int_literal, transform off) of the field that starts at p, read
// up to its terminator: true with *end = the terminator's position ('\t', '\n' or len); false at
// the first byte outside the grammar — for a sequence, its first byte.
__device__ inline bool seq_int_field(const uint8_t* __restrict__ in, uint64_t p, uint64_t len, uint64_t* end) {
  enum { LEAD, SIGN, DIG, UND, TRAIL };
  int st = LEAD;
  uint32_t ndig = 0;
  for (; p < len; p++) {
    const int c = in[p];
    if (c == '\t' || c == '\n') break;
    switch (st) {
      case LEAD:
        if (py_isspace(c)) break;
        if (c == '+' || c == '-') { st = SIGN; break; }
        if (py_isdigit(c)) { st = DIG; ndig = 1; break; }
        return false;
      case SIGN:
      case UND:
        if (py_isdigit(c)) { st = DIG; ndig++; break; }
        return false;
      case DIG:
        if (py_isdigit(c)) { ndig++; break; }
        if (c == '_') { st = UND; break; }
        if (py_isspace(c)) { st = TRAIL; break; }
        return false;
      default:  // TRAIL
        if (py_isspace(c)) break;
        return false;
    }
    if (ndig > 4300) return false;  // sys.int_info.default_max_str_digits
  }
  *end = p;
  return st == DIG || st == TRAIL;
}

// parser.py:146-151: the field at g splits at ':' into parts of lengths 2, 1, any
__device__ inline bool seq_tag_shaped(const uint8_t* __restrict__ in, uint64_t g, uint64_t len) {
  for (uint32_t j = 0; j < 5; j++) {
    if (g + j >= len) return false;
    const uint8_t c = in[g + j];
    if (c == '\t' || c == '\n') return false;
    if ((c == ':') != (j == 2 || j == 4)) return false;
  }
  return true;
}

// the node id of the key in[a, a + n) in the table over the names blob, or ~0u
__device__ inline uint32_t seq_ks_find(const uint8_t* __restrict__ in, uint64_t a, uint64_t n,
                                       const KsEntry* __restrict__ table, uint64_t mask,
                                       const uint8_t* __restrict__ sblob) {
  if (n > kKsMaxKeyLen) return ~0u;
  const uint8_t* k = in + a;
  const uint64_t h = ks_hash(k, n);
  const uint32_t tag = (uint32_t)(h >> 32);
  for (uint64_t idx = h & mask;; idx = (idx + 1) & mask) {
    const KsEntry e = table[idx];
    if (e.hdr == kKsEmpty) return ~0u;
    if ((uint32_t)(e.hdr >> 32) == tag && (e.loc >> 40) == n) {
      const uint8_t* s = sblob + (e.loc & kKsOffMask);
      uint64_t j = 0;
      while (j < n && s[j] == k[j]) j++;
      if (j == n) return (uint32_t)e.hdr;
    }
  }
}

__global__ void __launch_bounds__(256) k_seq_classify(const uint8_t* __restrict__ in, uint64_t len,
                                                      const uint64_t* __restrict__ lines, uint64_t n_lines,
                                                      const KsEntry* __restrict__ table, uint64_t mask,
                                                      const uint8_t* __restrict__ names_blob, uint64_t n_nodes,
                                                      SeqQuery q, uint32_t* __restrict__ node_of,
                                                      uint64_t* __restrict__ fpos, uint32_t* __restrict__ flags,
                                                      unsigned long long* __restrict__ last,
                                                      uint32_t* __restrict__ cand0, uint32_t* __restrict__ cand1,
                                                      SeqState* st) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n_lines;  // (no early return: the appends need the whole wave)
  uint32_t fl = 0, node = ~0u;
  uint64_t f = 0;
  bool c[2] = {false, false};
  if (live) {
    const uint64_t p = lines[i];
    const uint64_t a = p + 2;  // in[p] = 'S', in[p + 1] = '\t', p + 1 < len
    uint64_t e = a;
    while (e < len && in[e] != '\t' && in[e] != '\n') e++;
    node = seq_ks_find(in, a, e - a, table, mask, names_blob);
    if (node >= n_nodes) {
      st->bad = 1u;
      node = ~0u;
    } else if (e < len && in[e] == '\t') {
      uint64_t end = 0;
      if (!seq_int_field(in, e + 1, len, &end)) {
        fl = kSeqHas;
        f = e + 1;
      } else if (end < len && in[end] == '\t' && !seq_tag_shaped(in, end + 1, len)) {
        fl = kSeqHas;
        f = end + 1;
      }
    }
    if (fl) {
      atomicMax(last + node, (unsigned long long)(p + 1));
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const uint64_t m = q.m[k];
        if (m == kSeqNoQuery || m > len - f) continue;
        if (f + m < len && in[f + m] != '\t' && in[f + m] != '\n') continue;
        const uint32_t h = m < kSeqHead ? (uint32_t)m : kSeqHead;
        uint32_t j = 0;
        while (j < h && in[f + j] == q.head[k][j]) j++;
        c[k] = j == h;
        if (c[k]) fl |= kSeqCand << k;
      }
    }
    node_of[i] = node;
    fpos[i] = f;
    flags[i] = fl;
  }
  const unsigned long long has = __ballot(fl != 0);
  if (has && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)has) - 1))
    atomicAdd(&st->n_with_seq, (uint32_t)__popcll(has));
  const uint32_t s0 = seq_wave_slot(c[0], &st->cand[0]);
  const uint32_t s1 = seq_wave_slot(c[1], &st->cand[1]);
  if (c[0] && q.m[0] > kSeqHead && s0 < n_lines) cand0[s0] = (uint32_t)i;
  if (c[1] && q.m[1] > kSeqHead && s1 < n_lines) cand1[s1] = (uint32_t)i;
}

// 16 bytes at any address
__device__ inline uint4 seq_load16u(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// Candidate j of one query (m > 16 bytes, at `query` on the device): bytes [16, m) of its field
// against the query's.  The input is read in aligned 16-byte chunks, the few bytes before the
// first and after the last one at a time; a mismatch takes the candidate's bit back.
__global__ void __launch_bounds__(256) k_seq_compare(const uint8_t* __restrict__ in, uint64_t len,
                                                     const uint8_t* __restrict__ query, uint64_t m, uint32_t bit,
                                                     const uint32_t* __restrict__ cand, uint64_t n_cand,
                                                     const uint64_t* __restrict__ fpos, uint32_t* __restrict__ flags) {
  for (uint64_t j = blockIdx.x; j < n_cand; j += gridDim.x) {
    const uint32_t line = cand[j];
    const uint64_t lo = fpos[line] + kSeqHead, hi = fpos[line] + m;  // hi <= len: checked when it became a candidate
    if (hi > len || lo > hi) continue;                               // (never: nothing outside the input is read)
    const uint64_t body = ((lo + 15) & ~15ull) < hi ? ((lo + 15) & ~15ull) : hi;
    const uint64_t n_chunks = (hi - body) / 16;
    const uint64_t tail = body + n_chunks * 16;
    const uint64_t t = threadIdx.x;
    bool ok = true;  // (the query byte of input position x: query[x - lo + 16])
    if (lo + t < body) ok = in[lo + t] == query[t + kSeqHead];
    if (tail + t < hi) ok = ok && in[tail + t] == query[tail + t - lo + kSeqHead];
    for (uint64_t k = t; k < n_chunks && ok; k += 256) {
      const uint64_t x = body + k * 16;
      const uint4 a = *(const uint4*)(in + x);
      const uint4 b = seq_load16u(query + (x - lo + kSeqHead));
      ok = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
    }
    if (!__syncthreads_and(ok) && threadIdx.x == 0) atomicAnd(flags + line, ~bit);
  }
}

__global__ void __launch_bounds__(256) k_seq_nodes(const uint64_t* __restrict__ lines, uint64_t n_lines,
                                                   const uint32_t* __restrict__ node_of,
                                                   const uint32_t* __restrict__ flags,
                                                   const unsigned long long* __restrict__ last,
                                                   uint32_t* __restrict__ ids0, uint32_t* __restrict__ ids1,
                                                   SeqState* st) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t fl = 0, node = 0;
  if (i < n_lines) {
    fl = flags[i];
    node = node_of[i];
    if (!(fl & kSeqHas) || last[node] != (unsigned long long)(lines[i] + 1)) fl = 0;  // last record wins
  }
  const bool h0 = (fl & kSeqCand) != 0, h1 = (fl & (kSeqCand << 1)) != 0;
  const uint32_t s0 = seq_wave_slot(h0, &st->hits[0]);
  const uint32_t s1 = seq_wave_slot(h1, &st->hits[1]);
  if (h0 && s0 < n_lines) ids0[s0] = node;
  if (h1 && s1 < n_lines) ids1[s1] = node;
}

// The keys of the listed nodes for the caller (sequence_nodes): their lengths, then — the host
// having summed them into offsets — their bytes, one lane per node (a key is short).
__global__ void __launch_bounds__(256) k_seq_hit_lens(const int64_t* __restrict__ ids, uint64_t n_ids, uint64_t n_nodes,
                                                      const int64_t* __restrict__ names_offsets,
                                                      int64_t* __restrict__ lens) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ids) return;
  const uint64_t id = (uint64_t)ids[i];
  lens[i] = id < n_nodes ? names_offsets[id + 1] - names_offsets[id] : 0;
}

__global__ void __launch_bounds__(256) k_seq_hit_names(const int64_t* __restrict__ ids, uint64_t n_ids,
                                                       uint64_t n_nodes, const int64_t* __restrict__ names_offsets,
                                                       const uint8_t* __restrict__ names_blob,
                                                       const int64_t* __restrict__ out_offs,
                                                       uint8_t* __restrict__ out_blob) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ids) return;
  const uint64_t id = (uint64_t)ids[i];
  if (id >= n_nodes) return;
  const uint8_t* src = names_blob + names_offsets[id];
  const int64_t n = names_offsets[id + 1] - names_offsets[id];
  if (n != out_offs[i + 1] - out_offs[i]) return;  // (never: the lengths were these)
  uint8_t* dst = out_blob + out_offs[i];
  for (int64_t j = 0; j < n; j++) dst[j] = src[j];
}

}  // namespace g2n
