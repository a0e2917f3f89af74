// g2n_graphjson.hip — export --format json (cli.py:282-306): json.dump(nx.node_link_data(G)) of the
// graph parse_gfa(build_graph=True, directed=True, bidirected=..., keep_directed_bidir=...) builds,
// rendered in HBM without building a graph object.  Included by g2n_pipeline.hip (same translation
// unit: the parse's field layout, the scans and the radix sort are used as they are).
//
// The document is {"directed": D, "multigraph": M, "graph": {}, "nodes": [...], "links": [...]} with
// json.dump's default separators and ensure_ascii.  The nodes are the build's node ids (first touch).
// An ENTRY is one add_edge call of the reference (builders.py:246-256): entry k of the stream-order COO
// of the same mode (one per L/E/C record; --bidirected alone: the record, then its reverse-complement
// twin).  NetworkX lists links in adjacency order:
//   * entries with the same (source, target) form a group (MultiGraph: the pair is unordered, its
//     source the endpoint with the smaller node id);
//   * groups are listed by (source id, stream position of the group's first entry);
//   * DiGraph: one link per group, carrying the orientation strings of the group's LAST entry;
//     MultiGraph / MultiDiGraph: one link per entry, "key" = the entry's rank in its group.
//
// G1  k_gj_keys            canonical (r, c) per entry, idx = stream position (the undirected build's COO
//                          holds every entry twice, (a, b) then (b, a), builders.py:222-228: the even ones)
// G2  sort_pairs_u32 x 2   stable LSD radix sort on c, then on r: entries ordered by (r, c, k)
// G3  k_gj_heads + scan    group heads; a member's group = the heads at or before it, its rank = its
//                          distance from the head; the group's first / last entry = its first / last member
// G4  k_gj_first_mark, scan, k_gj_first_compact
//                          the groups' first entries in stream order: (r, group)
// G5  sort_pairs_u32       ... stably sorted by r: the listing order (first entries keep stream order
//                          inside a source)
// G6  k_gj_counts + scan, k_gj_gbase
//                          links per group in listing order -> each group's base slot
// G7  k_gj_emit            every emitted entry to base + rank (DiGraph: the last member to base)
// No atomics: every position is a scan or sort result, so the bytes are the same on every run, and no
// step walks a row or a group (a 70 000-member group and a 70 000-target source are plain array ranges).
//
// T1  k_gj_name_esc        escaped length of every node name (gathered twice per link)
// T2  k_gj_node_len / k_gj_link_len  item lengths: nodes, then links, then the closing item; head and
//                          separators folded into the items; excl_scan<uint64_t> -> positions
// T3  k_gj_text            kGjItems consecutive items per block, assembled in LDS at their offset from the
//                          16-byte-aligned start of the block's range and written with aligned 16-byte
//                          stores (k_edge_text's scheme); a block whose text exceeds the stage writes its
//                          items straight to HBM.
// Plain mode needs each record's two orientation strings, which are not in the node names there:
// O1 (k_gj_line_count / k_gj_line_starts) lists the L/E/C lines' starts in stream order, O2 (k_gj_ori)
// re-runs the parse's own field layout (edge_layout) on each for the two spans in the staged input.
#pragma once

namespace g2n {

constexpr uint32_t kGjItems = 256;       // items per render block: one per thread (a DiGraph link of
                                         // 7-digit names is ~90 bytes: 256 of them fit the stage)
constexpr uint32_t kGjLds = 32 * 1024;   // the LDS stage
constexpr uint32_t kGjChunk = 16;        // input bytes per thread in the line scans

struct GjOri {  // a record's orientation spans in the staged input (an offset may carry kConstFlag)
  uint64_t uo, vo;
  uint32_t ul, vl;
};

// ------------------------------------------------------------------ O1: L/E/C line starts ----
// Bit k: byte p + k starts a line (parser.py:114: after a '\n', or byte 0).  b[0] = the byte before p
// ('\n' at p = 0), b[1..16] = bytes p .. p + 15, b[17] = byte p + 16; bytes at or past len read '\n'.
__device__ inline void gj_chunk(const uint8_t* __restrict__ in, uint64_t len, uint64_t p, uint8_t* b) {
  b[0] = p ? in[p - 1] : (uint8_t)'\n';
  if (p + kGjChunk <= len && ((uintptr_t)in & 15) == 0) {  // (p is a multiple of 16)
    const uint4 v = *(const uint4*)(in + p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < kGjChunk; k++) b[1 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kGjChunk; k++) b[1 + k] = p + k < len ? in[p + k] : (uint8_t)'\n';
  }
  b[1 + kGjChunk] = p + kGjChunk < len ? in[p + kGjChunk] : (uint8_t)'\n';
}

// the L / E / C records among them (parser.py:117-134: the first field is exactly the type byte)
__device__ inline uint32_t gj_edge_mask(const uint8_t* __restrict__ in, uint64_t len, uint64_t p) {
  if (p >= len) return 0;
  uint8_t b[kGjChunk + 2];
  gj_chunk(in, len, p, b);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kGjChunk; k++) {
    const uint8_t t = b[1 + k], nx = b[2 + k];
    const bool rec = b[k] == '\n' && p + k < len && (t == 'L' || t == 'E' || t == 'C') && (nx == '\t' || nx == '\n');
    m |= rec ? 1u << k : 0u;
  }
  return m;
}

__global__ void __launch_bounds__(kTPB) k_gj_line_count(const uint8_t* __restrict__ in, uint64_t len,
                                                        uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t red[kTPB / 64];
  const uint64_t p = ((uint64_t)blockIdx.x * kTPB + threadIdx.x) * kGjChunk;
  uint32_t ex;
  const uint32_t tot = block_excl_scan_u32((uint32_t)__popc(gj_edge_mask(in, len, p)), &ex, red);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kTPB) k_gj_line_starts(const uint8_t* __restrict__ in, uint64_t len,
                                                         const uint32_t* __restrict__ boff, uint64_t n_edges,
                                                         uint64_t* __restrict__ starts) {
  __shared__ uint32_t red[kTPB / 64];
  const uint64_t p = ((uint64_t)blockIdx.x * kTPB + threadIdx.x) * kGjChunk;
  uint32_t m = gj_edge_mask(in, len, p);
  uint32_t ex;
  (void)block_excl_scan_u32((uint32_t)__popc(m), &ex, red);
  uint64_t q = (uint64_t)boff[blockIdx.x] + ex;
  for (; m; m &= m - 1, q++)
    if (q < n_edges) starts[q] = p + (uint32_t)__builtin_ctz(m);  // (n_edges = the count: the bound is a guard)
}

// the first line whose first byte is none of SLPECOHF (parser.py:117-131: the one-shot warning's line)
__global__ void __launch_bounds__(kTPB) k_gj_first_unknown(const uint8_t* __restrict__ in, uint64_t len,
                                                           unsigned long long* first) {
  const uint64_t p = ((uint64_t)blockIdx.x * kTPB + threadIdx.x) * kGjChunk;
  unsigned long long best = ~0ull;
  if (p < len) {
    uint8_t b[kGjChunk + 2];
    gj_chunk(in, len, p, b);
    for (uint32_t k = kGjChunk; k-- > 0;) {
      const uint8_t t = b[1 + k];
      const bool known = t == 'S' || t == 'L' || t == 'P' || t == 'E' || t == 'C' || t == 'O' || t == 'H' || t == 'F';
      if (b[k] == '\n' && p + k < len && !known) best = p + k;
    }
  }
  best = wave_reduce_min(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(first, best);  // (an integer minimum: order-free)
}

// ------------------------------------------------------------------ O2: orientation spans ----
__global__ void __launch_bounds__(64) k_gj_ori(const uint8_t* __restrict__ in_, uint64_t len,
                                               const uint64_t* __restrict__ starts, uint64_t n_edges,
                                               GjOri* __restrict__ ori, unsigned int* bad) {
  const uint64_t e = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= n_edges) return;
  const Src in{in_, 0, len};
  const uint64_t s = starts[e];
  const EdgeLayout L = edge_layout(in, s, next_nl(in, s, len));
  GjOri o{kConstFlag | '+', kConstFlag | '+', 1, 1};
  if (L.err) *bad = 1u;  // (a clean build has none: the driver refuses the result)
  else o = GjOri{L.ouo, L.ovo, L.oul, L.ovl};
  ori[e] = o;
}

// ------------------------------------------------------------------ JSON string escapes ----
// json.dumps(s) with ensure_ascii (json/encoder.py ESCAPE_ASCII): '"' and '\\' behind a backslash, \n \r
// \t \b \f, every other character outside ' '..'~' as \uXXXX (lower-case hex; above U+FFFF a surrogate
// pair).  kW: write at d (else count only); returns the escaped length.  utf8: s is valid UTF-8 (the parse
// decoded it) and is read as code points; else every byte is one character.  Reads s[0, n) only.
template <bool kW>
__device__ inline uint64_t gj_hex4(uint8_t* d, uint64_t o, uint32_t v) {
  if (kW) {
    d[o] = '\\';
    d[o + 1] = 'u';
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t h = (v >> (12 - 4 * k)) & 15u;
      d[o + 2 + k] = (uint8_t)(h < 10 ? '0' + h : 'a' + (h - 10));
    }
  }
  return o + 6;
}

template <bool kW>
__device__ inline uint64_t gj_esc(uint8_t* d, const uint8_t* __restrict__ s, uint64_t n, bool utf8) {
  uint64_t o = 0;
  for (uint64_t i = 0; i < n;) {
    const uint32_t c = s[i++];
    if (c >= 0x20 && c < 0x7F && c != '"' && c != '\\') {
      if (kW) d[o] = (uint8_t)c;
      o++;
      continue;
    }
    if (utf8 && c >= 0xC0) {
      uint32_t k = c >= 0xF0 ? 3 : c >= 0xE0 ? 2 : 1;  // continuation bytes
      uint32_t cp = c & (0x3Fu >> k);
      for (; k && i < n; k--) cp = (cp << 6) | (s[i++] & 0x3Fu);
      if (cp > 0xFFFF) {
        cp -= 0x10000;
        o = gj_hex4<kW>(d, o, 0xD800u | ((cp >> 10) & 0x3FFu));
        o = gj_hex4<kW>(d, o, 0xDC00u | (cp & 0x3FFu));
      } else {
        o = gj_hex4<kW>(d, o, cp);
      }
      continue;
    }
    uint8_t two = 0;
    switch (c) {
      case '"': two = '"'; break;
      case '\\': two = '\\'; break;
      case '\n': two = 'n'; break;
      case '\r': two = 'r'; break;
      case '\t': two = 't'; break;
      case '\b': two = 'b'; break;
      case '\f': two = 'f'; break;
      default: break;
    }
    if (two) {
      if (kW) {
        d[o] = '\\';
        d[o + 1] = two;
      }
      o += 2;
    } else {
      o = gj_hex4<kW>(d, o, c);
    }
  }
  return o;
}

// an orientation span (k_gj_ori): the constant byte '+' / '-' or bytes of the staged input
template <bool kW>
__device__ inline uint64_t gj_esc_ori(uint8_t* d, const uint8_t* __restrict__ in, uint64_t len, uint64_t off,
                                      uint32_t n) {
  if (off & kConstFlag) {
    if (kW) d[0] = (uint8_t)(off & 0xFF);
    return 1;
  }
  if (off > len || n > len - off) return 0;  // (never: the spans come from lines inside [0, len))
  return gj_esc<kW>(d, in + off, n, true);
}

template <size_t K>
__device__ inline uint8_t* gj_lit(uint8_t* d, const char (&s)[K]) {
#pragma unroll
  for (size_t k = 0; k + 1 < K; k++) d[k] = (uint8_t)s[k];
  return d + (K - 1);
}
#define GJ_LEN(s) ((uint64_t)(sizeof(s) - 1))
#define GJ_SEP ", "
#define GJ_MID "], \"links\": ["
#define GJ_TAIL "]}"
#define GJ_NODE_A "{\"id\": \""
#define GJ_NODE_B "\"}"
#define GJ_DI_A "{\"orientation_from\": \""
#define GJ_DI_B "\", \"orientation_to\": \""
#define GJ_DI_C "\", \"source\": \""
#define GJ_MU_A "{\"source\": \""
#define GJ_TGT "\", \"target\": \""
#define GJ_DI_E "\"}"
#define GJ_MU_K "\", \"key\": "
#define GJ_MU_E "}"

__device__ inline uint32_t gj_ndig(uint32_t v) {
  uint32_t n = 1;
  for (uint32_t p = 10; n < 10 && v >= p; p *= 10) n++;  // (10^10 overflows: ten digits at most)
  return n;
}

// ------------------------------------------------------------------ G1-G7: group and order ----
__global__ void __launch_bounds__(kTPB) k_gj_keys(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                  uint64_t m, uint32_t step, int unordered,
                                                  uint32_t* __restrict__ cr, uint32_t* __restrict__ cc,
                                                  uint32_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i >= m) return;
  const uint32_t r = (uint32_t)rows[i * step], c = (uint32_t)cols[i * step];  // entry i is COO triplet i * step
  const bool swap = unordered && c < r;
  cr[i] = swap ? c : r;
  cc[i] = swap ? r : c;
  idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kTPB) k_gj_gather(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx,
                                                    uint64_t m, uint32_t* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (j < m) out[j] = src[idx[j]];
}

// head[j] = 1 when sorted entry j opens a group (m + 1 flags, the last 0)
__global__ void __launch_bounds__(kTPB) k_gj_heads(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ cc,
                                                   const uint32_t* __restrict__ perm, uint64_t m,
                                                   uint32_t* __restrict__ head) {
  const uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (j > m) return;
  uint32_t h = 0;
  if (j < m) h = j == 0 || rs[j] != rs[j - 1] || cc[perm[j]] != cc[perm[j - 1]];
  head[j] = h;
}

// hs[g] = the sorted position of group g's head (hs[G] = m); the stream entry that is the group's first
// member is marked and told its group (m + 1 flags, zeroed before, the last stays 0)
__global__ void __launch_bounds__(kTPB) k_gj_first_mark(const uint32_t* __restrict__ head,
                                                        const uint32_t* __restrict__ hx,
                                                        const uint32_t* __restrict__ perm, uint64_t m,
                                                        uint32_t* __restrict__ hs, uint32_t* __restrict__ fflag,
                                                        uint32_t* __restrict__ fgroup) {
  const uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (j > m) return;
  if (j == m) {
    hs[hx[m]] = (uint32_t)m;
    return;
  }
  if (!head[j]) return;
  const uint32_t g = hx[j], k = perm[j];
  hs[g] = (uint32_t)j;
  fflag[k] = 1u;
  fgroup[k] = g;
}

__global__ void __launch_bounds__(kTPB) k_gj_first_compact(const uint32_t* __restrict__ fflag,
                                                           const uint32_t* __restrict__ fx,
                                                           const uint32_t* __restrict__ fgroup,
                                                           const uint32_t* __restrict__ cr, uint64_t m,
                                                           uint32_t* __restrict__ lr, uint32_t* __restrict__ lg) {
  const uint64_t k = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (k >= m || !fflag[k]) return;
  const uint32_t q = fx[k];
  lr[q] = cr[k];
  lg[q] = fgroup[k];
}

// links of the group at listing position p (G + 1 counts, the last 0)
__global__ void __launch_bounds__(kTPB) k_gj_counts(const uint32_t* __restrict__ order, const uint32_t* __restrict__ hs,
                                                    uint64_t G, int multi, uint32_t* __restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (p > G) return;
  uint32_t n = 0;
  if (p < G) {
    const uint32_t g = order[p];
    n = multi ? hs[g + 1] - hs[g] : 1u;
  }
  cnt[p] = n;
}

__global__ void __launch_bounds__(kTPB) k_gj_gbase(const uint32_t* __restrict__ order, const uint32_t* __restrict__ base,
                                                   uint64_t G, uint32_t* __restrict__ gbase) {
  const uint64_t p = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (p < G) gbase[order[p]] = base[p];
}

// link slot <- (source, target, x): x = the key (multi) or the record of the group's last entry (DiGraph)
__global__ void __launch_bounds__(kTPB) k_gj_emit(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ cc,
                                                  const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head,
                                                  const uint32_t* __restrict__ hx, const uint32_t* __restrict__ hs,
                                                  const uint32_t* __restrict__ gbase, uint64_t m, uint64_t n_links,
                                                  int multi, uint32_t* __restrict__ ls, uint32_t* __restrict__ lt,
                                                  uint32_t* __restrict__ lx) {
  const uint64_t j = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (j >= m) return;
  const uint32_t g = hx[j] + head[j] - 1u;  // heads at or before j, minus one
  const uint32_t t = (uint32_t)j - hs[g];
  if (!multi && (uint32_t)j + 1u != hs[g + 1]) return;  // DiGraph: the last member speaks for the group
  const uint64_t slot = (uint64_t)gbase[g] + (multi ? t : 0u);
  if (slot >= n_links) return;  // (never: the bases are the scan of the same counts)
  const uint32_t k = perm[j];
  ls[slot] = rs[j];
  lt[slot] = cc[k];
  lx[slot] = multi ? t : k;
}

// ------------------------------------------------------------------ T1-T3: the text ----
__global__ void __launch_bounds__(kTPB) k_gj_name_esc(const uint8_t* __restrict__ blob, const int64_t* __restrict__ offs,
                                                      uint64_t n, uint64_t* __restrict__ nesc) {
  const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  const int64_t o = offs[i];
  nesc[i] = gj_esc<false>(nullptr, blob + o, (uint64_t)(offs[i + 1] - o), false);
}

// item i < n: node i, behind the head (i = 0) or a separator
__global__ void __launch_bounds__(kTPB) k_gj_node_len(const uint64_t* __restrict__ nesc, uint64_t n, uint64_t head_len,
                                                      uint64_t* __restrict__ ilen) {
  const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  ilen[i] = (i ? GJ_LEN(GJ_SEP) : head_len) + GJ_LEN(GJ_NODE_A) + nesc[i] + GJ_LEN(GJ_NODE_B);
}

// item n + l, l < n_links: link l behind "], "links": [" (l = 0) or a separator; item n + n_links closes
// the document (and opens the links of a graph that has none); one more entry, 0, ends the scan
__global__ void __launch_bounds__(kTPB) k_gj_link_len(const uint32_t* __restrict__ ls, const uint32_t* __restrict__ lt,
                                                      const uint32_t* __restrict__ lx, uint64_t n_links, int multi,
                                                      const uint64_t* __restrict__ nesc, const GjOri* __restrict__ ori,
                                                      const uint8_t* __restrict__ in, uint64_t len,
                                                      uint64_t* __restrict__ ilen /* at item n */) {
  const uint64_t l = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (l > n_links + 1) return;
  if (l == n_links + 1) {
    ilen[l] = 0;
    return;
  }
  if (l == n_links) {
    ilen[l] = (n_links ? 0 : GJ_LEN(GJ_MID)) + GJ_LEN(GJ_TAIL);
    return;
  }
  uint64_t b = (l ? GJ_LEN(GJ_SEP) : GJ_LEN(GJ_MID)) + nesc[ls[l]] + nesc[lt[l]];
  if (multi) {
    b += GJ_LEN(GJ_MU_A) + GJ_LEN(GJ_TGT) + GJ_LEN(GJ_MU_K) + gj_ndig(lx[l]) + GJ_LEN(GJ_MU_E);
  } else {
    const GjOri o = ori[lx[l]];
    b += GJ_LEN(GJ_DI_A) + GJ_LEN(GJ_DI_B) + GJ_LEN(GJ_DI_C) + GJ_LEN(GJ_TGT) + GJ_LEN(GJ_DI_E) +
         gj_esc_ori<false>(nullptr, in, len, o.uo, o.ul) + gj_esc_ori<false>(nullptr, in, len, o.vo, o.vl);
  }
  ilen[l] = b;
}

struct GjText {
  uint64_t n, n_links;         // items: n nodes, n_links links, the closing item
  int multi;
  const uint8_t* head;         // {"directed": D, "multigraph": M, "graph": {}, "nodes": [
  uint32_t head_len;
  const uint8_t* blob;         // node names
  const int64_t* offs;
  const uint64_t* nesc;
  const uint32_t *ls, *lt, *lx;
  const GjOri* ori;            // plain mode
  const uint8_t* in;           // the staged input (orientation spans)
  uint64_t len;
  const uint64_t* pos;         // n + n_links + 2 positions
};

__device__ inline uint8_t* gj_name(uint8_t* d, const GjText& T, uint32_t id) {
  const int64_t o = T.offs[id];
  const uint64_t nl = (uint64_t)(T.offs[id + 1] - o);
  if (T.nesc[id] == nl) {  // nothing to escape
    for (uint64_t k = 0; k < nl; k++) d[k] = T.blob[o + k];
    return d + nl;
  }
  return d + gj_esc<true>(d, T.blob + o, nl, false);
}

__device__ inline void gj_item(uint8_t* d, const GjText& T, uint64_t e) {
  if (e < T.n) {
    if (e) {
      d = gj_lit(d, GJ_SEP);
    } else {
      for (uint32_t k = 0; k < T.head_len; k++) d[k] = T.head[k];
      d += T.head_len;
    }
    d = gj_lit(d, GJ_NODE_A);
    d = gj_name(d, T, (uint32_t)e);
    gj_lit(d, GJ_NODE_B);
    return;
  }
  const uint64_t l = e - T.n;
  if (l == T.n_links) {
    if (!T.n_links) d = gj_lit(d, GJ_MID);
    gj_lit(d, GJ_TAIL);
    return;
  }
  d = l ? gj_lit(d, GJ_SEP) : gj_lit(d, GJ_MID);
  const uint32_t s = T.ls[l], t = T.lt[l], x = T.lx[l];
  if (T.multi) {
    d = gj_lit(d, GJ_MU_A);
    d = gj_name(d, T, s);
    d = gj_lit(d, GJ_TGT);
    d = gj_name(d, T, t);
    d = gj_lit(d, GJ_MU_K);
    const uint32_t nd = gj_ndig(x);
    uint32_t v = x;
    for (uint32_t k = nd; k-- > 0; v /= 10u) d[k] = (uint8_t)('0' + v % 10u);
    d += nd;
    gj_lit(d, GJ_MU_E);
  } else {
    const GjOri o = T.ori[x];
    d = gj_lit(d, GJ_DI_A);
    d += gj_esc_ori<true>(d, T.in, T.len, o.uo, o.ul);
    d = gj_lit(d, GJ_DI_B);
    d += gj_esc_ori<true>(d, T.in, T.len, o.vo, o.vl);
    d = gj_lit(d, GJ_DI_C);
    d = gj_name(d, T, s);
    d = gj_lit(d, GJ_TGT);
    d = gj_name(d, T, t);
    gj_lit(d, GJ_DI_E);
  }
}

__global__ void __launch_bounds__(kTPB) k_gj_text(GjText T, uint8_t* __restrict__ out) {
  static_assert(kGjItems == (uint32_t)kTPB, "one item per thread");
  __shared__ uint4 stage4[kGjLds / 16];
  uint8_t* stage = (uint8_t*)stage4;
  const uint64_t n_items = T.n + T.n_links + 1;
  const uint64_t e0 = (uint64_t)blockIdx.x * kGjItems;
  const uint64_t e1 = e0 + kGjItems < n_items ? e0 + kGjItems : n_items;
  const uint64_t p0 = T.pos[e0], p1 = T.pos[e1];  // pos holds n_items + 1 entries
  const uint64_t base = p0 & ~15ull;
  const bool staged = p1 - base <= kGjLds;  // block-uniform
  const uint64_t e = e0 + threadIdx.x;
  if (e < e1) {
    const uint64_t pe = T.pos[e];
    gj_item(staged ? stage + (pe - base) : out + pe, T, e);
  }
  if (!staged) return;
  __syncthreads();
  const uint64_t w0 = base >> 4, w1 = (p1 + 15) >> 4;
  for (uint64_t w = w0 + threadIdx.x; w < w1; w += kTPB) {
    const uint64_t a = w << 4;
    if (a >= p0 && a + 16 <= p1) {
      *(uint4*)(out + a) = stage4[w - w0];
    } else {
      for (uint64_t b = a < p0 ? p0 : a; b < a + 16 && b < p1; b++) out[b] = stage[b - base];
    }
  }
}

// ------------------------------------------------------------------ the driver ----
// The lowest node id whose key has a byte >= 0x80 (the graph path decodes node keys as ASCII,
// builders.py:155-162), -1: none.
static int64_t gj_high_key(g2n_context* c, const g2n_result* R) {
  if (!R->names_blob || !R->names_bytes || !R->n_nodes) return -1;
  auto* so = dget<StatsOut>(c, S_STOUT, 1);
  G2N_HIP(hipMemsetAsync(so, 0, sizeof(StatsOut), c->stream));
  G2N_HIP(hipMemsetAsync(&so->high_off, 0xFF, sizeof(so->high_off), c->stream));
  const unsigned g = (unsigned)std::min<uint64_t>(grid_for((R->names_bytes + 15) / 16, 256), (uint64_t)c->n_cu * 8);
  hipLaunchKernelGGL(k_high_byte, dim3(g), dim3(256), 0, c->stream, R->names_blob, (uint64_t)R->names_bytes, so);
  hipLaunchKernelGGL(k_high_owner, dim3(1), dim3(64), 0, c->stream, R->names_offsets, (uint64_t)R->n_nodes, so);
  const StatsOut h = read_dev(c, so);
  if (h.high_off == ~0ull) return -1;
  if (h.high_id < 0 || h.high_id >= R->n_nodes) throw Failure(G2N_E_DEVICE, "node keys: key lookup failed");
  return h.high_id;
}

// The build of the JSON export's graph: the stream-order COO (one entry per add_edge call) and the names,
// with the failure the reference's build raises first in the stream.  ascii (keys are decoded: not
// --raw-bytes-id): a key with a byte >= 0x80 is G2N_E_UNICODE, err_line -1, err_index = the node id,
// err_detail = the key — also when a later line is malformed (the input before that line is built again
// to see), and the one-shot warning counts only when its line precedes the key's first touch.
static int gj_build(g2n_context* c, const uint8_t* in, uint64_t len, const g2n_options* o, g2n_result* R, bool ascii) {
  g2n_options b = *o;
  b.directed = 1;
  b.asymmetric = 1;
  b.strip_orientation = 0;
  b.weight_tag = nullptr;
  b.dtype = G2N_BOOL;
  b.output = G2N_OUT_COO;
  b.want_node_names = 1;
  b.range_flags = G2N_RANGE_NO_VALUES;  // the order and the text read ids only
  if (!b.bidirected) b.keep_directed_bidir = 0;
  const int rc = run_build(c, in, len, &b, R);
  if (!ascii) return rc;
  if (rc >= G2N_E_MALFORMED_L && rc <= G2N_E_INT_TOO_LARGE && R->err_line >= 0) {
    const g2n_result first = *R;  // (its err_detail points into the input)
    const uint64_t off = c->err_line_off;
    g2n_result P;
    if (off && gj_build(c, in, off, o, &P, true) == G2N_E_UNICODE && P.err_line < 0) {
      P.n_lines = first.n_lines;
      P.n_records = first.n_records;
      *R = P;
      return R->status;
    }
    *R = first;
    return rc;
  }
  if (rc != G2N_OK) return rc;
  const int64_t bad = gj_high_key(c, R);
  if (bad < 0) return G2N_OK;
  int64_t span[2];
  G2N_HIP(hipMemcpyAsync(span, R->names_offsets + bad, sizeof(span), hipMemcpyDeviceToHost, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  auto* key = dget<uint8_t>(c, S_GJKEY, (uint64_t)(span[1] - span[0]));  // (the names blob does not outlive the next build)
  G2N_HIP(hipMemcpyAsync(key, R->names_blob + span[0], (size_t)(span[1] - span[0]), hipMemcpyDeviceToDevice, c->stream));
  G2N_HIP(hipStreamSynchronize(c->stream));
  g2n_result E = *R;
  if (E.has_warning) {  // does the unsupported record come before the key's first touch?
    auto* first = dget<unsigned long long>(c, S_EFIRST, 1);
    G2N_HIP(hipMemsetAsync(first, 0xFF, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_gj_first_unknown, dim3(grid_for((len + kGjChunk - 1) / kGjChunk)), dim3(kTPB), 0, c->stream, in,
                       len, first);
    const unsigned long long w = read_dev(c, first);
    g2n_result P;
    if (w != ~0ull && w > 0 && w <= len && run_build(c, in, w, &b, &P) == G2N_OK && gj_high_key(c, &P) >= 0)
      E.has_warning = 0;
  }
  *R = E;
  R->status = G2N_E_UNICODE;
  R->err_line = -1;
  R->err_index = bad;
  R->err_detail = key;
  R->err_detail_len = span[1] - span[0];
  R->rows = R->cols = R->data = nullptr;
  R->nnz = 0;
  R->names_blob = nullptr;
  R->names_offsets = nullptr;
  R->names_bytes = 0;
  set_last_error("a node key is not ASCII (the graph path decodes node keys as ASCII)");
  return R->status;
}

// O1, O2: the orientation spans of the m L/E/C records, in stream order
static const GjOri* gj_spans(g2n_context* c, const uint8_t* in, uint64_t len, uint64_t m) {
  const uint64_t nb = grid_for((len + kGjChunk - 1) / kGjChunk);
  auto* bcnt = dget<uint32_t>(c, S_GJBCNT, nb + 1);
  auto* boff = dget<uint32_t>(c, S_GJBOFF, nb + 1);
  hipLaunchKernelGGL(k_gj_line_count, dim3((unsigned)nb), dim3(kTPB), 0, c->stream, in, len, bcnt);
  G2N_HIP(hipMemsetAsync(bcnt + nb, 0, sizeof(uint32_t), c->stream));
  scan_excl<uint32_t, uint32_t>(c, bcnt, boff, nb + 1);
  if ((uint64_t)read_dev(c, boff + nb) != m) throw Failure(G2N_E_DEVICE, "graph JSON: L/E/C lines differ from the build's entries");
  auto* starts = dget<uint64_t>(c, S_GJSTART, m);
  auto* spans = dget<GjOri>(c, S_GJORI, m);
  auto* badf = dget<unsigned int>(c, S_ZBAD, 1);
  G2N_HIP(hipMemsetAsync(badf, 0, sizeof(unsigned int), c->stream));
  hipLaunchKernelGGL(k_gj_line_starts, dim3((unsigned)nb), dim3(kTPB), 0, c->stream, in, len, (const uint32_t*)boff, m,
                     starts);
  hipLaunchKernelGGL(k_gj_ori, dim3(grid_for(m, 64)), dim3(64), 0, c->stream, in, len, (const uint64_t*)starts, m, spans,
                     badf);
  if (read_dev(c, badf)) throw Failure(G2N_E_DEVICE, "graph JSON: a record of a clean build did not parse again");
  return spans;
}

// G1-G7: the links in listing order (ls, lt: source and target ids; lx: the key (multi) or the record of the
// group's last entry).  Entry i is COO triplet i * step; unordered: the pair's source is its smaller id.
struct GjLinks {
  uint64_t n_links = 0;
  uint32_t *ls = nullptr, *lt = nullptr, *lx = nullptr;
};

static GjLinks gj_links(g2n_context* c, const int32_t* rows, const int32_t* cols, uint64_t m, uint32_t step,
                        bool unordered, bool multi, uint64_t n) {
  GjLinks K;
  if (!m) return K;
  const int bits = bits_for(n);
  auto* cr = dget<uint32_t>(c, S_GJCR, m);
  auto* cc = dget<uint32_t>(c, S_GJCC, m);
  auto* idx = dget<uint32_t>(c, S_GJIDX, m);
  auto* k1 = dget<uint32_t>(c, S_GJK1, m);    // c sorted; later the sources in stream order of the first entries
  auto* idx1 = dget<uint32_t>(c, S_GJIDX1, m);
  auto* k2 = dget<uint32_t>(c, S_GJK2, m);    // r in c order; later the groups beside k1
  auto* rs = dget<uint32_t>(c, S_GJRS, m);
  auto* perm = dget<uint32_t>(c, S_GJPERM, m);
  auto* head = dget<uint32_t>(c, S_GJHEAD, m + 1);
  auto* hx = dget<uint32_t>(c, S_GJHX, m + 1);
  auto* hs = dget<uint32_t>(c, S_GJHS, m + 1);
  auto* fflag = dget<uint32_t>(c, S_GJFFLAG, m + 1);
  auto* fx = dget<uint32_t>(c, S_GJFX, m + 1);
  auto* fgroup = dget<uint32_t>(c, S_GJFGRP, m);
  hipLaunchKernelGGL(k_gj_keys, dim3(grid_for(m)), dim3(kTPB), 0, c->stream, rows, cols, m, step, (int)unordered,
                     cr, cc, idx);
  sort_pairs_u32<uint32_t>(c, cc, k1, idx, idx1, m, bits);
  hipLaunchKernelGGL(k_gj_gather, dim3(grid_for(m)), dim3(kTPB), 0, c->stream, (const uint32_t*)cr,
                     (const uint32_t*)idx1, m, k2);
  sort_pairs_u32<uint32_t>(c, k2, rs, idx1, perm, m, bits);
  hipLaunchKernelGGL(k_gj_heads, dim3(grid_for(m + 1)), dim3(kTPB), 0, c->stream, (const uint32_t*)rs,
                     (const uint32_t*)cc, (const uint32_t*)perm, m, head);
  scan_excl<uint32_t, uint32_t>(c, head, hx, m + 1);
  const uint64_t G = read_dev(c, hx + m);
  G2N_HIP(hipMemsetAsync(fflag, 0, (m + 1) * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_gj_first_mark, dim3(grid_for(m + 1)), dim3(kTPB), 0, c->stream, (const uint32_t*)head,
                     (const uint32_t*)hx, (const uint32_t*)perm, m, hs, fflag, fgroup);
  scan_excl<uint32_t, uint32_t>(c, fflag, fx, m + 1);
  uint32_t *lr = k1, *lg = k2;  // (both sorts are done with them)
  hipLaunchKernelGGL(k_gj_first_compact, dim3(grid_for(m)), dim3(kTPB), 0, c->stream, (const uint32_t*)fflag,
                     (const uint32_t*)fx, (const uint32_t*)fgroup, (const uint32_t*)cr, m, lr, lg);
  auto* lrs = dget<uint32_t>(c, S_GJLRS, G);
  auto* order = dget<uint32_t>(c, S_GJORDER, G);
  sort_pairs_u32<uint32_t>(c, lr, lrs, lg, order, G, bits);
  auto* cnt = dget<uint32_t>(c, S_GJCNT, G + 1);
  auto* base = dget<uint32_t>(c, S_GJBASE, G + 1);
  auto* gbase = dget<uint32_t>(c, S_GJGBASE, G);
  hipLaunchKernelGGL(k_gj_counts, dim3(grid_for(G + 1)), dim3(kTPB), 0, c->stream, (const uint32_t*)order,
                     (const uint32_t*)hs, G, (int)multi, cnt);
  scan_excl<uint32_t, uint32_t>(c, cnt, base, G + 1);
  hipLaunchKernelGGL(k_gj_gbase, dim3(grid_for(G)), dim3(kTPB), 0, c->stream, (const uint32_t*)order,
                     (const uint32_t*)base, G, gbase);
  K.n_links = multi ? m : G;
  K.ls = dget<uint32_t>(c, S_GJLS, K.n_links);
  K.lt = dget<uint32_t>(c, S_GJLT, K.n_links);
  K.lx = dget<uint32_t>(c, S_GJLX, K.n_links);
  hipLaunchKernelGGL(k_gj_emit, dim3(grid_for(m)), dim3(kTPB), 0, c->stream, (const uint32_t*)rs, (const uint32_t*)cc,
                     (const uint32_t*)perm, (const uint32_t*)head, (const uint32_t*)hx, (const uint32_t*)hs,
                     (const uint32_t*)gbase, m, K.n_links, (int)multi, K.ls, K.lt, K.lx);
  return K;
}

// G2N_OUT_GRAPH_JSON.  Result: format G2N_FMT_TEXT, data = the document, nnz = its bytes.
static int run_graph_json(g2n_context* c, const uint8_t* in, uint64_t len, const g2n_options* o, g2n_result* R) {
  const bool keys_str = o->want_node_names != 0;
  const int rc = gj_build(c, in, len, o, R, keys_str);
  if (rc != G2N_OK) return rc;
  const bool multi = o->bidirected != 0;
  const bool directed = !multi || o->keep_directed_bidir != 0;
  // the MultiGraph's matrix is undirected: its COO carries (a, b), (b, a) per add_edge call (builders.py:222-228)
  const uint32_t step = multi && !directed ? 2u : 1u;
  const uint64_t m = (uint64_t)R->nnz / step, n = (uint64_t)R->n_nodes;
  const auto* rows = (const int32_t*)R->rows;
  const auto* cols = (const int32_t*)R->cols;
  const int64_t* offs = R->names_offsets;
  const uint8_t* blob = R->names_blob;
  R->format = G2N_FMT_TEXT;
  R->rows = R->cols = R->data = nullptr;
  R->nnz = 0;
  R->names_blob = nullptr;  // the names are in the text
  R->names_offsets = nullptr;
  R->names_bytes = 0;
  const std::string head_str = std::string("{\"directed\": ") + (directed ? "true" : "false") + ", \"multigraph\": " +
                           (multi ? "true" : "false") + ", \"graph\": {}, \"nodes\": [";
  if (!keys_str && n) {  // bytes keys are not JSON serializable: the reference stops at the first node
    finish_timings(c, R);
    return G2N_OK;
  }
  if (n == 0) {  // no records: the constant document
    const std::string doc = head_str + GJ_MID + GJ_TAIL;
    auto* text = dget<uint8_t>(c, S_ETEXT, doc.size() + 16);
    G2N_HIP(hipMemcpyAsync(text, doc.data(), doc.size(), hipMemcpyHostToDevice, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
    R->data = text;
    R->nnz = (int64_t)doc.size();
    finish_timings(c, R);
    return G2N_OK;
  }
  if (m >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, "graph JSON: 2^32-1 or more entries");
  if (n && (!blob || !offs)) throw Failure(G2N_E_DEVICE, "graph JSON: the build returned no names");

  // ---- O1, O2: the records' orientation spans (plain mode: entry k is record k)
  const GjOri* ori = !multi && m ? gj_spans(c, in, len, m) : nullptr;
  phase(c, "gj_spans");

  // ---- G1-G7: the links in listing order
  const GjLinks K = gj_links(c, rows, cols, m, step, multi && !directed, multi, n);
  const uint64_t n_links = K.n_links;
  const uint32_t *ls = K.ls, *lt = K.lt, *lx = K.lx;
  phase(c, "gj_order");

  // ---- T1-T3: the text
  const uint64_t n_items = n + n_links + 1;
  auto* dhead = dget<uint8_t>(c, S_GJHEADSTR, head_str.size());
  G2N_HIP(hipMemcpyAsync(dhead, head_str.data(), head_str.size(), hipMemcpyHostToDevice, c->stream));
  auto* nesc = dget<uint64_t>(c, S_EBAD, n);
  auto* ilen = dget<uint64_t>(c, S_ELEN, n_items + 1);
  auto* ipos = dget<uint64_t>(c, S_EPOS, n_items + 1);
  hipLaunchKernelGGL(k_gj_name_esc, dim3(grid_for(n)), dim3(kTPB), 0, c->stream, blob, offs, n, nesc);
  hipLaunchKernelGGL(k_gj_node_len, dim3(grid_for(n)), dim3(kTPB), 0, c->stream, (const uint64_t*)nesc, n,
                     (uint64_t)head_str.size(), ilen);
  hipLaunchKernelGGL(k_gj_link_len, dim3(grid_for(n_links + 2)), dim3(kTPB), 0, c->stream, (const uint32_t*)ls,
                     (const uint32_t*)lt, (const uint32_t*)lx, n_links, (int)multi, (const uint64_t*)nesc, ori, in, len,
                     ilen + n);
  excl_scan<uint64_t>(c, ilen, ipos, n_items + 1);
  const uint64_t total = read_dev(c, ipos + n_items);  // (the copy of head has landed too: the stream is idle)
  auto* text = dget<uint8_t>(c, S_ETEXT, total + 16);
  GjText T{};
  T.n = n;
  T.n_links = n_links;
  T.multi = (int)multi;
  T.head = dhead;
  T.head_len = (uint32_t)head_str.size();
  T.blob = blob;
  T.offs = offs;
  T.nesc = nesc;
  T.ls = ls;
  T.lt = lt;
  T.lx = lx;
  T.ori = ori;
  T.in = in;
  T.len = len;
  T.pos = ipos;
  hipLaunchKernelGGL(k_gj_text, dim3((unsigned)((n_items + kGjItems - 1) / kGjItems)), dim3(kTPB), 0, c->stream, T, text);
  phase(c, "gj_text");
  R->data = text;
  R->nnz = (int64_t)total;
  finish_timings(c, R);
  return G2N_OK;
}

#undef GJ_LEN

}  // namespace g2n
