// g2n_graphgexf.hip — export --format gexf (cli.py:296-297): nx.write_gexf(G, path) of the graph
// parse_gfa(build_graph=True, directed=True, bidirected=..., keep_directed_bidir=...) builds, rendered in HBM
// without building a graph object.  Included by g2n_pipeline.hip behind g2n_graphjson.hip, whose build
// (gj_build), orientation spans (O1/O2) and listing order (G1-G7) are used as they are: GEXFWriter.add_edges
// walks G.edges(data=True[, keys=True]), the sequence node_link_data walks.
//
// The document (encoding utf-8, prettyprint, version 1.2draft; networkx/readwrite/gexf.py imports
// xml.etree.ElementTree and nothing else, so the bytes are a function of the graph, the creator string and
// the date):
//   HEAD   the XML declaration, <gexf ...>, <meta lastmodifieddate="DATE"> / <creator>: composed by the caller
//          (g2n_graph_gexf_from_path / _from_buffer), escaped there
//   <graph defaultedgetype="directed|undirected" mode="static" name="">     (undirected: the MultiGraph)
//     <attributes mode="static" class="edge"> ...   only when an edge is written: plain mode declares
//          0 orientation_from / 1 orientation_to (string), the multigraph modes 0 networkx_key (long)
//     <nodes> one <node id="K" label="K" /> per node id </nodes>            (<nodes /> without nodes)
//     <edges> per link l in listing order <edge source="S" target="T" id="l"> with its <attvalues>: the
//          two orientation strings of the group's last record (plain) or the key </edges>   (<edges /> without)
// K = str(key): the ASCII key, or with bytes keys (want_node_names == 0) the bytes repr (gx_repr).  Attribute
// values are escaped as ElementTree._escape_attrib does (gx_put): & < > " and \r; every other byte as it is.
//
// The chosen constants (tests/test_gpu_graph_gexf_shapes.py is keyed to them):
//   kGxItems = 128   items per render block, one per thread
//   kGxLds   = 32 KiB  the LDS stage: 256 bytes per item.  A plain-mode edge is 174 bytes of fixed text, its
//                    id, two orientation strings and two names, so blocks of edges whose two names total up
//                    to ~70 bytes are staged; five blocks fit a CU's 160 KiB.
//
// T1  k_gx_name_esc   the written length of every node's K (used twice per node, once per link end)
// T2  k_gx_len        item lengths: n nodes (item 0 behind the prefix: HEAD .. <nodes>), n_links links (the
//                     first behind </nodes><edges>), the closing item; excl_scan<uint64_t> -> positions
// T3  k_gx_text       k_gj_text's scheme: kGxItems consecutive items per block, assembled in LDS at their offset
//                     from the 16-byte-aligned start of the block's range, written with aligned 16-byte stores;
//                     a block whose text exceeds the stage writes its items straight to HBM.
// No atomics, no loop over a row or a group: as the JSON path.
#pragma once

namespace g2n {

constexpr uint32_t kGxItems = 128;
constexpr uint32_t kGxLds = 32 * 1024;

// ------------------------------------------------------------------ escapes ----
// one character of an attribute value (ElementTree._escape_attrib; '\n' and '\t' never occur in a field).
// kW: write at d + o (else count only); returns the offset behind it.
template <bool kW>
__device__ inline uint64_t gx_put(uint8_t* d, uint64_t o, uint32_t c) {
  switch (c) {
    case '&':
      if (kW) gj_lit(d + o, "&amp;");
      return o + 5;
    case '<':
      if (kW) gj_lit(d + o, "&lt;");
      return o + 4;
    case '>':
      if (kW) gj_lit(d + o, "&gt;");
      return o + 4;
    case '"':
      if (kW) gj_lit(d + o, "&quot;");
      return o + 6;
    case '\r':
      if (kW) gj_lit(d + o, "&#13;");
      return o + 5;
    default:
      if (kW) d[o] = (uint8_t)c;
      return o + 1;
  }
}

template <bool kW>
__device__ inline uint64_t gx_esc(uint8_t* d, const uint8_t* __restrict__ s, uint64_t n) {
  uint64_t o = 0;
  for (uint64_t i = 0; i < n; i++) o = gx_put<kW>(d, o, s[i]);
  return o;
}

// str(key) of a bytes key (CPython bytes_repr): b, the quote — '"' exactly when the key holds a "'" and no
// '"' —, inside it a backslash before a backslash and before the quote, \t \n \r, \xNN (lower case) for every
// other byte outside 0x20-0x7e; then escaped as above.
template <bool kW>
__device__ inline uint64_t gx_repr(uint8_t* d, const uint8_t* __restrict__ s, uint64_t n) {
  bool sq = false, dq = false;
  for (uint64_t i = 0; i < n; i++) {
    sq |= s[i] == '\'';
    dq |= s[i] == '"';
  }
  const uint32_t q = sq && !dq ? '"' : '\'';
  uint64_t o = gx_put<kW>(d, 0, 'b');
  o = gx_put<kW>(d, o, q);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t c = s[i];
    if (c == q || c == '\\') {
      o = gx_put<kW>(d, o, '\\');
      o = gx_put<kW>(d, o, c);
    } else if (c == '\t' || c == '\n' || c == '\r') {
      o = gx_put<kW>(d, o, '\\');
      o = gx_put<kW>(d, o, c == '\t' ? 't' : c == '\n' ? 'n' : 'r');
    } else if (c < 0x20 || c >= 0x7F) {
      const uint32_t hi = c >> 4, lo = c & 15u;
      o = gx_put<kW>(d, o, '\\');
      o = gx_put<kW>(d, o, 'x');
      o = gx_put<kW>(d, o, hi < 10 ? '0' + hi : 'a' + (hi - 10));
      o = gx_put<kW>(d, o, lo < 10 ? '0' + lo : 'a' + (lo - 10));
    } else {
      o = gx_put<kW>(d, o, c);
    }
  }
  return gx_put<kW>(d, o, q);
}

// an orientation span (k_gj_ori): the constant byte '+' / '-' or bytes of the staged input
template <bool kW>
__device__ inline uint64_t gx_esc_ori(uint8_t* d, const uint8_t* __restrict__ in, uint64_t len, uint64_t off,
                                      uint32_t n) {
  if (off & kConstFlag) {
    if (kW) d[0] = (uint8_t)(off & 0xFF);
    return 1;
  }
  if (off > len || n > len - off) return 0;  // (never: the spans come from lines inside [0, len))
  return gx_esc<kW>(d, in + off, n);
}

#define GX_LEN(s) ((uint64_t)(sizeof(s) - 1))
#define GX_NODES_OPEN "    <nodes>\n"
#define GX_NODE_A "      <node id=\""
#define GX_NODE_B "\" label=\""
#define GX_NODE_C "\" />\n"
#define GX_MID "    </nodes>\n    <edges>\n"
#define GX_EDGE_A "      <edge source=\""
#define GX_EDGE_B "\" target=\""
#define GX_EDGE_C "\" id=\""
#define GX_EDGE_D "\">\n        <attvalues>\n          <attvalue for=\"0\" value=\""
#define GX_EDGE_E "\" />\n          <attvalue for=\"1\" value=\""
#define GX_EDGE_F "\" />\n        </attvalues>\n      </edge>\n"
#define GX_TAIL_EDGES "    </edges>\n  </graph>\n</gexf>\n"
#define GX_TAIL_NONE "    </nodes>\n    <edges />\n  </graph>\n</gexf>\n"
#define GX_EMPTY "    <nodes />\n    <edges />\n  </graph>\n</gexf>\n"

// ------------------------------------------------------------------ T1-T3: the text ----
__global__ void __launch_bounds__(kTPB) k_gx_name_esc(const uint8_t* __restrict__ blob, const int64_t* __restrict__ offs,
                                                      uint64_t n, int raw, uint64_t* __restrict__ nesc) {
  const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  const int64_t o = offs[i];
  const uint64_t nl = (uint64_t)(offs[i + 1] - o);
  nesc[i] = raw ? gx_repr<false>(nullptr, blob + o, nl) : gx_esc<false>(nullptr, blob + o, nl);
}

struct GxText {
  uint64_t n, n_links;         // items: n nodes, n_links links, the closing item
  int multi, raw;
  const uint8_t* head;         // the prefix: HEAD, <graph>, the attributes block, <nodes>
  uint32_t head_len;
  const uint8_t* blob;         // node keys
  const int64_t* offs;
  const uint64_t* nesc;
  const uint32_t *ls, *lt, *lx;
  const GjOri* ori;            // plain mode
  const uint8_t* in;           // the staged input (orientation spans)
  uint64_t len;
  const uint64_t* pos;         // n + n_links + 2 positions
};

// item e of n + n_links + 1; entry n + n_links + 1, 0, ends the scan
__global__ void __launch_bounds__(kTPB) k_gx_len(GxText T, uint64_t* __restrict__ ilen) {
  const uint64_t e = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
  const uint64_t n_items = T.n + T.n_links + 1;
  if (e > n_items) return;
  uint64_t b = 0;
  if (e < T.n) {
    b = (e ? 0 : T.head_len) + GX_LEN(GX_NODE_A) + GX_LEN(GX_NODE_B) + GX_LEN(GX_NODE_C) + 2 * T.nesc[e];
  } else if (e < T.n + T.n_links) {
    const uint64_t l = e - T.n;
    const uint32_t x = T.lx[l];
    b = (l ? 0 : GX_LEN(GX_MID)) + GX_LEN(GX_EDGE_A) + GX_LEN(GX_EDGE_B) + GX_LEN(GX_EDGE_C) + GX_LEN(GX_EDGE_D) +
        GX_LEN(GX_EDGE_F) + T.nesc[T.ls[l]] + T.nesc[T.lt[l]] + gj_ndig((uint32_t)l);
    if (T.multi) {
      b += gj_ndig(x);
    } else {
      const GjOri o = T.ori[x];
      b += GX_LEN(GX_EDGE_E) + gx_esc_ori<false>(nullptr, T.in, T.len, o.uo, o.ul) +
           gx_esc_ori<false>(nullptr, T.in, T.len, o.vo, o.vl);
    }
  } else if (e == n_items - 1) {
    b = T.n_links ? GX_LEN(GX_TAIL_EDGES) : GX_LEN(GX_TAIL_NONE);
  }
  ilen[e] = b;
}

__device__ inline uint8_t* gx_key(uint8_t* d, const GxText& T, uint32_t id) {
  const int64_t o = T.offs[id];
  const uint64_t nl = (uint64_t)(T.offs[id + 1] - o);
  if (T.raw) return d + gx_repr<true>(d, T.blob + o, nl);
  if (T.nesc[id] == nl) {  // nothing to escape
    for (uint64_t k = 0; k < nl; k++) d[k] = T.blob[o + k];
    return d + nl;
  }
  return d + gx_esc<true>(d, T.blob + o, nl);
}

__device__ inline uint8_t* gx_dec(uint8_t* d, uint32_t x) {
  const uint32_t nd = gj_ndig(x);
  for (uint32_t k = nd; k-- > 0; x /= 10u) d[k] = (uint8_t)('0' + x % 10u);
  return d + nd;
}

__device__ inline void gx_item(uint8_t* d, const GxText& T, uint64_t e) {
  if (e < T.n) {
    if (!e) {
      for (uint32_t k = 0; k < T.head_len; k++) d[k] = T.head[k];
      d += T.head_len;
    }
    d = gj_lit(d, GX_NODE_A);
    d = gx_key(d, T, (uint32_t)e);
    d = gj_lit(d, GX_NODE_B);
    d = gx_key(d, T, (uint32_t)e);
    gj_lit(d, GX_NODE_C);
    return;
  }
  const uint64_t l = e - T.n;
  if (l == T.n_links) {
    if (T.n_links) gj_lit(d, GX_TAIL_EDGES);
    else gj_lit(d, GX_TAIL_NONE);
    return;
  }
  if (!l) d = gj_lit(d, GX_MID);
  const uint32_t x = T.lx[l];
  d = gj_lit(d, GX_EDGE_A);
  d = gx_key(d, T, T.ls[l]);
  d = gj_lit(d, GX_EDGE_B);
  d = gx_key(d, T, T.lt[l]);
  d = gj_lit(d, GX_EDGE_C);
  d = gx_dec(d, (uint32_t)l);
  d = gj_lit(d, GX_EDGE_D);
  if (T.multi) {
    d = gx_dec(d, x);
  } else {
    const GjOri o = T.ori[x];
    d += gx_esc_ori<true>(d, T.in, T.len, o.uo, o.ul);
    d = gj_lit(d, GX_EDGE_E);
    d += gx_esc_ori<true>(d, T.in, T.len, o.vo, o.vl);
  }
  gj_lit(d, GX_EDGE_F);
}

__global__ void __launch_bounds__(kGxItems) k_gx_text(GxText T, uint8_t* __restrict__ out) {
  __shared__ uint4 stage4[kGxLds / 16];
  uint8_t* stage = (uint8_t*)stage4;
  const uint64_t n_items = T.n + T.n_links + 1;
  const uint64_t e0 = (uint64_t)blockIdx.x * kGxItems;
  const uint64_t e1 = e0 + kGxItems < n_items ? e0 + kGxItems : n_items;
  const uint64_t p0 = T.pos[e0], p1 = T.pos[e1];  // pos holds n_items + 1 entries
  const uint64_t base = p0 & ~15ull;
  const bool staged = p1 - base <= kGxLds;  // block-uniform
  const uint64_t e = e0 + threadIdx.x;
  if (e < e1) {
    const uint64_t pe = T.pos[e];
    gx_item(staged ? stage + (pe - base) : out + pe, T, e);
  }
  if (!staged) return;
  __syncthreads();
  const uint64_t w0 = base >> 4, w1 = (p1 + 15) >> 4;
  for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGxItems) {
    const uint64_t a = w << 4;
    if (a >= p0 && a + 16 <= p1) {
      *(uint4*)(out + a) = stage4[w - w0];
    } else {
      for (uint64_t b = a < p0 ? p0 : a; b < a + 16 && b < p1; b++) out[b] = stage[b - base];
    }
  }
}

// ------------------------------------------------------------------ the driver ----
// The document's HEAD, set by the entry points that take it (thread-local, as the stats request).
static thread_local const GexfHead* t_gexf_head = nullptr;
void set_gexf_head(const GexfHead* head) { t_gexf_head = head; }

// G2N_OUT_GRAPH_GEXF.  Result: format G2N_FMT_TEXT, data = the document, nnz = its bytes.
static int run_graph_gexf(g2n_context* c, const uint8_t* in, uint64_t len, const g2n_options* o, g2n_result* R) {
  if (!t_gexf_head) throw Failure(G2N_E_ARG, "graph GEXF: the document's head comes with g2n_graph_gexf_from_path / _from_buffer");
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
  std::string head_str((const char*)t_gexf_head->p, (size_t)t_gexf_head->n);
  head_str += std::string("  <graph defaultedgetype=\"") + (directed ? "directed" : "undirected") +
              "\" mode=\"static\" name=\"\">\n";
  if (n == 0) {  // no records: the constant document
    const std::string doc = head_str + GX_EMPTY;
    auto* text = dget<uint8_t>(c, S_ETEXT, doc.size() + 16);
    G2N_HIP(hipMemcpyAsync(text, doc.data(), doc.size(), hipMemcpyHostToDevice, c->stream));
    G2N_HIP(hipStreamSynchronize(c->stream));
    R->data = text;
    R->nnz = (int64_t)doc.size();
    finish_timings(c, R);
    return G2N_OK;
  }
  if (m >= 0xFFFFFFFFull) throw Failure(G2N_E_UNSUPPORTED, "graph GEXF: 2^32-1 or more entries");
  if (!blob || !offs) throw Failure(G2N_E_DEVICE, "graph GEXF: the build returned no names");

  const GjOri* ori = !multi && m ? gj_spans(c, in, len, m) : nullptr;
  phase(c, "gx_spans");
  const GjLinks K = gj_links(c, rows, cols, m, step, multi && !directed, multi, n);
  phase(c, "gx_order");

  // ---- T1-T3: the text
  if (K.n_links) {  // get_attr_id inserts the block in front of <nodes> when the first edge declares an attribute
    head_str += "    <attributes mode=\"static\" class=\"edge\">\n";
    if (multi) {
      head_str += "      <attribute id=\"0\" title=\"networkx_key\" type=\"long\" />\n";
    } else {
      head_str += "      <attribute id=\"0\" title=\"orientation_from\" type=\"string\" />\n";
      head_str += "      <attribute id=\"1\" title=\"orientation_to\" type=\"string\" />\n";
    }
    head_str += "    </attributes>\n";
  }
  head_str += GX_NODES_OPEN;
  if (head_str.size() >= 0xFFFFFFFFull) throw Failure(G2N_E_ARG, "graph GEXF: the head is too long");
  const uint64_t n_items = n + K.n_links + 1;
  auto* dhead = dget<uint8_t>(c, S_GJHEADSTR, head_str.size());
  G2N_HIP(hipMemcpyAsync(dhead, head_str.data(), head_str.size(), hipMemcpyHostToDevice, c->stream));
  auto* nesc = dget<uint64_t>(c, S_EBAD, n);
  auto* ilen = dget<uint64_t>(c, S_ELEN, n_items + 1);
  auto* ipos = dget<uint64_t>(c, S_EPOS, n_items + 1);
  GxText T{};
  T.n = n;
  T.n_links = K.n_links;
  T.multi = (int)multi;
  T.raw = (int)!keys_str;
  T.head = dhead;
  T.head_len = (uint32_t)head_str.size();
  T.blob = blob;
  T.offs = offs;
  T.nesc = nesc;
  T.ls = K.ls;
  T.lt = K.lt;
  T.lx = K.lx;
  T.ori = ori;
  T.in = in;
  T.len = len;
  T.pos = ipos;
  hipLaunchKernelGGL(k_gx_name_esc, dim3(grid_for(n)), dim3(kTPB), 0, c->stream, blob, offs, n, T.raw, nesc);
  hipLaunchKernelGGL(k_gx_len, dim3(grid_for(n_items + 1)), dim3(kTPB), 0, c->stream, T, ilen);
  excl_scan<uint64_t>(c, ilen, ipos, n_items + 1);
  const uint64_t total = read_dev(c, ipos + n_items);  // (the copy of head has landed too: the stream is idle)
  auto* text = dget<uint8_t>(c, S_ETEXT, total + 16);
  hipLaunchKernelGGL(k_gx_text, dim3((unsigned)((n_items + kGxItems - 1) / kGxItems)), dim3(kGxItems), 0, c->stream, T,
                     text);
  phase(c, "gx_text");
  R->data = text;
  R->nnz = (int64_t)total;
  finish_timings(c, R);
  return G2N_OK;
}

#undef GX_LEN

}  // namespace g2n
