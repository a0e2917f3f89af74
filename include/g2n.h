/*
 * g2n.h — C-ABI of the MI355X-native GFA -> CSR ingest path (libg2n.so).
 *
 * Drop-in boundary for the hot path of sclipman/gfa2network (reference @ 2025-07-04).
 * The reference is pure Python and has no FFI of its own; these entry
 * points are what its Python call surface binds through ctypes (INTEGRATION.md shows the
 * stub a maintainer adds).  Plain pointers and sizes only: no torch / numpy types.
 *
 *   g2n_build_from_path    replaces GFAParser(path) iteration + the build_matrix=True
 *                          branch of parse_gfa      gfa2network/parser.py:95-176,
 *                                                    gfa2network/builders.py:129-299
 *   g2n_build_from_buffer  same, for an in-memory / already-read file object
 *                          (GFAParser(BinaryIO) parser.py:90-92, stdin parser.py:104-105)
 *   g2n_build_device       same, input already resident in HBM (the measured hot path)
 *   g2n_coo_to_csr         replaces convert_format(A, "csr") = A.asformat("csr")
 *                          for a COO matrix   gfa2network/utils.py:40-63 (scipy coo.tocsr)
 *
 * Output selection (g2n_options.output):
 *   G2N_OUT_PARSE  exactly what parse_gfa(..., build_matrix=True) returns: the MAX-SYM
 *                  CSR when graph_directed and not asymmetric (builders.py:282-283),
 *                  otherwise the stream-order, unsummed COO (builders.py:281).
 *   G2N_OUT_CSR    what convert_format(parse_gfa(...), "csr") returns (cli.py:239).
 *   G2N_OUT_EDGE_LIST  the bytes `gfa2network export --format edge-list [--bidirected]`
 *                  writes (cli.py:264-281): "u\tv\n" per L/E/C record in stream order
 *                  (bidirected: "u:ori\tv:ori\n").  Only `bidirected` is read from the
 *                  options.  Result format G2N_FMT_TEXT: data = the text, nnz = its length.
 *                  An endpoint key that is not UTF-8 (the export's u.decode() raises):
 *                  status G2N_E_UNICODE with err_line = -1, err_index = the edge record,
 *                  err_detail = the key, and the text holds the lines written before it.
 *                  Parse errors (err_line >= 0) carry no text: the caller renders the
 *                  input's prefix [0, start of err_line) to reproduce the partial output.
 *   G2N_OUT_GRAPH_JSON  the bytes `gfa2network export --format json [--bidirected
 *                  [--keep-directed-bidir]]` writes (cli.py:282-306): json.dump of
 *                  nx.node_link_data(G) for the DiGraph / MultiGraph / MultiDiGraph that
 *                  parse_gfa(build_graph=True, directed=True, ...) builds: nodes in first-touch
 *                  order, links in NetworkX's adjacency order.  `bidirected` and
 *                  `keep_directed_bidir` select the class; `want_node_names` = 0 is
 *                  --raw-bytes-id.  Result format G2N_FMT_TEXT: data = the document, nnz = its
 *                  length.  The reference builds the graph before it opens its output, so a
 *                  failed build carries no text.  With str keys (want_node_names = 1) a node key
 *                  with a byte >= 0x80 is G2N_E_UNICODE with err_line = -1, err_index = the node
 *                  id and err_detail = the key (the graph path decodes keys as ASCII); it wins
 *                  over a parse error on a later line, and has_warning is set only when the
 *                  unsupported record precedes the key's first touch.  With bytes keys a graph
 *                  that has a node carries no text (data = NULL, n_nodes > 0): json.dump writes
 *                  up to the first node's id and raises TypeError.  Limits: fewer than 2^32 - 1
 *                  entries (add_edge calls) and 2^31 - 1 nodes, else G2N_E_UNSUPPORTED.
 *   G2N_OUT_GRAPH_GEXF  the bytes `gfa2network export --format gexf [--bidirected
 *                  [--keep-directed-bidir]]` writes (cli.py:296-297): nx.write_gexf(G, path) with
 *                  its defaults (utf-8, prettyprint, version 1.2draft) for the same graph, its
 *                  nodes and edges in the same order as the JSON document's.  The document opens
 *                  with a head that holds the date and the NetworkX version, so this output is
 *                  built through g2n_graph_gexf_from_path / _from_buffer, which take the head
 *                  (G2N_E_ARG from the plain build entry points).  Options, result, errors and
 *                  limits as G2N_OUT_GRAPH_JSON's, except that bytes keys (want_node_names = 0)
 *                  give a complete document: a key is written as str(key), the bytes repr.
 *
 * Errors: a non-zero status is one of G2N_E_*; each maps 1:1 to the exception the
 * reference raises for the same input (type + message; the Python shim re-raises it).
 * Everything runs on the GPU: there is no CPU fallback.  Without a usable HIP device the
 * build entry points return G2N_E_DEVICE.
 */
#ifndef G2N_H
#define G2N_H

#include <stddef.h>
#include <stdint.h>

#define G2N_VERSION_STRING "0.3.0" /* == gfa2network_amd.__version__ (tests check) */

#ifdef __cplusplus
extern "C" {
#endif

#define G2N_ABI_VERSION 2u /* 2: named range / test fields replace options.reserved[] */

/* ---- status codes ------------------------------------------------------------------ */
enum {
  G2N_OK = 0,
  G2N_E_MALFORMED_L = 1,   /* ValueError("Malformed L record")   parser.py:208-209 */
  G2N_E_MALFORMED_E = 2,   /* ValueError("Malformed E record")   parser.py:251-252 */
  G2N_E_MALFORMED_C = 3,   /* ValueError("Malformed C record")   parser.py:299-300 */
  G2N_E_MALFORMED_P = 4,   /* ValueError("Malformed P record")   parser.py:231-232 */
  G2N_E_MALFORMED_O = 5,   /* ValueError("Malformed O record")   parser.py:345-346 */
  G2N_E_INDEX_LIST = 6,    /* IndexError("list index out of range"): S without a name, parser.py:163 */
  G2N_E_INDEX_BYTES = 7,   /* IndexError("index out of range"): u_field[-1] on b"", parser.py:220-221 */
  G2N_E_UNICODE = 8,       /* UnicodeDecodeError: err_detail bytes .decode() (parser.py:127,212,214,291,293,337,339) */
  G2N_E_INT_TOO_LARGE = 9, /* OverflowError("int too large to convert to float"), builders.py:209 */
  G2N_E_CAST_OVERFLOW = 10,/* OverflowError("Python integer X out of bounds for <dtype>"), builders.py:281 */
  G2N_E_CAST_INF = 11,     /* OverflowError("cannot convert float infinity to integer"), builders.py:281 */
  G2N_E_CAST_NAN = 12,     /* ValueError("cannot convert float NaN to integer"), builders.py:281 */
  G2N_E_ARG = 13,          /* invalid options / arguments */
  G2N_E_IO = 14,           /* OSError opening/reading the input; errno in err_index */
  G2N_E_GZIP = 15,         /* corrupt gzip stream (gzip.open path, parser.py:108-109) */
  G2N_E_DEVICE = 16,       /* no usable HIP device / HIP runtime failure */
  G2N_E_NOMEM = 17,        /* host or device allocation failure */
  G2N_E_UNSUPPORTED = 18   /* input exceeds a documented implementation limit */
};

/* ---- matrix dtypes (cli.py:92-97 --dtype choices) ------------------------------------ */
enum { G2N_BOOL = 0, G2N_INT8 = 1, G2N_INT32 = 2, G2N_FLOAT32 = 3, G2N_FLOAT64 = 4 };

enum {
  G2N_OUT_PARSE = 0,
  G2N_OUT_CSR = 1,
  G2N_OUT_COO = 2,
  G2N_OUT_EDGE_LIST = 3,
  G2N_OUT_GRAPH_JSON = 4,
  G2N_OUT_GRAPH_GEXF = 5
};
enum { G2N_FMT_COO = 0, G2N_FMT_CSR = 1, G2N_FMT_TEXT = 2 };

/* Mirrors parse_gfa's keyword arguments that affect the matrix (builders.py:30-50). */
typedef struct g2n_options {
  uint32_t abi_version;        /* = G2N_ABI_VERSION */
  int32_t directed;            /* default 1 */
  int32_t bidirected;          /* default 0 */
  int32_t keep_directed_bidir; /* default 0 */
  int32_t asymmetric;          /* default 0 */
  int32_t strip_orientation;   /* default 0 */
  int32_t dtype;               /* G2N_* dtype, default G2N_FLOAT64 */
  int32_t output;              /* G2N_OUT_PARSE (default) | G2N_OUT_CSR | G2N_OUT_COO (the
                                  stream-order COO in every mode: one shard of a sharded build) */
  const char *weight_tag;      /* UTF-8, NUL-terminated; NULL or "" = no weights */
  int32_t want_node_names;     /* 1 (default): produce the names blob in id order */
  int32_t device;              /* HIP device ordinal, default 0 */
  /* ---- set by the sharded / chunked protocol (gfa2network_amd/shard.py); 0 in a plain build ---- */
  int32_t unknown_warned;      /* 1: unsupported records are skipped silently (an earlier byte range
                                  of the same file already raised the one-shot warning) */
  int32_t range_flags;         /* G2N_RANGE_* bits, below */
  int64_t range_s_base;        /* G2N_RANGE_DECIMAL: S lines in the file before this byte range */
  int64_t range_n_segments;    /* G2N_RANGE_DECIMAL: S lines in the whole file */
  /* ---- tests only ---- */
  uint32_t test_flags;         /* G2N_TEST_* bits: take a normally rare path (same results) */
  int32_t reserved_[3];        /* must be 0 (g2n_options_init) */
} g2n_options;

/* g2n_options.range_flags */
enum {
  G2N_RANGE_DECIMAL = 1,        /* one byte range of a sharded decimal-id build: this range's node ids
                                   are global decimals (range_s_base / range_n_segments); output
                                   G2N_OUT_COO, no names; G2N_E_UNSUPPORTED when the range needs the
                                   general protocol (ids that are not decimal, errors, warnings, slow
                                   weights) */
  G2N_RANGE_EVIDENCE = 2,       /* with DECIMAL: report the range's evidence instead of checking the
                                   premise (set by g2n_build_decimal_range) */
  G2N_RANGE_NO_VALUES = 4,      /* no weight tag and the caller reads coordinates only: the result's
                                   values are left unwritten */
  G2N_RANGE_SLOTS = 8           /* with DECIMAL and NO_VALUES (unweighted, not bidirected): the COO stays
                                   in the tile-local parse's group slots (no stream-order compaction);
                                   result rows / cols are the slot arrays, nnz the entries they hold,
                                   the layout from g2n_context_group_slots — what
                                   g2n_route_group_slots and g2n_csr_from_group_slots read */
};

/* g2n_options.test_flags (tests only; every real build leaves 0): the same results through a path
 * that is normally rare on the given input. */
enum {
  G2N_TEST_NO_BUCKETS = 2,      /* MAX-SYM / SUM CSR through the general row sums */
  G2N_TEST_NO_LEAN = 4,         /* decimal ids without the lean parse */
  G2N_TEST_DICT_HASH = 8,       /* hash dictionary (no decimal ids, no direct-address tier) */
  G2N_TEST_DICT_GENERAL = 16,   /* general dictionary rounds */
  G2N_TEST_NO_TILE_LOCAL = 32,  /* decimal ids parsed after K1 (not the tile-local pass) */
  G2N_TEST_HOST_INFLATE = 64,   /* a BGZF .gz read by the host readers (not inflated on the GPU) */
  G2N_TEST_NO_GROUP = 128,      /* tile-local parse into per-tile slots + compaction */
  G2N_TEST_NO_HASH_LEAN = 256,  /* the classic hash tiers, never the lean S-first one */
  G2N_TEST_THROW_AFTER_IDS = 512, /* the build fails (G2N_E_DEVICE) once its ids are set up */
  G2N_TEST_INDEX64 = 1024,      /* CSR results in int64 indptr / indices (the > 2^31 - 1 entries path) */
  G2N_TEST_DICT_DIRECT = 2048,  /* decimal ids in S order through the direct-address tier */
  G2N_TEST_NO_DIRECT = 4096,    /* never the direct-address tier (the lean hash tier instead) */
  G2N_TEST_NO_EXT_LEAN = 8192,  /* bidirected / weighted decimal builds: K1 + the lean parse, not the
                                   extended tile-local parse */
  G2N_TEST_NO_DEC_TEXT = 16384, /* edge-list export of a decimal-id build through the names blob, not
                                   the arithmetic render */
  G2N_TEST_NO_DEC_PREFIX = 32768, /* names "P1".."PN" in S order through the direct-address tier, not
                                   the tile-local decimal parse behind the prefix */
  G2N_TEST_NO_DIRECT_FINISH = 65536 /* the MAX-SYM bucket finish through its staged route (F1, scan, F2),
                                   never counted first and written in place */
};

#define G2N_MAX_PHASES 40

/* Result of one build.  All pointers are owned by the result (host memory for the
 * host entry points, device memory for g2n_build_device) and stay valid until
 * g2n_result_free (or, for g2n_build_device, until the next build on the context). */
typedef struct g2n_result {
  uint32_t abi_version;
  int32_t status;              /* G2N_OK or G2N_E_* */
  int64_t err_line;            /* 0-based input line of the failing record (parse errors) */
  int64_t err_index;           /* cast errors: element index in the triplet stream; IO: errno */
  double err_value;            /* cast errors: the offending float64 value */
  const uint8_t *err_detail;   /* G2N_E_UNICODE: the bytes whose .decode() raises */
  int64_t err_detail_len;
  int32_t has_warning;         /* RuntimeWarning("Skipping unsupported record: <c>") */
  int32_t warn_byte;           /* <c> (first byte of the first unsupported line) */
  int64_t warn_line;           /* first unsupported-record line (-1: none), warned or not */
  int64_t n_lines;             /* lines seen (Python binary line iteration) */
  int64_t n_records;           /* records the parser yielded (S/L/E/C/P/O) */
  int64_t n_records_before_error;
  int64_t n_edges;             /* L + E + C records */
  int64_t n_nodes;             /* matrix is n_nodes x n_nodes */
  const uint8_t *names_blob;   /* node keys in id order (builders.py:284-288), concatenated */
  const int64_t *names_offsets;/* n_nodes + 1 offsets into names_blob */
  int32_t format;              /* G2N_FMT_COO | G2N_FMT_CSR */
  int32_t dtype;
  int32_t index_width;         /* 4 (int32) or 8 (int64) for rows/cols/indptr/indices */
  int32_t sum_sorted;          /* scipy has_sorted_indices of the scattered COO (diagnostic; -1: not
                                  computed — the CSR came from the bucket partition) */
  int64_t nnz;                 /* COO: triplet count; CSR: stored entries */
  const void *rows;            /* COO */
  const void *cols;            /* COO */
  const void *indptr;          /* CSR: n_nodes + 1 */
  const void *indices;         /* CSR */
  const void *data;            /* nnz elements of dtype */
  uint64_t names_bytes;        /* names blob length (0 when want_node_names is 0) */
  int64_t n_cast_overflow;     /* float32 casts that overflowed to +-inf: numpy warns
                                  RuntimeWarning("overflow encountered in cast") once each */
  uint64_t input_bytes;        /* uncompressed GFA bytes parsed */
  int32_t n_phases;            /* device phase timings (hipEvent, pipeline stream) */
  int32_t sum_t_sorted;        /* MAX-SYM: has_sorted_indices of A.T's scattered COO (diagnostic; -1: not
                                  computed — the bucket partition's staged finish; -2: its finish
                                  counted first and written in place) */
  double phase_ms[G2N_MAX_PHASES];
  const char *phase_names[G2N_MAX_PHASES];
  double host_ms_read;         /* host ingest (read / inflate) */
  double host_ms_h2d;          /* host -> device copy of the input */
  double host_ms_d2h;          /* device -> host copy of the outputs */
  void *priv_;
} g2n_result;

/* ---- library ------------------------------------------------------------------------- */
const char *g2n_version(void);
uint32_t g2n_abi_version(void);
void g2n_options_init(g2n_options *opts);      /* reference defaults (builders.py:30-50) */
int g2n_device_count(void);                    /* HIP devices visible (0 without a GPU) */
/* hipMemGetInfo of `device`: free / total HBM bytes (G2N_E_DEVICE without such a device).  What
 * parse_gfa sizes its one-GPU chunked build by (gfa2network_amd/api.py), without torch. */
int g2n_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes);
/* The host entry points (g2n_build_from_path / _buffer, g2n_coo_to_csr) keep one cached context per
 * device whose grow-only buffers outlive the call (results are host copies).  This frees them all
 * (*freed: the bytes released): what parse_gfa does before sizing a build against free HBM when an
 * earlier, larger build's buffers would otherwise count as used. */
int g2n_release_shared(int32_t device, uint64_t *freed);
const char *g2n_last_error(void);              /* thread-local message of the last failure */
const char *g2n_status_name(int status);

/* ---- host entry points (results in host memory) ---------------------------------------- */
/* path: "-" = stdin; a name ending in ".gz" is gunzipped (multi-member); anything else is
 * read raw — the same rule as parser.py:100-112 (by name, not by magic bytes). */
int g2n_build_from_path(const char *path, const g2n_options *opts, g2n_result **out);
int g2n_build_from_buffer(const void *buf, size_t len, const g2n_options *opts, g2n_result **out);
/* export --format gexf: the same two with opts->output taken as G2N_OUT_GRAPH_GEXF.  head (head_len bytes,
 * host) opens the document: everything nx.write_gexf writes before the <graph> element — the XML
 * declaration, the <gexf ...> tag and the <meta lastmodifieddate="DATE"><creator>...</creator></meta>
 * block, each line with its newline — already escaped; it is copied as it is.  The result's text
 * (G2N_FMT_TEXT) is the whole document, the head included. */
int g2n_graph_gexf_from_path(const char *path, const g2n_options *opts, const void *head, size_t head_len,
                             g2n_result **out);
int g2n_graph_gexf_from_buffer(const void *buf, size_t len, const g2n_options *opts, const void *head,
                               size_t head_len, g2n_result **out);
void g2n_result_free(g2n_result *res);

/* gzip.open(...).read() of an in-memory .gz file (parser.py:108-109): the reader that
 * g2n_build_from_path uses for ".gz" names.  parallel = 1: members are inflated concurrently
 * on host threads (G2N_HOST_THREADS) when the file is a clean member chain, else serially;
 * parallel = 0: always the serial reader.  On success *out (free with g2n_free) holds *out_len
 * bytes and *members the member count.  On failure returns G2N_E_GZIP, *sub = the exception
 * gzip.py raises (1 BadGzipFile, 2 EOFError, 3 zlib.error, 4 BadGzipFile CRC/length),
 * g2n_last_error() its message, and *out / *out_len the bytes gzip.py's reader returned before
 * raising (io.BufferedReader refills of 8192: what a line loop over gzip.open sees; g2n_free it). */
int g2n_gunzip(const void *buf, size_t len, int32_t parallel, void **out, size_t *out_len, int32_t *members,
               int32_t *sub);
/* The chunk-parallel single-member inflate alone (what g2n_gunzip's parallel path tries first
 * for a file of >= 64 MiB with few member candidates): one gzip member to the end of the file
 * (zero padding allowed), its deflate stream cut into chunks of chunk_bytes compressed bytes
 * (0 = sized for the host threads) that are inflated concurrently.  G2N_OK with *out / *out_len
 * (g2n_free) and *chunks = the chunks that decoded from a block start of their own; G2N_E_UNSUPPORTED
 * when it declines (not one clean member, or a stream its decoder refuses: the exact reader decides).
 * Replaces gzip.open's serial read of one member (parser.py:108-109). */
int g2n_gunzip_chunked(const void *buf, size_t len, size_t chunk_bytes, void **out, size_t *out_len,
                       int32_t *chunks);
void g2n_free(void *p);

/* parse_gfa(..., split_on_alignment=True) (builders.py:110-128 -> _parse_gfa_split,
 * builders.py:302-568), host side: the segments cut at the E / C alignment coordinates, the
 * records re-targeted to the intervals, and that record stream rendered as GFA text ("S" lines
 * for the interval segments unless bidirected, "E\t*\tu\tori\tv\tori[\ttags]" for every link
 * and edge) for g2n_build_from_buffer to build with the reference's main-path semantics.  The
 * input must have parsed cleanly first (errors are the plain parse's).  names = the interval
 * segments in mint order (bidirected: placed before the GPU build's nodes); warn_* = the
 * "skipping edge / link" warnings in order (kind 0 edge, 1 link; the segment bytes);
 * many_nodes = the ">10x more nodes" warning; g2n_split_segments = intervals per segment.  G2N_E_UNSUPPORTED for a length or coordinate
 * beyond int64.  Free with g2n_split_free. */
typedef struct g2n_split_out g2n_split_out;
int g2n_split_render(const void *buf, size_t len, int32_t bidirected, g2n_split_out **out);
void g2n_split_get(const g2n_split_out *o, const uint8_t **text, uint64_t *text_len, const uint8_t **names,
                   const int64_t **name_offs, uint64_t *n_names, const uint8_t **warn_segs,
                   const int64_t **warn_offs, const int32_t **warn_kind, uint64_t *n_warn, int32_t *many_nodes);
/* intervals per segment (the segments dict's order): the bidirected id map's block sizes */
void g2n_split_segments(const g2n_split_out *o, const int64_t **intervals, uint64_t *n_segments);
void g2n_split_free(g2n_split_out *o);

/* The node list's bytes joined by `sep` (builders.py:284-288 node_list, built in one pass by
 * the Python shim): out (n_names ? blob_len + n_names - 1 : 0 bytes) = name 0, sep, name 1, ...
 * with name i = blob[offsets[i] .. offsets[i+1]).  Host memory, parallel over host threads. */
int g2n_join_names(const uint8_t *blob, const int64_t *offsets, uint64_t n_names, uint8_t sep, uint8_t *out);

/* Names in a new order: out name i = name order[i] of (blob, offsets), written at out_offsets[i] -
 * out_offsets[0] (the caller scans the reordered lengths).  The sharded build's node list: each
 * owner rank's distinct keys arrive in owner order and are put in global id order
 * (builders.py:284-288 node_list = keys in node2idx insertion order).  Host threads. */
int g2n_gather_names(const uint8_t *blob, const int64_t *offsets, const int64_t *order, uint64_t n_names,
                     const int64_t *out_offsets, uint8_t *out);

/* ---- convert CLI writers (host threads) -------------------------------------------------
 * scipy.sparse.save_npz(path, A) as `convert --matrix x.npz` calls it (utils.py:85-86): a
 * zip64 archive of deflated members (numpy savez_compressed's layout).  Member i is named
 * names[i] and holds heads[i] (its .npy header, head_lens[i] bytes, built by numpy's format
 * code) followed by datas[i] (data_lens[i] bytes).  level: zlib level (-1 = zlib's default, as
 * numpy).  Returns G2N_E_IO (errno text in g2n_last_error) when the file cannot be written. */
int g2n_write_npz(const char *path, int32_t n_members, const char *const *names, const uint8_t *const *heads,
                  const uint64_t *head_lens, const void *const *datas, const uint64_t *data_lens, int32_t level);

/* save_node_map (utils.py:108-114): "i\tname\n" for the names blob/offsets in id order.
 * check_utf8 = 1 (raw_bytes_id names, decoded while writing): only the names before the first
 * one that is not valid UTF-8 are written and *bad_index is its id (-1: all valid). */
int g2n_write_node_map(const char *path, const uint8_t *blob, const int64_t *offsets, uint64_t n_names,
                       int32_t check_utf8, int64_t *bad_index);

/* The components CLI's listing: "name\tlabel\n" for the names blob/offsets in id order, labels[i] the
 * int32 label of node i.  path "-" writes to standard output (the ranges are written in order, so
 * the target may be a pipe).  check_utf8 and *bad_index as g2n_write_node_map's. */
int g2n_write_node_labels(const char *path, const uint8_t *blob, const int64_t *offsets, const int32_t *labels,
                          uint64_t n_names, int32_t check_utf8, int64_t *bad_index);

/* Index of the first name that is not valid UTF-8 (Python's strict decoder), or -1. */
int64_t g2n_first_bad_utf8(const uint8_t *blob, const int64_t *offsets, uint64_t n_names);

/* ---- convert CLI dense writers (GPU) ------------------------------------------------------
 * `convert --matrix x.csv` / `x.npy` (utils.py:87-96): np.savetxt(dest, A.toarray(), delimiter=",",
 * fmt="%.6g") and np.save(dest, A.toarray()) of a CSR matrix, byte for byte, without the dense array:
 * the document is rendered on the device in bands of band_bytes (g2n_dense.hip) and streamed to the
 * file — a band renders while the one before it is copied to pinned host memory and the one before
 * that is written.  The CSR is in HOST memory: indptr (n_rows + 1) / indices of index_width 4 or 8
 * bytes, data of `dtype` (one of the five G2N_* codes), n_rows, n_cols >= 1 and < 2^31 - 1, fewer than
 * 2^32 - 1 entries (else G2N_E_UNSUPPORTED); rows sorted and free of duplicates.  kind: 0 the csv, 1
 * the .npy, whose header `head` (head_len bytes, built by the caller with numpy's format code; empty
 * for the csv) is written first.  band_bytes: 0 = sized from the device's free memory, else a multiple
 * of info->tile_bytes.  info: doc_bytes = the bytes of the body (the file holds head_len more), bands,
 * tile_bytes = the aligned tile of the csv one render block writes, band_bytes = the band used.
 * declined = 1 (status G2N_OK, the file not touched): a row whose columns do not ascend strictly —
 * numpy's toarray() adds duplicates in an order that is scipy's, so the caller takes numpy's route.
 * G2N_E_ARG for an indptr that is no non-decreasing map into [0, nnz] or a column outside [0, n_cols)
 * (nothing out of range is ever addressed); G2N_E_IO, the errno's text in g2n_last_error, when the
 * file cannot be opened or written.  Device memory: the CSR, 25 bytes per entry (csv) and two bands. */
typedef struct g2n_dense_info {
  uint64_t doc_bytes, bands, tile_bytes, band_bytes;
  int32_t declined;
} g2n_dense_info;
int g2n_write_dense(const char *path, int32_t kind /* 0 csv, 1 npy */, const void *head, size_t head_len,
                    const void *indptr, const void *indices, int32_t index_width, const void *data, int32_t dtype,
                    uint64_t n_rows, uint64_t n_cols, uint64_t band_bytes /* 0 = default */, int32_t device,
                    g2n_dense_info *info);
/* Where the calling thread's last g2n_write_dense spent its time, in ms: out_ms[0] the upload of the
 * CSR with D1 and the scan (host clock), [1] the bands' renders and [2] their copies to the host
 * (hipEvent, summed over the bands: they overlap each other and the writes), [3] the write(2) calls
 * (host clock), [4] the whole call. */
void g2n_dense_last_times(double out_ms[5]);
/* Bytes [b0, b1) of the same document's body (b0 <= b1 <= info->doc_bytes, else G2N_E_ARG) to out
 * (host, b1 - b0 bytes): what the band loop renders, for any place of a document too large to write.
 * info as above with bands = band_bytes = 0; declined = 1 leaves out unwritten. */
int g2n_dense_range(int32_t kind, const void *indptr, const void *indices, int32_t index_width, const void *data,
                    int32_t dtype, uint64_t n_rows, uint64_t n_cols, int32_t device, uint64_t b0, uint64_t b1,
                    uint8_t *out, g2n_dense_info *info);
/* Python's '%.6g' % v (what np.savetxt writes per cell; csrc/g6fmt.h, the code the device runs): the
 * text into out[0 .. length), at most 13 bytes, out[15] = the length, the bytes between zero.  Returns
 * the length.  Exact for every double: 6 significant digits, ties to even on the binary value. */
uint32_t g2n_format_g6(double v, uint8_t out[16]);

/* convert_format(A, "csr") for a COO matrix (utils.py:40-63 -> scipy coo.tocsr):
 * sums duplicates in dtype with scipy's summation order, keeps explicit zeros.
 * rows/cols have index_width (4) bytes per element, data has dtype elements; n_rows x n_cols
 * (each < 2^31 - 1).  indptr / indices come back in scipy's index dtype: int64 (index_width 8)
 * once nnz passes 2^31 - 1 (_coo_to_compressed: maxval = coo.nnz, duplicates included).  Up to
 * 2^32 - 2 entries when every value is dtype(1) (a parse without a weight tag); other values
 * past 2^31 - 2 entries return G2N_E_UNSUPPORTED.  test_flags: G2N_TEST_INDEX64 /
 * G2N_TEST_NO_BUCKETS (tests only; 0 otherwise). */
int g2n_coo_to_csr(const void *rows, const void *cols, const void *data, int64_t nnz, int64_t n_rows,
                   int64_t n_cols, int32_t index_width, int32_t dtype, int32_t device, uint32_t test_flags,
                   g2n_result **out);

/* One row band of a COO too large for g2n_coo_to_csr's weighted limit (rows band-local, 0..n_rows-1,
 * in the whole COO's stream order): the band's CSR.  force_unsorted = -1: the band's own sortedness
 * decides (as for a whole matrix); 0 / 1: scipy's has_sorted_indices verdict of the WHOLE matrix
 * (coo.tocsr -> sum_duplicates sorts every row when any is unsorted, utils.py:55), which decides
 * the order float duplicates are summed in.  result.sum_sorted: this band's own verdict (-1: the
 * band's sums cannot depend on order).  The caller (gfa2network_amd/_native.py coo_to_csr) cuts the
 * bands, asks each for its verdict, re-runs the sorted ones with 1 when another is unsorted, and
 * concatenates them with int64 indptr / indices as scipy returns past 2^31 - 1 entries. */
int g2n_coo_to_csr_band(const void *rows, const void *cols, const void *data, int64_t nnz, int64_t n_rows,
                        int64_t n_cols, int32_t dtype, int32_t device, int32_t force_unsorted, g2n_result **out);

/* ---- device-resident entry points (the measured hot path) ------------------------------ */
typedef struct g2n_context g2n_context;
g2n_context *g2n_context_create(int device);   /* NULL on failure (see g2n_last_error) */
void g2n_context_destroy(g2n_context *ctx);
void *g2n_context_stream(g2n_context *ctx);    /* the hipStream_t the pipeline runs on */
/* d_input: len bytes already in this device's HBM.  The result's pointers are DEVICE
 * pointers owned by ctx, valid until the next build on ctx.  The call returns after the
 * stream has drained (counts must be read back); phase timings are hipEvent-based. */
int g2n_build_device(g2n_context *ctx, const void *d_input, size_t len, const g2n_options *opts,
                     g2n_result *out);
/* Release ctx's grow-only arena buffers except those holding one of the n_keep device pointers
 * (results the caller still reads, e.g. a build's rows / cols): the working set of one sharded rank
 * between protocol stages (its dictionary, touch descriptors, partition buffers), which would
 * otherwise stay allocated until ctx's next build needs them.  *freed (optional) = bytes released.
 * No reference counterpart (the reference has no device memory); a later call re-allocates. */
int g2n_context_trim(g2n_context *ctx, const void *const *keep, uint64_t n_keep, uint64_t *freed);

/* ---- sharded build: device-side steps of one file split over ranks --------
 * Each rank builds its byte range with output = G2N_OUT_COO (local ids = first-touch order
 * inside the range, local names blob).  The protocol (gfa2network_amd/shard.py) routes names
 * to owner ranks, where g2n_dedup_keys keeps the first occurrence of each key in arrival
 * order (arrivals are concatenated in rank order, so that is the global first-touch order);
 * global ids go back to the ranks, g2n_route_triplets remaps and partitions the COO by the
 * owner of each row (and, for MAX-SYM, of each column: the A.T stream), and
 * g2n_csr_from_coo_pair builds the rank's CSR row slice.  All pointers are DEVICE pointers
 * on ctx's device; calls return after the stream drained. */

/* keys i in [0, n): bytes d_blob[d_offsets[i] .. d_offsets[i+1]).  d_ids[i] = index of key i's
 * distinct key, numbered in order of first occurrence; d_first[k] = first occurrence of
 * distinct key k (k < *n_distinct; d_first sized n).  Exact byte comparison. */
int g2n_dedup_keys(g2n_context *ctx, const uint8_t *d_blob, uint64_t blob_len, const int64_t *d_offsets,
                   uint64_t n, uint32_t *d_ids, uint32_t *d_first, uint64_t *n_distinct);

/* A growing device set of byte keys with dense ids in insertion order (the chunked build's
 * file-wide names, gfa2network_amd/shard.py _chunked_general; replaces re-running
 * g2n_dedup_keys over every key so far for each chunk).  g2n_keyset_add looks up keys i < n
 * (d_blob / d_offsets as for g2n_dedup_keys; DISTINCT within one call): d_ids[i] = the key's id,
 * a key not in the set yet taking the next id in call order (builders.py:194-198 first-touch
 * minting); *n_total = keys in the set after the call.  g2n_keyset_view: the set's keys in id
 * order (device pointers owned by the set, valid until its next add or free).  The set works on
 * ctx's device and stream; ctx must outlive every add / view (g2n_keyset_free does not use it). */
typedef struct g2n_keyset g2n_keyset;
int g2n_keyset_create(g2n_context *ctx, g2n_keyset **out);
int g2n_keyset_add(g2n_keyset *ks, const uint8_t *d_blob, uint64_t blob_len, const int64_t *d_offsets, uint64_t n,
                   uint32_t *d_ids, uint64_t *n_total);
int g2n_keyset_view(g2n_keyset *ks, const uint8_t **d_blob, const int64_t **d_offsets, uint64_t *n,
                    uint64_t *blob_len);
void g2n_keyset_free(g2n_keyset *ks);

/* Key i of the names blob goes to rank fmix64(FNV-1a 64 of its bytes) mod n_ranks (fmix64:
 * MurmurHash3's 64-bit finaliser; 1 <= n_ranks <= 4096, else G2N_E_ARG) — every rank of a group,
 * on whichever GPU, computes the same owner: the keys, grouped by rank (order kept within a rank),
 * to d_out_blob / d_out_offsets (n + 1); d_out_index[j] = the input index of output key j;
 * d_starts[r] = first output key of rank r (d_starts[n_ranks] = n). */
int g2n_partition_keys(g2n_context *ctx, const uint8_t *d_blob, uint64_t blob_len, const int64_t *d_offsets,
                       uint64_t n, uint32_t n_ranks, uint8_t *d_out_blob, int64_t *d_out_offsets,
                       uint32_t *d_out_index, uint32_t *d_starts);

/* Keys d_index[j] (j < n) of a names blob, in that order, to d_out_blob (out_cap bytes) and
 * d_out_offsets (n + 1); *out_len = bytes written.  G2N_E_ARG if they exceed out_cap (nothing
 * written to d_out_blob then).  The owner's distinct keys for the names gather. */
int g2n_gather_keys(g2n_context *ctx, const uint8_t *d_blob, const int64_t *d_offsets, const uint32_t *d_index,
                    uint64_t n, uint8_t *d_out_blob, uint64_t out_cap, int64_t *d_out_offsets, uint64_t *out_len);

/* d_rows[i] = d_map[d_rows[i]], d_cols[i] = d_map[d_cols[i]] in place (i < n): a range's COO
 * from local to global ids.  G2N_E_ARG if an id is >= n_map (those entries become -1). */
int g2n_remap_pairs(g2n_context *ctx, const uint32_t *d_map, uint64_t n_map, int32_t *d_rows, int32_t *d_cols,
                    uint64_t n);

/* Triplet i = (d_map[d_rows[i]],d_map[d_cols[i]], d_data[i]) (transposed: row and column
 * swapped) goes to rank floor(row * n_ranks / n_global); the output holds them grouped by
 * rank, stream order kept within a rank; d_starts[r] = first output of rank r
 * (d_starts[n_ranks] = nnz).  Outputs sized nnz (data: nnz elements of dtype).  d_map may be
 * NULL: the identity map (the rows / cols already hold global ids, the decimal-id shard path).
 * d_data and d_out_data both NULL: the coordinates only (uniform values need no routing). */
int g2n_route_triplets(g2n_context *ctx, const int32_t *d_rows, const int32_t *d_cols, const void *d_data,
                       uint64_t nnz, int32_t dtype, const uint32_t *d_map, uint64_t n_global, uint32_t n_ranks,
                       int32_t transposed, int32_t *d_out_rows, int32_t *d_out_cols, void *d_out_data,
                       uint32_t *d_starts);

/* CSR of rows [row_base, row_base + n_rows) from the stream-order triplets of A whose rows
 * fall there (global row ids) and, for MAX-SYM, those of A.T (rows = A's columns):
 * maxsym = 0: coo.tocsr() of A's slice; 1: A.maximum(A.T)'s slice.  uniform: every value is
 * dtype(1) (no weight tag).  force_unsorted: -1 = this slice decides scipy's
 * has_sorted_indices; else the caller's global verdicts (the OR over all slices), bit 0 for
 * A, bit 1 for A.T (only weighted float rows of > 16 entries depend on them).  The result's
 * sum_sorted / sum_t_sorted report this slice's own verdicts.  Result pointers are device pointers
 * owned by ctx (format CSR, n_nodes = n_rows). */
int g2n_csr_from_coo_pair(g2n_context *ctx, const int32_t *a_rows, const int32_t *a_cols, const void *a_data,
                          uint64_t a_nnz, const int32_t *t_rows, const int32_t *t_cols, const void *t_data,
                          uint64_t t_nnz, int32_t maxsym, int64_t row_base, uint64_t n_rows, uint64_t n_cols,
                          int32_t dtype, int32_t uniform, int32_t force_unsorted, g2n_result *out);

/* Group slots (round 6): a sharded decimal range built with G2N_RANGE_SLOTS keeps its COO where the
 * tile-local parse wrote it — group g's entries at [g * gcap, g * gcap + gcount[g]) of rows / cols —
 * instead of compacting it into stream order.  g2n_context_group_slots reports the last build's layout
 * on ctx (n_groups 0: the last build left none); valid until ctx's next build.
 * g2n_route_group_slots: g2n_route_triplets of those slots (coordinates only, no map, n_ranks <= 256;
 *   nnz = the entries they hold; within an owner the order is slot order, which an unweighted slice
 *   CSR does not read).
 * g2n_csr_from_group_slots: a ONE-rank group's whole CSR (row_base 0, n_rows rows) from the slots —
 *   the SUM CSR (maxsym 0) or A.maximum(A.T) (maxsym 1) of unit values, the single-GPU bucket
 *   partition; G2N_E_UNSUPPORTED when it declines (no entries, an overfull bucket): the caller then
 *   builds the range's stream-order COO and calls g2n_csr_from_coo_pair. */
int g2n_context_group_slots(g2n_context *ctx, const uint32_t **d_gcount, uint64_t *n_groups, uint64_t *gcap);
int g2n_route_group_slots(g2n_context *ctx, const int32_t *d_rows, const int32_t *d_cols, const uint32_t *d_gcount,
                          uint64_t n_groups, uint64_t gcap, uint64_t nnz, uint64_t n_global, uint32_t n_ranks,
                          int32_t transposed, int32_t *d_out_rows, int32_t *d_out_cols, uint32_t *d_starts);
int g2n_csr_from_group_slots(g2n_context *ctx, const int32_t *d_rows, const int32_t *d_cols, const uint32_t *d_gcount,
                             uint64_t n_groups, uint64_t gcap, uint64_t nnz, int32_t maxsym, uint64_t n_rows,
                             int32_t dtype, g2n_result *out);

/* The general protocol's global node ids (shard.py step 4; builders.py:194-198 first-touch order
 * across byte ranges), on an owner rank's distinct keys (g2n_dedup_keys):
 * g2n_order_keys: out[j] = (source rank << 32) | the key's local id there, for the key's first arrival
 *   f = d_first_of[j], the source being the one whose arrival range holds f (src_ends: the sources'
 *   inclusive arrival-count prefix sums, host memory, n_src <= 4096); d_src_idx[f] = the local id the
 *   source sent with arrival f.  The keys ascend with j.
 * g2n_rank_keys: out[j] = j + the number of keys smaller than d_keys[j] in every other owner's sorted
 *   run of d_all (runs at all_offsets[o] .. all_offsets[o + 1], host memory): the key's global id. */
int g2n_order_keys(g2n_context *ctx, const uint32_t *d_first_of, const int64_t *d_src_idx, uint64_t nd,
                   const uint64_t *src_ends, uint32_t n_src, uint64_t *d_out);
int g2n_rank_keys(g2n_context *ctx, const uint64_t *d_keys, uint64_t n, const uint64_t *d_all,
                  const uint64_t *all_offsets, uint32_t n_ranks, uint32_t self_rank, int64_t *d_out);

/* One rank's byte range of a file split over ranks: bytes [offset, offset + len) of path, read
 * with pread into pinned staging slots and copied to d_dst (len bytes of `device`'s HBM). */
int g2n_upload_file_range(const char *path, uint64_t offset, uint64_t len, void *d_dst, int32_t device);

/* The record counts of a device-resident range, before any build (what the ranks of a sharded
 * build exchange first): out4 = {lines, S lines, edge records (L/E/C), records (S/L/E/C/P/O)}. */
int g2n_count_device(g2n_context *ctx, const void *d_input, size_t len, int64_t *out4);

/* One byte range of a sharded decimal-id build (S lines named "1".."N" in order), built BEFORE the
 * ranges' record counts are exchanged: one pass of the tile-local lean parse writes the range's
 * stream-order COO over GLOBAL ids (name value - 1; builders.py:190-198 first-touch order when the
 * premise holds) and reports the evidence the caller checks across ranges (shard.py):
 *   ev6 = {lines, S lines, edge records, records,
 *          d: the range's first S line names d + 1 and every later one continues it (-1: no S line;
 *             the premise needs d == the S lines of the ranges before),
 *          the largest edge key value (the premise needs it <= the file's S lines)}.
 * Options: output G2N_OUT_COO, no names, not bidirected, no weight tag, no strip (else G2N_E_ARG);
 * range_* are set by the call (G2N_RANGE_NO_VALUES is kept).  G2N_E_UNSUPPORTED when the one pass declines (a line past
 * its tile window, a record outside the lean shapes, S names that are not one decimal run, an S
 * line after an edge line in the range): the caller then counts the ranges (g2n_count_device) and
 * builds with G2N_RANGE_DECIMAL (g2n_build_device), whose check decides.  Replaces the count pass of
 * the sharded build for the common layout; results as g2n_build_device's (device pointers). */
int g2n_build_decimal_range(g2n_context *ctx, const void *d_input, size_t len, const g2n_options *opts,
                            int64_t *ev6, g2n_result *out);

/* ---- graph statistics (gfa2network/analysis.py:33-65 compute_stats, cli.py:364-376) ------------
 * What the reference reads off a NetworkX graph, as integer work on a CSR's structure (the values
 * are never read): n_nodes = n, n_entries = nnz, n_diag = rows that hold their own index,
 * n_components = connected components with every stored (u, v) joining u and v (isolated nodes
 * count; a lock-free union-find, the same count on every run), max_degree = the largest of
 *   directed (nx.DiGraph):  row length + occurrences of the row's index as a column
 *   undirected (nx.Graph):  row length + 1 if the row holds its own index
 * (0 when n == 0).  Edges and density follow from these in the caller (Python ints: n * (n - 1)
 * passes 2^53 inside the supported range).  ms_*: hipEvent times of the two kernel groups. */
typedef struct g2n_graph_stats {
  int64_t n_nodes, n_entries, n_diag, n_components, max_degree;
  double ms_degree, ms_components; /* hipEvent, pipeline stream */
} g2n_graph_stats;

/* d_indptr (n + 1) / d_indices (nnz): DEVICE pointers on ctx's device, index_width 4 (int32) or 8
 * (int64) bytes per element; scratch from ctx's arena; returns after the stream drained.
 * G2N_E_UNSUPPORTED for n >= 2^31 - 1 or nnz >= 2^32 - 1 (the build's own limits); G2N_E_ARG when
 * indptr is not a non-decreasing map into [0, nnz] or an index is outside [0, n) (nothing out of
 * range is ever addressed). */
int g2n_csr_stats(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width, uint64_t n,
                  uint64_t nnz, int32_t directed, g2n_graph_stats *out);

/* The same for a CSR in HOST memory: uploaded to `device` (the host entry points' cached context). */
int g2n_csr_stats_host(const void *indptr, const void *indices, int32_t index_width, uint64_t n, uint64_t nnz,
                       int32_t directed, int32_t device, g2n_graph_stats *out);

/* compute_stats(path): the input is ingested as by g2n_build_from_path (plain, gzip, BGZF) and
 * built as a plain graph — of opts only directed, strip_orientation, want_node_names, device,
 * unknown_warned and test_flags are read; the build is not bidirected, unweighted, asymmetric, its
 * output the summed CSR, which stays on the device — then g2n_csr_stats runs on it and only the
 * scalars come back.  *n_paths = the P / O records (records - edges - S lines).  *res (free with
 * g2n_result_free) carries status, error and warning fields, counts and phase times as a build's,
 * no matrix and no names.  want_node_names = 1 asks for the graph path's ASCII decode of node keys
 * (builders.py:155-162; 0 = raw_bytes_id): after a clean build, a key with a byte >= 0x80 gives
 * status G2N_E_UNICODE with err_line = -1, err_index = the lowest such node id and err_detail = its
 * key (whose .decode("ascii") raises the reference's error). */
int g2n_stats_from_path(const char *path, const g2n_options *opts, g2n_graph_stats *out, int64_t *n_paths,
                        g2n_result **res);

/* ---- connected components: node labels and the matrix regrouped by component (extension) ----------
 * Every stored (u, v) joins u and v; the values are never read.  labels[i] (int32) is the number of
 * i's component, components numbered by their smallest node index — the numbering of
 * scipy.sparse.csgraph.connected_components(A, directed=False), and of
 * enumerate(nx.connected_components(G.to_undirected())) for node ids in first-touch order.  The
 * union-find is g2n_csr_stats'; its roots are the components' smallest indices however the races go,
 * so the labels are the same on every run.  ms_*: hipEvent times of the kernel groups (the union-find,
 * the labels; the split's sort and bounds, its row starts and copy — 0 for a labels call). */
typedef struct g2n_components_info {
  int64_t n_components;
  double ms_union, ms_labels, ms_group, ms_split; /* hipEvent, pipeline stream */
} g2n_components_info;

/* d_indptr (n + 1) / d_indices (nnz) / d_labels (n, out): DEVICE pointers on ctx's device; sizes,
 * limits and G2N_E_ARG for a bad indptr / indices as g2n_csr_stats (nothing out of range is ever
 * addressed).  n = 0: no component. */
int g2n_csr_components(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width, uint64_t n,
                       uint64_t nnz, int32_t *d_labels, g2n_components_info *info);

/* The same for a CSR in HOST memory: labels (n, out) is host memory too. */
int g2n_csr_components_host(const void *indptr, const void *indices, int32_t index_width, uint64_t n, uint64_t nnz,
                            int32_t *labels, int32_t device, g2n_components_info *info);

/* The matrix regrouped by component, for a CSR in HOST memory with optional values (data: nnz items
 * of value_bytes 1, 4 or 8 bytes, copied as bits; value_bytes 0: none, data / out_data unread).  The
 * caller allocates every output:
 *   labels[n]          as above
 *   perm[n]            the nodes ordered by label, index order kept inside a component (numpy's
 *                      argsort(labels, kind="stable"))
 *   off[n + 1]         the first k + 1 are written (k = info->n_components <= n): component j's nodes
 *                      are perm[off[j] .. off[j + 1]), off[k] = n
 *   out_indptr[n + 1], out_indices[nnz], out_data[nnz]   (index_width / value_bytes as the input)
 *                      row p is the input's row perm[p], its entries in their stored order, each
 *                      column replaced by its node's index inside its own component.  Both ends of
 *                      a stored entry are in one component, so this is a permutation of the whole
 *                      matrix and component j is rows [off[j], off[j + 1]) of it: a CSR of its own
 *                      once out_indptr is rebased by out_indptr[off[j]].
 * Rows up to 64 entries are copied by a thread each, up to 4096 by a block each, longer ones by the
 * whole grid. */
int g2n_csr_split_components_host(const void *indptr, const void *indices, const void *data, int32_t value_bytes,
                                  int32_t index_width, uint64_t n, uint64_t nnz, int32_t *labels, int64_t *perm,
                                  int64_t *off, void *out_indptr, void *out_indices, void *out_data, int32_t device,
                                  g2n_components_info *info);

/* The labels of the graph compute_stats measures: ingest, build, options read, errors, the one-shot
 * warning and the ASCII key check (want_node_names = 1; 0 = raw_bytes_id) are g2n_stats_from_path's.
 * The CSR stays on the device and g2n_csr_components runs on it there.  On G2N_OK *res carries the
 * labels in `rows` (int32, n_nodes of them; no other matrix field is set) and the names
 * (names_blob / names_offsets) whatever want_node_names says. */
int g2n_components_from_path(const char *path, const g2n_options *opts, g2n_components_info *info, g2n_result **res);

/* ---- path distances (gfa2network/analysis.py genome_distance_matrix) ---------------------------
 * Hop distances between K node lists ("paths") over a CSR's structure: every stored (u, v) is an
 * edge u -> v of weight 1, the values are never read.  Path k's steps are
 * path_nodes[path_ptr[k] .. path_ptr[k + 1]) (node ids, in list order, duplicates kept);
 * path_ptr[0] = 0.  d_i(v) = hops from the nearest step of path i to v (0 on its own steps).  One
 * bit-parallel breadth-first search serves 64 paths (g2n_dist.hip).  The tables are row-major K x K:
 *   G2N_DIST_MIN   D, uint32: D[i][j] = min over the steps v of j of d_i(v); 0xFFFFFFFF = none reached
 *   G2N_DIST_MEAN  S then C, uint64 each: S[i][j] = the sum of d_i(v) over the steps v of j that i
 *                  reaches, each occurrence counted; C[i][j] = how many those are
 * (the reference's symmetric matrix: min takes D[i][j] for i < j; mean takes (S[i][j] + S[j][i]) /
 * (C[i][j] + C[j][i])).  info: levels = the deepest level any search reached, launches = kernels
 * launched by the searches, batches = ceil(K / 64); ms_*: hipEvent times (ms_resolve: the lookup of
 * step names, 0 where the caller passes node ids). */
#define G2N_DIST_MIN 0
#define G2N_DIST_MEAN 1
typedef struct g2n_dist_info {
  int64_t levels, launches, batches;
  double ms_resolve, ms_bfs; /* hipEvent, pipeline stream */
} g2n_dist_info;

/* load_paths (analysis.py:164-177), host only: the P / O records of the named file (plain, or
 * gunzipped when the name ends in ".gz") as names (blob + n_paths + 1 offsets, first-occurrence
 * order; a repeated name takes its last record's steps) and steps (blob + offsets; path k's steps
 * are steps path_ptr[k] .. path_ptr[k + 1]): field 2 cut at commas, one trailing '+' or '-' removed
 * from each, an empty field being one empty step.  bad_line = the 0-based line of the first P / O
 * record whose name or step has a byte >= 0x80 (-1: none) and bad_bytes that name or step — what
 * .decode("ascii") raises on, for the caller to order against a build's err_line.  The parser's own
 * errors are the build's to report: a record with fewer than three fields is skipped here, and on
 * a gzip error the whole lines read before it are scanned.  G2N_E_IO when the file cannot be read.
 * The pointers live until g2n_paths_free. */
typedef struct g2n_paths g2n_paths;
int g2n_load_paths(const char *path, g2n_paths **out);
void g2n_paths_get(const g2n_paths *p, const uint8_t **names, const int64_t **name_offs, uint64_t *n_paths,
                   const uint8_t **steps, const int64_t **step_offs, const int64_t **path_ptr, int64_t *bad_line,
                   const uint8_t **bad_bytes, uint64_t *bad_len);
void g2n_paths_free(g2n_paths *p);

/* genome_distance_matrix / `distance --path` (analysis.py:116-141, 180-272): the input is ingested
 * and built as by g2n_stats_from_path (of opts only directed, want_node_names, device,
 * unknown_warned and test_flags are read), the CSR and the node names stay on the device, the
 * paths' step names are looked up in the names there and g2n_csr_path_distances runs on the ids.
 * source < 0: every path of `paths` is searched, out_tables (host) = the K x K tables of all K
 * paths.  source >= 0: the two paths (source, target), out_tables = their 2 x 2 tables — cell
 * [0][1] is the answer; only the source's steps must be nodes, a target step that is none is
 * never reached.  *oriented = 1 when a node key ends in ":+" or ":-" (the reference's orientation
 * warning).  *missing_step = -1, or the first searched step that is no node (an index into the
 * steps of `paths`; source >= 0: into the source's steps): nothing is searched then.  *res as
 * g2n_stats_from_path's, want_node_names = 1 asking for the same ASCII check of node keys. */
int g2n_distances_from_path(const char *path, const g2n_options *opts, const g2n_paths *paths, int64_t source,
                            int64_t target, int32_t mode, void *out_tables, g2n_dist_info *info, int32_t *oriented,
                            int64_t *missing_step, g2n_result **res);

/* DEVICE pointers on ctx's device (index_width 4 or 8 bytes per indptr / indices element, path
 * arrays int64; a step of -1 is no node: never reached, no source); d_out_tables holds K * K * 4 (min) or K * K * 16 (mean) bytes; scratch from ctx's
 * arena; returns after the stream drained.  G2N_E_UNSUPPORTED for n >= 2^31 - 1, nnz >= 2^32 - 1,
 * 2^32 - 1 or more steps, or tables of K paths past the device's free memory; G2N_E_ARG when indptr
 * or path_ptr is not a non-decreasing map into its range or an index or step is outside [0, n)
 * (nothing out of range is ever addressed). */
int g2n_csr_path_distances(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width,
                           uint64_t n, uint64_t nnz, const int64_t *d_path_ptr, const int64_t *d_path_nodes, uint64_t K,
                           int32_t mode, void *d_out_tables, g2n_dist_info *info);

/* The same for arrays in HOST memory (out_tables too): uploaded to `device` (the host entry
 * points' cached context). */
int g2n_csr_path_distances_host(const void *indptr, const void *indices, int32_t index_width, uint64_t n, uint64_t nnz,
                                const int64_t *path_ptr, const int64_t *path_nodes, uint64_t K, int32_t mode,
                                void *out_tables, int32_t device, g2n_dist_info *info);

/* ---- weighted path distances (a graph built with weight_tag: NetworkX's multi-source Dijkstra with
 * weight="weight") -------------------------------------------------------------------------------
 * Shortest-path distances between K node lists over a CSR with float64 values: every stored entry
 * k of row u is an edge u -> indices[k] of length values[k]; repeated (u, v) are parallel edges, an
 * explicit zero is an edge of length 0 (scipy.sparse.csgraph's reading).  Every value must be
 * finite and >= 0 (-0.0 is 0): they are checked in one pass before anything is searched.  Paths as
 * in g2n_csr_path_distances.  d_i(v) = the smallest left-to-right float64 sum ((0.0 + w1) + w2) +
 * ... over the walks from a step of path i to v: 0.0 on its own steps, +inf when v is not reached
 * (or every sum overflows) — bit for bit what Dijkstra returns (g2n_wdist.hip).  The tables are
 * row-major K x K:
 *   G2N_DIST_MIN   D, float64: D[i][j] = min over the steps v of j of d_i(v); +inf = none reached
 *   G2N_DIST_MEAN  S float64, then C uint64: S[i][j] = the sum of d_i(v) over the steps v of j that
 *                  i reaches, added in step order, left to right from 0.0, each occurrence counted
 *                  (the same bits on every run); C[i][j] = how many those are
 *   G2N_DIST_MEAN_FOLD  (declared with g2n_wdistances_from_path below) the same, S above the diagonal
 *                  holding the reference's running total of the cell
 * info: rounds = the relaxation rounds of the longest batch (the last round that improved a
 * distance; at most n - 1), launches = kernels launched, batch_paths = B <= 64, the paths searched
 * together (B * n * 8 bytes of distances must fit the device's free memory), batches = ceil(K / B);
 * ms_search = the checks and the searches, ms_tables = the tables (hipEvent, pipeline stream). */
typedef struct g2n_wdist_info {
  int64_t rounds, launches, batches, batch_paths;
  double ms_search, ms_tables; /* hipEvent, pipeline stream */
} g2n_wdist_info;

/* DEVICE pointers on ctx's device (index_width 4 or 8 bytes per indptr / indices element, d_values
 * float64, path arrays int64; a step of -1 is no node); d_out_tables holds K * K * 8 (min) or
 * K * K * 16 (mean) bytes and is not written unless every array passed its check; scratch from
 * ctx's arena; returns after the stream drained.  G2N_E_UNSUPPORTED for n >= 2^31 - 1, nnz >=
 * 2^32 - 1, 2^32 - 1 or more steps, tables of K paths or one path's n distances past the device's
 * free memory; G2N_E_ARG as g2n_csr_path_distances, and for a value that is negative, NaN or
 * infinite (nothing out of range is ever addressed); G2N_E_DEVICE should a search not converge in
 * n rounds (it cannot: the loop is bounded rather than trusted). */
int g2n_csr_path_distances_weighted(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width,
                                    const double *d_values, uint64_t n, uint64_t nnz, const int64_t *d_path_ptr,
                                    const int64_t *d_path_nodes, uint64_t K, int32_t mode, void *d_out_tables,
                                    g2n_wdist_info *info);

/* The same for arrays in HOST memory (out_tables too): uploaded to `device` (the host entry
 * points' cached context). */
int g2n_csr_path_distances_weighted_host(const void *indptr, const void *indices, int32_t index_width,
                                         const double *values, uint64_t n, uint64_t nnz, const int64_t *path_ptr,
                                         const int64_t *path_nodes, uint64_t K, int32_t mode, void *out_tables,
                                         int32_t device, g2n_wdist_info *info);

/* ---- sequence distance (gfa2network/analysis.py:68-113 sequence_distance, `distance --seq`) -----
 * The fewest hops from any node whose sequence is seq_a to any node whose sequence is seq_b, over
 * the plain graph g2n_distances_from_path builds (of opts only directed, want_node_names, device,
 * unknown_warned and test_flags are read).  The input's bytes stay on the device after the build;
 * the nodes that carry a sequence are found there from its S records (g2n_seq.hip), no sequence
 * byte comes back to the host.  The sequence of an S record (parser.py:135-163): fields[2] when
 * int(fields[2]) raises ValueError (b"" and b"*" are sequences), else fields[3] when it exists and
 * is not tag-shaped (split(b":", 2) into parts of lengths 2, 1, any), else none; a line with fewer
 * than three fields has none.  The sequence of a node (builders.py:164-189): that of the last S
 * record of its name, in file order, that has one.  A query holding '\t' or '\n' matches nothing.
 * *out_dist = 0xFFFFFFFF when no node of B is reached or either set is empty (nothing is searched
 * then; the reference's KeyError is the caller's to raise from the empty list).  *hits: the two
 * node-id lists, ascending = node order, to be freed with g2n_seq_hits_free; the pointers of
 * g2n_seq_hits_get live until then.  info: n_s_lines = the S records, n_with_seq = those that have
 * a sequence, candidates_* = the records whose sequence field ends where the query would and
 * starts with its first min(len, 16) bytes (only these are compared further); levels / launches /
 * batches as g2n_dist_info's; ms_scan = the pass over the input's bytes, ms_match = the key table,
 * the per-record pass, the comparisons and the node lists, ms_bfs = the search (hipEvent, pipeline
 * stream).  *oriented and *res as g2n_distances_from_path's. */
typedef struct g2n_seq_info {
  int64_t n_s_lines, n_with_seq, candidates_a, candidates_b;
  int64_t levels, launches, batches;
  double ms_scan, ms_match, ms_bfs;
} g2n_seq_info;
typedef struct g2n_seq_hits g2n_seq_hits;
int g2n_seq_distance_from_path(const char *path, const g2n_options *opts, const uint8_t *seq_a, uint64_t len_a,
                               const uint8_t *seq_b, uint64_t len_b, uint32_t *out_dist, g2n_seq_hits **hits,
                               g2n_seq_info *info, int32_t *oriented, g2n_result **res);
void g2n_seq_hits_get(const g2n_seq_hits *h, const int64_t **ids_a, uint64_t *n_a, const int64_t **ids_b,
                      uint64_t *n_b);
/* the listed nodes' keys, A's then B's: key i is blob[offsets[i] .. offsets[i + 1]), n_a + n_b + 1 offsets */
void g2n_seq_hits_names(const g2n_seq_hits *h, const uint8_t **blob, const int64_t **offsets);
void g2n_seq_hits_free(g2n_seq_hits *h);

/* ---- the weighted graph of a file (parse_gfa(build_graph=True, weight_tag=T)) and distances over it
 * The reference's distance helpers run Dijkstra with weight="weight" over the GRAPH a weight tag
 * builds, whose edge lengths are not the summed matrix's: builders.py:246-256 calls G.add_edge(a, b,
 * weight=w) only for a record that carries a numeric tag T, and add_edge overwrites.  So the length
 * of an edge (u, v) is the weight of the LAST record of that edge, in file order, that carries a
 * numeric T (inside a record its last T field decides, and a value that is no number is none), or 1
 * when no record does; in an undirected build (u, v) and (v, u) are one edge.
 *
 * g2n_graph_weights_from_path builds that matrix ("LAST"; of opts: directed, weight_tag — required —,
 * want_node_names, device, unknown_warned, test_flags): *res holds a float64 CSR, one stored cell per
 * distinct edge (both cells of an undirected one), columns ascending within a row, an explicit 0.0
 * kept, nodes in first-touch order, with the names when want_node_names.  G2N_E_INT_TOO_LARGE as
 * ever for an integer tag float() overflows on.
 *
 * g2n_wdistances_from_path / g2n_seq_wdistance_from_path are g2n_distances_from_path /
 * g2n_seq_distance_from_path over that matrix with g2n_csr_path_distances_weighted as the search:
 * out_tables as that function's (min: K x K float64; mean and mean-fold: S float64 then C uint64),
 * *out_dist float64, +inf where the hop call has 0xFFFFFFFF.  *bad_weight = 1 when a stored value is
 * negative, NaN or infinite: nothing is searched then (NetworkX's result on such a graph depends on
 * its heap's order).  A value a later record replaced is not stored and does not count.
 *
 * G2N_DIST_MEAN_FOLD (the weighted searches only) is G2N_DIST_MEAN with, for i < j, S[i][j] = the
 * running total genome_distance_matrix keeps for the cell (analysis.py:254-264): it starts at 0.0,
 * adds d_j(u) over the steps u of path i that j reaches, then d_i(v) over the steps v of path j —
 * S[j][i] continued over path j's steps, not S[i][j] + S[j][i], which differs in the last bit for
 * general floats.  S[i][j] for i >= j and C are G2N_DIST_MEAN's. */
#define G2N_DIST_MEAN_FOLD 2
int g2n_graph_weights_from_path(const char *path, const g2n_options *opts, g2n_result **res);
int g2n_wdistances_from_path(const char *path, const g2n_options *opts, const g2n_paths *paths, int64_t source,
                             int64_t target, int32_t mode, void *out_tables, g2n_wdist_info *info, int32_t *oriented,
                             int64_t *missing_step, int32_t *bad_weight, g2n_result **res);
int g2n_seq_wdistance_from_path(const char *path, const g2n_options *opts, const uint8_t *seq_a, uint64_t len_a,
                                const uint8_t *seq_b, uint64_t len_b, double *out_dist, g2n_seq_hits **hits,
                                g2n_seq_info *info, int32_t *oriented, int32_t *bad_weight, g2n_result **res);

/* ---- node-to-node distances (gfa2network/analysis.py:142-159 genome_distance(method="mean")) --------
 * The distance from every source to every target over a CSR: what the reference takes from
 * len(A) * len(B) calls of shortest_path_length, as ceil(n_src / 64) bit-parallel breadth-first
 * searches (g2n_pairs.hip).  sources / targets are int64 node ids in list order, duplicates kept;
 * -1 is no node (a source that reaches nothing, a target nothing reaches).  d(i, t) = the hops from
 * sources[i] to targets[t], 0 when they are the same node.
 *   G2N_PAIR_SUMS   out = S then C, n_src uint64 each: C[i] = how many target occurrences source i
 *                   reaches, S[i] = the sum of their distances (O(n_src) output, whatever n_tgt)
 *   G2N_PAIR_TABLE  out = D, n_src x n_tgt uint32 row-major, 0xFFFFFFFF where t is not reached
 * info as g2n_csr_path_distances', batches = ceil(n_src / 64).  The weighted calls take float64
 * values as g2n_csr_path_distances_weighted does (finite, >= 0) and know the table only: out = n_src x
 * n_tgt float64, d(i, t) bit for bit Dijkstra's, +inf where not reached — a float sum's order is the
 * caller's to choose.  info as g2n_csr_path_distances_weighted's, with sources for paths.
 *
 * DEVICE pointers on ctx's device; scratch from ctx's arena; returns after the stream drained.
 * G2N_E_UNSUPPORTED for n >= 2^31 - 1, nnz >= 2^32 - 1, n_src or n_tgt >= 2^32 - 1; G2N_E_ARG for a
 * bad indptr, an index outside [0, n) or an id outside [0, n) other than -1 — nothing out of range is
 * ever addressed, and d_out is not written unless every array passed its check. */
#define G2N_PAIR_SUMS 0
#define G2N_PAIR_TABLE 1
int g2n_csr_pair_distances(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width,
                           uint64_t n, uint64_t nnz, const int64_t *d_sources, uint64_t n_src,
                           const int64_t *d_targets, uint64_t n_tgt, int32_t mode, void *d_out, g2n_dist_info *info);
int g2n_csr_pair_distances_weighted(g2n_context *ctx, const void *d_indptr, const void *d_indices, int32_t index_width,
                                    const double *d_values, uint64_t n, uint64_t nnz, const int64_t *d_sources,
                                    uint64_t n_src, const int64_t *d_targets, uint64_t n_tgt, void *d_out,
                                    g2n_wdist_info *info);

/* The same for arrays in HOST memory (out too): uploaded to `device` (the host entry points' cached
 * context).  Also G2N_E_UNSUPPORTED for an output past the device's free memory. */
int g2n_csr_pair_distances_host(const void *indptr, const void *indices, int32_t index_width, uint64_t n, uint64_t nnz,
                                const int64_t *sources, uint64_t n_src, const int64_t *targets, uint64_t n_tgt,
                                int32_t mode, void *out, int32_t device, g2n_dist_info *info);
int g2n_csr_pair_distances_weighted_host(const void *indptr, const void *indices, int32_t index_width,
                                         const double *values, uint64_t n, uint64_t nnz, const int64_t *sources,
                                         uint64_t n_src, const int64_t *targets, uint64_t n_tgt, void *out,
                                         int32_t device, g2n_wdist_info *info);

/* genome_distance(method="mean") of a file: built, resolved and reported as g2n_distances_from_path
 * (source, target >= 0: two paths of `paths`), with the source's steps as the sources and the target's
 * as the targets of g2n_csr_pair_distances — out (host) as that call's for `mode`, info filled, winfo
 * and bad_weight may be null.  With a weight tag in opts the graph is g2n_wdistances_from_path's LAST
 * build, mode must be G2N_PAIR_TABLE, out is the float64 table, and winfo and bad_weight are
 * required (info may be null).  *missing_step: the first step of the source that is no node (an index
 * into its steps; nothing is searched then), a target step that is none is a target never reached. */
int g2n_pair_distances_from_path(const char *path, const g2n_options *opts, const g2n_paths *paths, int64_t source,
                                 int64_t target, int32_t mode, void *out, g2n_dist_info *info, g2n_wdist_info *winfo,
                                 int32_t *oriented, int64_t *missing_step, int32_t *bad_weight, g2n_result **res);

#ifdef __cplusplus
}
#endif
#endif /* G2N_H */
