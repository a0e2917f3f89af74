// g2n_internal.h — host-side plumbing shared by g2n_pipeline.hip, g2n_host.cpp and g2n_ingest.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/g2n.h"

// g2n_load_paths' result (g2n_paths.cpp): the paths in first-occurrence order, each with the steps
// of its last record; path k's steps are steps [path_ptr[k], path_ptr[k + 1]) of step_offs.
struct g2n_paths {
  std::vector<uint8_t> names, steps;
  std::vector<int64_t> name_offs{0}, step_offs{0}, path_ptr{0};
  int64_t bad_line = -1;           // the first P / O record with a non-ASCII name or step (0-based line)
  std::vector<uint8_t> bad_bytes;  // that name or step
};

// g2n_seq_distance_from_path's node lists: the ids of the nodes that carry each sequence, ascending,
// and those nodes' keys (A's, then B's: key i is names[name_offs[i], name_offs[i + 1]))
struct g2n_seq_hits {
  std::vector<int64_t> ids[2];
  std::vector<uint8_t> names;
  std::vector<int64_t> name_offs{0};
};

namespace g2n {

// the P / O records of len bytes of GFA text into *out (g2n_paths.cpp)
void scan_paths(const uint8_t* text, size_t len, g2n_paths* out);

// Internal failure carrying a G2N_E_* status and a message for g2n_last_error().
struct Failure : std::runtime_error {
  int status;
  Failure(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

void set_last_error(const std::string& msg);

// Host threads for ingest / download (G2N_HOST_THREADS, default min(16, cores)).
int host_threads();

// Runs body(i) for i in [0, n) on up to T threads; the first exception is rethrown.
void parallel_for(size_t n, int T, const std::function<void(size_t)>& body);

// Large host buffer without value-initialisation: big allocations are 2 MiB aligned, advised
// for transparent huge pages and faulted in by host_threads() threads before a DMA lands in
// them (a fresh pageable destination otherwise caps D2H at the page-fault rate).
struct HostBuf {
  uint8_t* p = nullptr;
  size_t n = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  void reset();
  ~HostBuf();
  uint8_t* alloc(size_t bytes);  // discards old contents; returns p (never null)
  uint8_t* data() const { return p; }
};

// Host-side result storage: g2n_result plus the buffers its pointers refer to.
struct HostResult {
  g2n_result r;
  HostBuf detail, blob, rows, cols, indptr, indices, data, offs;
};

// Frees big host buffers on a detached thread (unmapping GBs of touched pages costs ~0.1 s/GB).
void free_later(std::vector<HostBuf>&& bufs);

HostResult* new_host_result();
void fill_defaults(g2n_result* r);

// Writes input bytes [off, off + len) to dst (a pinned staging slot).  Called concurrently
// from several threads with disjoint ranges; throws Failure on error.
using FillFn = std::function<void(size_t off, uint8_t* dst, size_t len)>;

// Copies len input bytes produced by `fill` into device memory d (on `device`) through the
// per-device pinned staging ring: host threads fill 16 MiB slots and issue async H2D copies on
// their own streams, so reading / copying overlaps the DMA.  Returns after every copy landed.
void staged_upload(int device, uint8_t* d, size_t len, const FillFn& fill);

// Runs the GPU pipeline on len input bytes delivered by `fill` (staged into HBM) and
// downloads the outputs.  read_ms = host time spent before the call (read / inflate).
int build_host_fill(size_t len, const FillFn& fill, const g2n_options* opts, g2n_result** out, double read_ms);
int build_host(const void* buf, size_t len, const g2n_options* opts, g2n_result** out, double read_ms);

// g2n_stats_from_path: while a request is set on the calling thread, build_host_fill / build_host_bgzf
// keep the built CSR on the device, run g2n_csr_stats on it and download the scalars only (the result
// carries status, errors, warning and counts as ever, no matrix and no names).
struct StatsRequest {
  g2n_graph_stats* out;
  int64_t* n_paths;
  int32_t directed;
  bool check_ascii;  // a node key with a byte >= 0x80: status G2N_E_UNICODE, err_line -1 (include/g2n.h)
};
void set_stats_request(const StatsRequest* req);  // nullptr: none (thread-local)

// g2n_components_from_path: the same build with its names kept whole; g2n_csr_components labels the
// CSR on the device, and the labels (the result's rows: int32, one per node) and the names come back.
struct LabelsRequest {
  g2n_components_info* info;
  bool check_ascii;  // as StatsRequest::check_ascii
};
void set_labels_request(const LabelsRequest* req);  // nullptr: none (thread-local)

// g2n_graph_gexf_from_path / _from_buffer: while set on the calling thread, a G2N_OUT_GRAPH_GEXF build opens
// its document with these bytes (host; the XML declaration through </meta>, a newline behind it).
struct GexfHead {
  const uint8_t* p;
  uint64_t n;
};
void set_gexf_head(const GexfHead* head);  // nullptr: none (thread-local)

// g2n_distances_from_path: the same, for path distances.  The build's CSR and names stay on the
// device; the K paths' step names (host blob + offsets, sources first) are looked up in the names
// there, and g2n_csr_path_distances runs on the ids.  Only the tables and the scalars come back.
struct DistRequest {
  const uint8_t* step_blob;   // host
  const int64_t* step_offs;   // host, n_steps + 1
  const int64_t* path_ptr;    // host, K + 1 offsets into the steps
  uint64_t K, n_steps;
  uint64_t n_source_steps;    // steps [0, n_source_steps) must be nodes (else *missing_step = the first that is not)
  int32_t mode;
  bool check_ascii;           // as StatsRequest::check_ascii
  bool names_if_high;         // raw keys of a directed graph: when one has a byte >= 0x80 the names come back too
                              // (the reference's orientation check decodes keys as UTF-8 until one is oriented)
  void* tables;               // host, out
  g2n_dist_info* info;
  int32_t* oriented;          // out: 1 when a node key ends in ":+" or ":-"
  int64_t* missing_step;      // out: -1, or a source step that is no node (nothing was searched then)
  // g2n_wdistances_from_path: the build is a LAST build (set_last_build) and g2n_csr_path_distances_weighted
  // searches its values; mode may be G2N_DIST_MEAN_FOLD.  winfo replaces info (null then).
  g2n_wdist_info* winfo;      // non-null: the weighted request
  int32_t* bad_weight;        // out: 1 when a stored value is negative or not finite (nothing was searched then)
  // g2n_pair_distances_from_path: K = 2, and the two paths' steps are the sources and the targets of
  // g2n_csr_pair_distances(_weighted); mode is a G2N_PAIR_* then and tables that call's output.
  bool pairs;
};
void set_dist_request(const DistRequest* req);  // nullptr: none (thread-local)

// A LAST build: while set on the calling thread, a host build produces the weighted CSR of the graph
// parse_gfa(build_graph=True, weight_tag=T) builds (g2n_pipeline.hip csr_last: the row finish's Last policy) — a cell's value is that of
// its last record carrying a numeric tag T, 1.0 without one — instead of the summed matrix.
void set_last_build(bool on);

// g2n_seq_distance_from_path: the same, for the distance between two sequences.  The staged input
// stays on the device next to the CSR and the names; the nodes whose sequence equals a query are
// found in its S records there (g2n_seq.hip) and g2n_csr_path_distances runs on the two id lists.
// Only the ids, one distance and the scalars come back.
struct SeqRequest {
  const uint8_t* seq[2];  // host: the two queries
  uint64_t len[2];
  bool check_ascii;       // as StatsRequest::check_ascii
  bool names_if_high;     // as DistRequest::names_if_high
  uint32_t* dist;         // out: the fewest hops from a node of A to a node of B; 0xFFFFFFFF: none reached, or a set is empty
  double* wdist;          // non-null (g2n_seq_wdistance_from_path, a LAST build; dist is null then): the shortest
                          // weighted distance instead, +inf: none reached, or a set is empty
  int32_t* bad_weight;    // ... and 1 when a stored value is negative or not finite (nothing was searched then)
  g2n_seq_hits* hits;     // out: the two lists of node ids, ascending
  g2n_seq_info* info;
  int32_t* oriented;      // out: 1 when a node key ends in ":+" or ":-"
};
void set_seq_request(const SeqRequest* req);  // nullptr: none (thread-local)

// Parallel multi-member gunzip.  Members are found by their header bytes and inflated
// speculatively on host_threads() threads; the chain of members from byte 0 (zero padding
// between members skipped, gzip.py _read_eof) is then walked in order.  Returns false when
// the input is not a clean chain of valid members (bad magic, trailing garbage, corrupt or
// truncated data): the caller then runs the serial gunzip, which raises the exact error.
struct Inflated {
  std::vector<HostBuf> parts;
  std::vector<size_t> start;  // output offset of each part (+ total at the end)
  size_t total = 0;
  int members = 0;
};
// Runs f; a Failure / bad_alloc / std::exception becomes its status + g2n_last_error().
int guarded(const std::function<int()>& f);
bool gunzip_parallel(const uint8_t* in, size_t n, Inflated& out);
// One gzip member spanning the whole file (zero padding after it allowed), inflated chunk-parallel
// (g2n_pinflate.cpp); chunk_bytes 0 = sized for the host threads.  false = declined (not one
// clean member, or anything the decoder refuses): the caller runs the member-chain readers.
bool gunzip_chunked(const uint8_t* in, size_t n, size_t chunk_bytes, Inflated& out);
// One member of a BGZF chain: its deflate data z[in_off, in_off + in_len), its output
// [out_off, out_off + out_len) (ISIZE) and the trailer's CRC-32.
struct ZMember {
  unsigned long long in_off, out_off;
  uint32_t in_len, out_len, crc, pad_;
};
// A clean BGZF chain (every member's size from its 'BC' subfield, members back to back, no
// other header fields, ISIZE <= 64 KiB): true with the members and the total output size.
bool bgzf_members(const uint8_t* in, size_t n, std::vector<ZMember>& out, size_t* total_out);
// g2n_build_from_path's ".gz" path for a BGZF chain: the compressed bytes to the GPU, the members
// inflated there (g2n_inflate.hip), then the build.  kBgzfFallback: a member did not inflate
// cleanly — the caller reads the file with the host readers instead.
constexpr int kBgzfFallback = -1;
constexpr uint32_t kTestHostInflate = G2N_TEST_HOST_INFLATE;  // BGZF read by the host readers
int build_host_bgzf(const uint8_t* z, size_t zlen, const std::vector<ZMember>& members, size_t total_out,
                    const g2n_options* opts, g2n_result** out, double read_ms);
// gzip.open's reader restated (serial, exact errors): false with *sub = 1 BadGzipFile,
// 2 EOFError, 3 zlib.error, 4 BadGzipFile (CRC / length) and *msg = the exception's message;
// `out` then holds the bytes the reference's reader returned before raising (not cut to lines).
bool gunzip_exact(const uint8_t* in, size_t n, Inflated& out, int* sub, std::string* msg);

// convert CLI writers (g2n_writers.cpp)
int write_npz(const std::string& path, int n, const char* const* names, const uint8_t* const* heads,
              const uint64_t* head_lens, const void* const* datas, const uint64_t* data_lens, int level);
int write_node_map(const std::string& path, const uint8_t* blob, const int64_t* offs, uint64_t n);
int64_t first_bad_utf8(const uint8_t* blob, const int64_t* offs, uint64_t n);
// "name\tlabel\n" per node (the components CLI's listing); path "-": standard output
int write_node_labels(const std::string& path, const uint8_t* blob, const int64_t* offs, const int32_t* labels,
                      uint64_t n);

}  // namespace g2n
