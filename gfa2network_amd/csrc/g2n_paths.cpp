// g2n_paths.cpp — the reference's load_paths (gfa2network/analysis.py:164-177) on host threads: the
// P / O records of a GFA text as name -> step list.  A record is a line whose first field is exactly
// "P" or "O" with at least three fields (a shorter one is the parser's "Malformed" error, which the
// GPU build reports); its name is field 1, its steps field 2 cut at commas with one trailing '+' or
// '-' removed from each (parser.py:229-247, 343-361: an empty field is one empty step).  A repeated
// name keeps its first position and takes the last record's steps (a dict assignment).  The text is
// cut at line starts into one range per thread; the ranges' records are merged in stream order.
// Also reported: the first record, in stream order, whose name or — after the name — whose step
// holds a byte >= 0x80 (what .decode("ascii") raises on), as its 0-based line and those bytes.
#include <cstring>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "g2n_internal.h"

namespace g2n {

namespace {

struct PathRec {
  const uint8_t* name;
  size_t name_len;
  const uint8_t* steps;
  size_t steps_len;
};

struct RangeOut {
  std::vector<PathRec> recs;
  int64_t lines = 0;
  int64_t bad_line = -1;  // within the range
  const uint8_t* bad = nullptr;
  size_t bad_len = 0;
};

inline bool has_high(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (p[i] & 0x80u) return true;
  return false;
}

// one step of a step field [p, e): its bytes without one trailing orientation sign; *next = the
// byte after its comma (or e + 1 after the last step)
inline void next_step(const uint8_t* p, const uint8_t* e, const uint8_t** s_end, const uint8_t** next) {
  const auto* c = (const uint8_t*)std::memchr(p, ',', (size_t)(e - p));
  const uint8_t* se = c ? c : e;
  *next = se + 1;
  if (se > p && (se[-1] == '+' || se[-1] == '-')) se--;
  *s_end = se;
}

void scan_range(const uint8_t* b, const uint8_t* e, RangeOut& out) {
  for (const uint8_t* p = b; p < e;) {
    const auto* nl = (const uint8_t*)std::memchr(p, '\n', (size_t)(e - p));
    const uint8_t* le = nl ? nl : e;  // the line without its newline
    if (le - p >= 2 && (p[0] == 'P' || p[0] == 'O') && p[1] == '\t') {
      const uint8_t* name = p + 2;
      const auto* t2 = (const uint8_t*)std::memchr(name, '\t', (size_t)(le - name));
      if (t2) {  // (fewer than three fields: the parser's error, not a path)
        const uint8_t* steps = t2 + 1;
        const auto* t3 = (const uint8_t*)std::memchr(steps, '\t', (size_t)(le - steps));
        const uint8_t* se = t3 ? t3 : le;
        out.recs.push_back(PathRec{name, (size_t)(t2 - name), steps, (size_t)(se - steps)});
        if (out.bad_line < 0 && has_high(name, (size_t)(se - name))) {
          out.bad_line = out.lines;
          if (has_high(name, (size_t)(t2 - name))) {
            out.bad = name;
            out.bad_len = (size_t)(t2 - name);
          } else {
            for (const uint8_t* s = steps; s <= se;) {
              const uint8_t *s_end, *next;
              next_step(s, se, &s_end, &next);
              if (has_high(s, (size_t)(s_end - s))) {
                out.bad = s;
                out.bad_len = (size_t)(s_end - s);
                break;
              }
              s = next;
            }
            if (!out.bad) out.bad_line = -1;  // (cannot be: a high byte is in some step)
          }
        }
      }
    }
    out.lines++;
    p = nl ? nl + 1 : e;
  }
}

}  // namespace

void scan_paths(const uint8_t* text, size_t len, g2n_paths* out) {
  int T = host_threads();
  if (len < ((size_t)1 << 20) || T < 1) T = 1;
  std::vector<size_t> cut(T + 1, len);
  cut[0] = 0;
  for (int t = 1; t < T; t++) {  // range t starts after the first newline at or past its even share
    size_t at = std::max(cut[t - 1], len / (size_t)T * (size_t)t);
    const auto* nl = at < len ? (const uint8_t*)std::memchr(text + at, '\n', len - at) : nullptr;
    cut[t] = nl ? (size_t)(nl - text) + 1 : len;
  }
  std::vector<RangeOut> parts(T);
  parallel_for((size_t)T, T, [&](size_t t) { scan_range(text + cut[t], text + cut[t + 1], parts[t]); });
  // ---- merge in stream order: first position, last steps
  std::unordered_map<std::string_view, size_t> index;
  std::vector<PathRec> paths;
  int64_t line0 = 0;
  for (const RangeOut& r : parts) {
    if (out->bad_line < 0 && r.bad_line >= 0) {
      out->bad_line = line0 + r.bad_line;
      out->bad_bytes.assign(r.bad, r.bad + r.bad_len);
    }
    line0 += r.lines;
    for (const PathRec& rec : r.recs) {
      const std::string_view key((const char*)rec.name, rec.name_len);
      auto it = index.find(key);
      if (it == index.end()) {
        index.emplace(key, paths.size());
        paths.push_back(rec);
      } else {
        paths[it->second].steps = rec.steps;
        paths[it->second].steps_len = rec.steps_len;
      }
    }
  }
  out->name_offs.assign(1, 0);
  out->step_offs.assign(1, 0);
  out->path_ptr.assign(1, 0);
  for (const PathRec& rec : paths) {
    out->names.insert(out->names.end(), rec.name, rec.name + rec.name_len);
    out->name_offs.push_back((int64_t)out->names.size());
    const uint8_t* se = rec.steps + rec.steps_len;
    for (const uint8_t* s = rec.steps; s <= se;) {
      const uint8_t *s_end, *next;
      next_step(s, se, &s_end, &next);
      out->steps.insert(out->steps.end(), s, s_end);
      out->step_offs.push_back((int64_t)out->steps.size());
      s = next;
    }
    out->path_ptr.push_back((int64_t)out->step_offs.size() - 1);
  }
}

}  // namespace g2n

extern "C" {

void g2n_paths_get(const g2n_paths* p, const uint8_t** names, const int64_t** name_offs, uint64_t* n_paths,
                   const uint8_t** steps, const int64_t** step_offs, const int64_t** path_ptr, int64_t* bad_line,
                   const uint8_t** bad_bytes, uint64_t* bad_len) {
  if (names) *names = p->names.data();
  if (name_offs) *name_offs = p->name_offs.data();
  if (n_paths) *n_paths = p->name_offs.size() - 1;
  if (steps) *steps = p->steps.data();
  if (step_offs) *step_offs = p->step_offs.data();
  if (path_ptr) *path_ptr = p->path_ptr.data();
  if (bad_line) *bad_line = p->bad_line;
  if (bad_bytes) *bad_bytes = p->bad_bytes.data();
  if (bad_len) *bad_len = p->bad_bytes.size();
}

void g2n_paths_free(g2n_paths* p) { delete p; }

}  // extern "C"
