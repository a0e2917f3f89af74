// Host build of the product's host+device headers (pylit.h, stl_sort.h, decfmt.h) so the CPU test
// suite can fuzz them against CPython's int()/float(), libstdc++'s std::sort and snprintf.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gfa2network_amd/csrc/decfmt.h"
#include "../../gfa2network_amd/csrc/pylit.h"
#include "../../gfa2network_amd/csrc/stl_sort.h"

extern "C" {

int hc_py_float(const uint8_t* p, int64_t n, double* out) {
  if (!g2n::utf8_valid(p, (uint64_t)n)) return 0;
  static thread_local g2n::Decimal dec;
  uint8_t tmp[g2n::DEC_TMP];
  return g2n::py_float_literal(p, (uint64_t)n, true, out, &dec, tmp) ? 1 : 0;
}

// 0 invalid, 1 ok (*out = float(int(s))), 2 valid int whose float() overflows
int hc_py_int(const uint8_t* p, int64_t n, int transform, double* out) {
  if (transform && !g2n::utf8_valid(p, (uint64_t)n)) return 0;
  static thread_local g2n::Decimal dec;
  uint8_t tmp[g2n::DEC_TMP];
  if (!g2n::py_int_literal(p, (uint64_t)n, transform != 0, &dec)) return 0;
  return g2n::py_int_to_f64(&dec, out, tmp) ? 1 : 2;
}

int hc_fast_int(const uint8_t* p, int64_t n, double* out) { return g2n::fast_int(p, (uint64_t)n, out) ? 1 : 0; }
int hc_fast_float(const uint8_t* p, int64_t n, double* out) { return g2n::fast_float(p, (uint64_t)n, out) ? 1 : 0; }
int hc_utf8_valid(const uint8_t* p, int64_t n) { return g2n::utf8_valid(p, (uint64_t)n) ? 1 : 0; }

// Sort (key, original position) pairs by key with std::sort and with the restatement;
// write both resulting position permutations.
void hc_sort_both(const int32_t* keys, int64_t n, int32_t* out_std, int32_t* out_emul) {
  std::vector<std::pair<int32_t, int32_t>> a((size_t)n);
  std::vector<g2n::KV<int32_t, int32_t>> b((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    a[i] = {keys[i], (int32_t)i};
    b[i] = {keys[i], (int32_t)i};
  }
  std::sort(a.begin(), a.end(), [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) {
    return x.first < y.first;
  });
  if (n) g2n::stl_sort(b.data(), b.data() + n);
  for (int64_t i = 0; i < n; i++) {
    out_std[i] = a[i].second;
    out_emul[i] = b[i].v;
  }
}

// decfmt.h against snprintf.  One value: its digit count by dec_ndig (the table as the kernels fill it) and by
// dec_digits, and its key by dec_key_put — plain and bidirected, both id parities — into a buffer of canary
// bytes: the bytes, the returned end and every byte around the key.
static bool dec_key_ok(uint32_t v) {
  static const uint32_t p10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
  char want[16];
  const uint32_t n = (uint32_t)snprintf(want, sizeof want, "%u", v);
  if (g2n::dec_ndig(v, p10) != n || g2n::dec_digits(v) != n) return false;
  for (int bidir = 0; bidir < 2; bidir++)
    for (uint32_t id = 0; id < 2; id++) {
      uint8_t buf[32];
      memset(buf, 0xAA, sizeof buf);
      const uint8_t* end = g2n::dec_key_put(buf + 8, v, n, bidir, 2u * (v - 1u) + id);
      const uint32_t len = n + (bidir ? 2u : 0u);
      if (end != buf + 8 + len || memcmp(buf + 8, want, n) != 0) return false;
      if (bidir && (buf[8 + n] != ':' || buf[8 + n + 1] != (id ? '-' : '+'))) return false;
      for (uint32_t j = 0; j < sizeof buf; j++)
        if ((j < 8 || j >= 8 + len) && buf[j] != 0xAA) return false;
    }
  return true;
}

// every v = lo, lo + step, ... <= hi (1 <= lo, hi <= 2^31): the first value that fails, or 0
uint64_t hc_dec_key_range(uint64_t lo, uint64_t hi, uint64_t step) {
  for (uint64_t v = lo; v <= hi; v += step)
    if (!dec_key_ok((uint32_t)v)) return v;
  return 0;
}

uint64_t hc_dec_key_list(const uint32_t* v, int64_t n) {
  for (int64_t i = 0; i < n; i++)
    if (!dec_key_ok(v[i])) return v[i];
  return 0;
}

uint64_t hc_dec_name_off(uint64_t id, int bidir) { return g2n::dec_name_off(id, bidir); }

// dec_name_off(id) for id = 0 .. n_ids against the running sum of the keys' lengths (snprintf; bidirected:
// node id's key is str(id / 2 + 1) + ":+" / ":-"): the first id that differs, or -1
int64_t hc_dec_name_off_run(uint64_t n_ids, int bidir) {
  uint64_t sum = 0;
  char tmp[24];
  for (uint64_t id = 0; id <= n_ids; id++) {
    if (g2n::dec_name_off(id, bidir) != sum) return (int64_t)id;
    sum += (uint64_t)snprintf(tmp, sizeof tmp, "%llu", (unsigned long long)((bidir ? id >> 1 : id) + 1)) + (bidir ? 2 : 0);
  }
  return -1;
}
}
