// g2n_write_node_labels (gfa2network_amd/csrc/g2n_writers.cpp: the components CLI's
// "name\tlabel\n" listing) under AddressSanitizer and UndefinedBehaviorSanitizer: built with g++ from
// the library's host sources plus this driver by tests/test_components_host.py (CPU only; the GPU
// paths of those files are linked but never called).  argv[1]: a directory to write into.  Cases:
// no node, empty names, a null blob, names that are not UTF-8 with and without the check, the
// largest and a negative label, more nodes than one range, a path that cannot be opened.  Prints
// "OK" and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../gfa2network_amd/csrc/g2n_internal.h"

namespace g2n {
static thread_local std::string t_err;
void set_last_error(const std::string& msg) { t_err = msg; }  // g2n_host.cpp's, not linked here
int guarded(const std::function<int()>& f) {                  // g2n_host.cpp's, not linked here
  try {
    return f();
  } catch (const Failure& e) {
    set_last_error(e.what());
    return e.status;
  }
}
}  // namespace g2n

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                                  \
    }                                                              \
  } while (0)

static std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return "<unreadable>";
  char buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, k);
  fclose(f);
  return s;
}

struct Names {
  std::vector<uint8_t> blob;
  std::vector<int64_t> offs{0};
  void add(const std::string& s) {
    blob.insert(blob.end(), s.begin(), s.end());
    offs.push_back((int64_t)blob.size());
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string out = std::string(argv[1]) + "/labels.tsv";
  int64_t bad = 7;
  // no node: an empty file, nothing read
  CHECK(g2n_write_node_labels(out.c_str(), nullptr, nullptr, nullptr, 0, 1, &bad) == G2N_OK && bad == -1);
  CHECK(slurp(out).empty());
  // empty names only, the blob null
  {
    const std::vector<int64_t> offs{0, 0, 0, 0};
    const std::vector<int32_t> lab{0, 1, 0};
    CHECK(g2n_write_node_labels(out.c_str(), nullptr, offs.data(), lab.data(), 3, 1, &bad) == G2N_OK && bad == -1);
    CHECK(slurp(out) == "\t0\n\t1\n\t0\n");
  }
  // mixed names: an empty one, valid two- and four-byte UTF-8, the largest and a negative label
  {
    Names nm;
    for (const char* s : {"s1", "", "\xc3\xa9t\xc3\xa9", "\xf0\x9f\x98\x80", "tail:+"}) nm.add(s);
    const std::vector<int32_t> lab{0, 2147483647, 1, -2147483647 - 1, 10};
    CHECK(g2n_write_node_labels(out.c_str(), nm.blob.data(), nm.offs.data(), lab.data(), 5, 1, &bad) == G2N_OK);
    CHECK(bad == -1);
    CHECK(slurp(out) ==
          "s1\t0\n\t2147483647\n\xc3\xa9t\xc3\xa9\t1\n\xf0\x9f\x98\x80\t-2147483648\ntail:+\t10\n");
    CHECK(g2n_write_node_labels(out.c_str(), nm.blob.data(), nm.offs.data(), lab.data(), 5, 0, nullptr) == G2N_OK);
  }
  // names that are not UTF-8 (a lone continuation byte, a truncated sequence at the blob's end)
  {
    Names nm;
    for (const char* s : {"ok", "also ok", "\x80", "after", "\xe2\x82"}) nm.add(s);
    const std::vector<int32_t> lab{3, 3, 4, 5, 6};
    CHECK(g2n_write_node_labels(out.c_str(), nm.blob.data(), nm.offs.data(), lab.data(), 5, 1, &bad) == G2N_OK);
    CHECK(bad == 2 && slurp(out) == "ok\t3\nalso ok\t3\n");
    CHECK(g2n_write_node_labels(out.c_str(), nm.blob.data(), nm.offs.data(), lab.data(), 5, 0, &bad) == G2N_OK);
    CHECK(bad == -1 && slurp(out) == "ok\t3\nalso ok\t3\n\x80\t4\nafter\t5\n\xe2\x82\t6\n");
    // the first name bad: nothing is written
    Names first;
    first.add("\xff");
    first.add("x");
    CHECK(g2n_write_node_labels(out.c_str(), first.blob.data(), first.offs.data(), lab.data(), 2, 1, &bad) == G2N_OK);
    CHECK(bad == 0 && slurp(out).empty());
  }
  // more nodes than one range, several rounds of ranges: every line where it belongs
  {
    const uint64_t n = 3u * (1u << 18) * 4u + 12345u;
    Names nm;
    std::vector<int32_t> lab(n);
    std::string want;
    for (uint64_t i = 0; i < n; i++) {
      const std::string s = i % 7 ? "n" + std::to_string(i) : std::string();
      nm.add(s);
      lab[i] = (int32_t)(i % 1000003u);
      want += s + "\t" + std::to_string(lab[i]) + "\n";
    }
    CHECK(g2n_write_node_labels(out.c_str(), nm.blob.data(), nm.offs.data(), lab.data(), n, 1, &bad) == G2N_OK);
    CHECK(bad == -1 && slurp(out) == want);
  }
  // arguments and a path that cannot be opened
  {
    const std::vector<int64_t> offs{0, 0};
    const int32_t lab = 0;
    CHECK(g2n_write_node_labels(nullptr, nullptr, offs.data(), &lab, 1, 0, nullptr) == G2N_E_ARG);
    CHECK(g2n_write_node_labels(out.c_str(), nullptr, nullptr, &lab, 1, 0, nullptr) == G2N_E_ARG);
    CHECK(g2n_write_node_labels(out.c_str(), nullptr, offs.data(), nullptr, 1, 0, nullptr) == G2N_E_ARG);
    const std::string nowhere = std::string(argv[1]) + "/no/such/dir/labels.tsv";
    CHECK(g2n_write_node_labels(nowhere.c_str(), nullptr, offs.data(), &lab, 1, 0, nullptr) == G2N_E_IO);
  }
  if (failures) return 1;
  printf("OK\n");
  return 0;
}
