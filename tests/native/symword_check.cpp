// Host check of g2n_symword.h (stand-alone, built under ASan + UBSan by tests/test_symword.py): a pair
// word cut to 16 bits — what the last partition pass writes — gives the finish the same two rows as
// the 32-bit word, for every bucket size and every pass-1 word layout.
// Prints "symword OK <cases>" and exits 0, or prints the first failure and exits 1.
#include <stdint.h>
#include <stdio.h>

#include "../../gfa2network_amd/csrc/g2n_symword.h"

using namespace g2n;

int main() {
  unsigned long long cases = 0;
  for (uint32_t low = 1; low <= kSymLowMax; low++) {
    const uint32_t nb = 1u << low;
    uint64_t x = 0x9E3779B97F4A7C15ull + low;
    // pass 1 lays (a mod 2^shift1) << low | (b mod 2^low) into shift1 + low <= 26 bits (shift1 = low: the
    // only pass); pass 7 sorts by the bits from 2 low up and passes the word on
    for (uint32_t shift1 = low; shift1 + low <= 26; shift1++) {
      const uint32_t wmask = (uint32_t)((1ull << (shift1 + low)) - 1ull);
      for (int t = 0; t < 8192; t++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        uint32_t w = (uint32_t)x & wmask;
        if (t == 0) w = wmask;       // every bit set
        if (t == 1) w = 0;
        if (t == 2) w = wmask & ~0xFFFFu;  // only bits the cut drops
        if (t == 3) w = wmask & 0xFFFFu;
        const uint32_t bucket = (uint32_t)(x >> 40) & ((1u << (30 - low)) - 1u);  // rows < 2^30
        uint32_t a, b, a16, b16;
        sym_word_rows(w, bucket, low, &a, &b);
        sym_word_rows((uint32_t)(uint16_t)w, bucket, low, &a16, &b16);
        cases++;
        if (a != a16 || b != b16 || (a >> low) != bucket || (b >> low) != bucket ||
            (a & (nb - 1)) != ((w >> low) & (nb - 1)) || (b & (nb - 1)) != (w & (nb - 1)))
          return printf("pair word: w=%x low=%u shift1=%u bucket=%u\n", w, low, shift1, bucket), 1;
      }
    }
    // exhaustive over the 2 low bits the finish uses, under an arbitrary upper part
    for (uint32_t lo = 0; lo < (1u << (2 * low)); lo++) {
      const uint32_t w = lo | (0x2A5u << (2 * low));
      uint32_t a, b, a16, b16;
      sym_word_rows(w, 5, low, &a, &b);
      sym_word_rows((uint32_t)(uint16_t)w, 5, low, &a16, &b16);
      cases++;
      if (a != a16 || b != b16 || a != ((5u << low) | (lo >> low)) || b != ((5u << low) | (lo & (nb - 1))))
        return printf("pair word: w=%x low=%u\n", w, low), 1;
    }
  }
  printf("symword OK %llu\n", cases);
  return 0;
}
