// g2n_symword.h — the pair word of the bucket partition (g2n_sym.hip), as the finish reads it.
// Host and device share the definition (tests/native/symword_check.cpp checks the 16-bit cut).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define G2N_HD __host__ __device__
#else
#define G2N_HD
#endif

namespace g2n {

// A finish bucket holds 2^low <= 2^kSymLowMax rows: 8 bits name a row inside it, and the last
// partition pass writes its pair words 16 bits wide.
constexpr uint32_t kSymLowMax = 8;

// A pair word of bucket `bucket` (rows a and b both inside it): a's bits below `low` at bit `low`, b's
// at bit 0.  Whatever lies from bit 2 low up — a's bits below pass 1's digit, which pass 7 has spent
// as its own digit — is ignored, so the low 16 bits of the word give the same rows.  Returns the two
// rows (relative to the slice's row base).
G2N_HD inline void sym_word_rows(uint32_t w, uint32_t bucket, uint32_t low, uint32_t* a, uint32_t* b) {
  const uint32_t rmask = (1u << low) - 1u, hi = bucket << low;
  *a = hi | ((w >> low) & rmask);
  *b = hi | (w & rmask);
}

}  // namespace g2n
