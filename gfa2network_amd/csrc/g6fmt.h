// g6fmt.h — CPython's '%.6g' % v for every double, as host+device code.
//
// The reference's dense csv writer is np.savetxt(dest, A.toarray(), delimiter=",", fmt="%.6g")
// (gfa2network/utils.py:87-96), which formats each cell with Python's % operator: PyOS_double_to_string(v,
// 'g', 6, 0) — the value correctly rounded to 6 significant digits (half-even on the exact binary value,
// Python/dtoa.c mode 2), fixed notation for decimal exponents -4..5, otherwise d.ddddde+XX with at least two
// exponent digits; trailing zeros and a bare point removed; "inf", "-inf", "nan" (no sign), "-0".
//
// Restated here with exact integer arithmetic: v = m * 2^e, and for the decimal exponent d the integer
// floor(2 * v / 10^(d-5)) is computed in a fixed 896-bit integer (m times a power of five, shifted, or m
// shifted and divided by a power of five; the largest intermediate is 5^329 * 2 of the smallest subnormal,
// 766 bits, and 2^1024 / 10^303 * 2 before its division, 723 bits) together with a sticky flag for what the
// divisions dropped: its low bit and the flag decide the rounding, ties to even.  d starts from the binary
// exponent (floor(e2 * log10 2) in integers) and is corrected when the quotient has 5 or 7 digits.  Integers
// below 10^6 — every unweighted build's values — never reach the big integer.
//
// Everything is G2N_HD so tests/test_dense_format_host.py checks the host build (g2n_format_g6) against
// CPython's own '%.6g' on the CPU; the GPU kernel (g2n_dense.hip k_dn_fmt) includes the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define G2N_HD __host__ __device__
#else
#define G2N_HD
#endif

namespace g2n {

constexpr int kG6Words = 28;                // 896 bits
constexpr uint32_t kG6Pow5_13 = 1220703125u;  // 5^13, the largest power of five in 32 bits

struct G6Big {
  uint32_t w[kG6Words];
  int n;  // words in use (w[n - 1] != 0, or n == 0)
};

G2N_HD inline void g6_mul(G6Big& b, uint32_t f) {
  uint64_t carry = 0;
  for (int i = 0; i < b.n; i++) {
    const uint64_t t = (uint64_t)b.w[i] * f + carry;
    b.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  if (carry && b.n < kG6Words) b.w[b.n++] = (uint32_t)carry;
}

// b /= d; returns the remainder
G2N_HD inline uint32_t g6_div(G6Big& b, uint32_t d) {
  uint64_t rem = 0;
  for (int i = b.n - 1; i >= 0; i--) {
    const uint64_t t = (rem << 32) | b.w[i];
    b.w[i] = (uint32_t)(t / d);
    rem = t % d;
  }
  while (b.n && !b.w[b.n - 1]) b.n--;
  return (uint32_t)rem;
}

G2N_HD inline void g6_shl(G6Big& b, int bits) {
  const int ws = bits >> 5, bs = bits & 31;
  if (!b.n) return;
  int n = b.n + ws + 1;
  if (n > kG6Words) n = kG6Words;  // (never: the header's bound)
  for (int i = n - 1; i >= 0; i--) {
    const int s = i - ws;
    uint32_t v = 0;
    if (s >= 0 && s < b.n) v = b.w[s] << bs;
    if (bs && s - 1 >= 0 && s - 1 < b.n) v |= b.w[s - 1] >> (32 - bs);
    b.w[i] = v;
  }
  b.n = n;
  while (b.n && !b.w[b.n - 1]) b.n--;
}

// b >>= bits; returns whether a dropped bit was set
G2N_HD inline bool g6_shr(G6Big& b, int bits) {
  const int ws = bits >> 5, bs = bits & 31;
  bool sticky = false;
  for (int i = 0; i < ws && i < b.n; i++) sticky |= b.w[i] != 0;
  if (ws >= b.n) {
    b.n = 0;
    return sticky;
  }
  if (bs) sticky |= (b.w[ws] & ((1u << bs) - 1u)) != 0;
  const int n = b.n - ws;
  for (int i = 0; i < n; i++) {
    uint32_t v = b.w[i + ws] >> bs;
    if (bs && i + ws + 1 < b.n) v |= b.w[i + ws + 1] << (32 - bs);
    b.w[i] = v;
  }
  b.n = n;
  while (b.n && !b.w[b.n - 1]) b.n--;
  return sticky;
}

// floor(2 * m * 2^e / 10^s), capped at 2^32 - 1, and *sticky = whether anything was dropped
G2N_HD inline uint32_t g6_scaled(uint64_t m, int e, int s, bool* sticky) {
  G6Big b;
  b.w[0] = (uint32_t)m;
  b.w[1] = (uint32_t)(m >> 32);
  b.n = b.w[1] ? 2 : 1;
  bool st = false;
  int p5 = s < 0 ? -s : s;   // the power of five: a factor when s < 0, a divisor otherwise
  const int sh = e - s + 1;  // the power of two
  if (s < 0) {
    for (; p5 >= 13; p5 -= 13) g6_mul(b, kG6Pow5_13);
    uint32_t f = 1;
    for (; p5 > 0; p5--) f *= 5u;
    g6_mul(b, f);
    if (sh > 0) g6_shl(b, sh);
  } else {
    if (sh > 0) g6_shl(b, sh);
    for (; p5 >= 13; p5 -= 13) st |= g6_div(b, kG6Pow5_13) != 0;
    uint32_t f = 1;
    for (; p5 > 0; p5--) f *= 5u;
    if (f > 1) st |= g6_div(b, f) != 0;
  }
  if (sh < 0) st |= g6_shr(b, -sh);
  *sticky = st;
  if (b.n > 1) return 0xFFFFFFFFu;
  return b.n ? b.w[0] : 0u;
}

// the bytes of '%.6g' % v into out[0 .. length); out[15] = the length (at most 13), the bytes between zero
G2N_HD inline uint32_t g6_format(double v, uint8_t out[16]) {
  for (int i = 0; i < 16; i++) out[i] = 0;
  uint64_t bits;
  __builtin_memcpy(&bits, &v, 8);
  const bool neg = (bits >> 63) != 0;
  const uint32_t be = (uint32_t)(bits >> 52) & 0x7FFu;
  uint64_t frac = bits & ((1ull << 52) - 1);
  uint32_t o = 0;
  if (be == 0x7FF) {
    if (frac) {
      out[0] = 'n', out[1] = 'a', out[2] = 'n';
      out[15] = 3;
      return 3;
    }
    if (neg) out[o++] = '-';
    out[o++] = 'i', out[o++] = 'n', out[o++] = 'f';
    out[15] = (uint8_t)o;
    return o;
  }
  if (neg) out[o++] = '-';
  if (!be && !frac) {
    out[o++] = '0';
    out[15] = (uint8_t)o;
    return o;
  }
  const uint64_t m = be ? frac | (1ull << 52) : frac;
  const int e = be ? (int)be - 1075 : -1074;
  uint32_t N;  // the 6 digits
  int d;       // the decimal exponent of the first
  const int tz = __builtin_ctzll(m);
  if (e <= 0 && -e <= tz && (m >> -e) < 1000000ull) {  // an integer below 10^6: its digits
    N = (uint32_t)(m >> -e);
    d = 5;
    while (N < 100000u) N *= 10u, d--;
  } else {
    const int e2 = 63 - __builtin_clzll(m) + e;  // 2^e2 <= |v| < 2^(e2 + 1)
    d = (e2 * 1233) >> 12;                       // floor(e2 * log10(2)), or one less near a power of ten
    uint32_t q2;
    bool sticky;
    for (;;) {
      q2 = g6_scaled(m, e, d - 5, &sticky);
      if ((q2 >> 1) >= 1000000u) d++;
      else if ((q2 >> 1) < 100000u) d--;
      else break;
    }
    N = q2 >> 1;
    if ((q2 & 1u) && (sticky || (N & 1u))) N++;
    if (N == 1000000u) N = 100000u, d++;
  }
  uint8_t dig[6];
  for (int i = 5; i >= 0; i--) dig[i] = (uint8_t)('0' + N % 10u), N /= 10u;
  int nd = 6;
  while (nd > 1 && dig[nd - 1] == '0') nd--;
  if (d >= -4 && d < 6) {
    if (d < 0) {
      out[o++] = '0', out[o++] = '.';
      for (int i = -1; i > d; i--) out[o++] = '0';
      for (int i = 0; i < nd; i++) out[o++] = dig[i];
    } else {
      for (int i = 0; i <= d; i++) out[o++] = i < nd ? dig[i] : (uint8_t)'0';
      if (nd > d + 1) {
        out[o++] = '.';
        for (int i = d + 1; i < nd; i++) out[o++] = dig[i];
      }
    }
  } else {
    out[o++] = dig[0];
    if (nd > 1) {
      out[o++] = '.';
      for (int i = 1; i < nd; i++) out[o++] = dig[i];
    }
    out[o++] = 'e';
    out[o++] = d < 0 ? '-' : '+';
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    if (a >= 100u) out[o++] = (uint8_t)('0' + a / 100u);
    out[o++] = (uint8_t)('0' + a / 10u % 10u);
    out[o++] = (uint8_t)('0' + a % 10u);
  }
  out[15] = (uint8_t)o;
  return o;
}

}  // namespace g2n
