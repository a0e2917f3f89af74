// decfmt.h — the decimal digit arithmetic of a decimal-id build's names and edge-list text, as host+device code.
//
// A decimal-id build (S line k names "k+1", S lines first) never reads a key's bytes again: node id's key is
// str(k + 1) (bidirected: id = 2k + [ori == '-'], key str(k + 1) + ":+" / ":-"), so the names blob and its
// offsets (g2n_kernels.hip k_names_dec) and every line of export --format edge-list (k_edge_dec_sum,
// k_edge_dec_text) are arithmetic on the ids.  What that arithmetic consists of is here:
//
//   dec_digits / dec_digits_upto / dec_name_off   a key's length and its offset in the names blob, closed form;
//   dec_ndig                                      a key's digit count from clz and one table read;
//   dec4_ascii                                    four digits at a time by SWAR multiply-shift;
//   dec_key_put                                   a key's bytes: up to 8 digits in one shifted 64-bit word, the
//                                                 leading 1-2 digits of a 9-10 digit key before it.
//
// Everything is G2N_HD so tests/test_host_headers.py (tests/native/hostcheck.cpp) checks the host build
// against snprintf over every value a kernel test cannot afford; the kernels include the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define G2N_HD __host__ __device__
#else
#define G2N_HD
#endif

namespace g2n {

G2N_HD inline uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  for (uint64_t p = 10; v >= p && d < 20; p *= 10) d++;
  return d;
}
G2N_HD inline uint64_t dec_digits_upto(uint64_t v) {  // sum of dec_digits(k), k = 1..v
  uint64_t s = 0, lo = 1;
  for (uint32_t d = 1; lo <= v && d < 20; d++, lo *= 10) {
    const uint64_t hi = lo * 10 - 1, top = v < hi ? v : hi;
    s += (top - lo + 1) * d;
  }
  return s;
}
G2N_HD inline uint64_t dec_name_off(uint64_t id, int bidir) {  // offset of node id's key
  if (!bidir) return dec_digits_upto(id);
  const uint64_t k = id >> 1;
  return 2 * (dec_digits_upto(k) + 2 * k) + ((id & 1) ? dec_digits(k + 1) + 2 : 0);
}

// The digit work is VALU and sets the render's pace: a key's digit count is clz-based (one LDS table read, no
// compare chain), its digits come four at a time by SWAR (a 4-digit value split into 2-digit then 1-digit byte
// lanes by multiply-shift: x / 100 = (x * 5243) >> 19 for x < 10^4, x / 10 = (x * 103) >> 10 for x < 100; no
// carry crosses a lane).
G2N_HD inline uint32_t dec4_ascii(uint32_t y) {  // y < 10^4: its 4 digits, most significant in byte 0
  const uint32_t h = (y * 5243u) >> 19;
  uint32_t z = h | ((y - h * 100u) << 16);
  const uint32_t t = ((z * 103u) >> 10) & 0x000F000Fu;
  z = t | ((z - t * 10u) << 8);
  return z | 0x30303030u;
}
#if defined(__HIP_DEVICE_COMPILE__)
G2N_HD inline uint32_t dec_clz(uint32_t v) { return (uint32_t)__clz(v); }
#else
G2N_HD inline uint32_t dec_clz(uint32_t v) { return (uint32_t)__builtin_clz(v); }
#endif
G2N_HD inline uint32_t dec_ndig(uint32_t v, const uint32_t* p10 /* (the kernels: LDS) 10^0 .. 10^9 */) {  // v >= 1
  const uint32_t t = ((32u - dec_clz(v)) * 1233u) >> 12;  // log10(2^bits), 0..9
  return t + (v >= p10[t] ? 1u : 0u);
}
// the key of value v (n digits) at d, plus ":+" / ":-" when bidirected; returns the byte after it.
// (Writing every key as 8 zero-padded bytes back to front, without per-byte predicates, measured the
// same 1.19 ms on C4: the render runs at ~4.3 TB/s of ids read + text written.)
G2N_HD inline uint8_t* dec_key_put(uint8_t* d, uint32_t v, uint32_t n, int bidir, uint32_t id) {
  if (n > 8) {  // the leading 1-2 digits, then the low 8
    const uint32_t hi = v / 100000000u;
    v -= hi * 100000000u;
    if (hi > 9) *d++ = (uint8_t)('0' + hi / 10u);
    *d++ = (uint8_t)('0' + hi % 10u);
    n = 8;
  }
  const uint32_t a = v / 10000u;
  const uint64_t w = (((uint64_t)dec4_ascii(v - a * 10000u) << 32) | dec4_ascii(a)) >> (8u * (8u - n));
  for (uint32_t j = 0; j < n; j++) d[j] = (uint8_t)(w >> (8u * j));
  d += n;
  if (bidir) {
    d[0] = ':';
    d[1] = (id & 1u) ? '-' : '+';
    d += 2;
  }
  return d;
}

}  // namespace g2n
