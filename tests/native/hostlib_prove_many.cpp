// Host entry point for the digits of the many-pair prover's walk (kernels.hip k_prove_points_micro),
// part of the same CPU test library as hostlib.cpp: a scalar reduced mod l as prove_scalar reduces
// it, then sc_recode_radix16 -- digits 0..31 go on B, digits 32..63 on 2^128 B.
// With CPZT_PROVE_MANY_MAIN the file is a program of its own (for a sanitizer build): it recodes
// the edge scalars of tests/prove_many_cases.py and pseudo-random ones and checks the digits' range,
// their value, the values of the two halves (digits 0..31 and 32..63, the carry between them) and
// the top digit.
#include <cstring>

#include "scalar25519.h"

using namespace cpz;

extern "C" {

// `scalar`: 32 little-endian bytes, any value.  reduced: the value mod l (32 bytes); digits: the 64
// signed radix-16 digits of it, digit i = nibble i % 8 of word i / 8 as the kernel unpacks it.
void cpzt_prove_many_digits(int8_t digits[64], uint8_t reduced[32], const uint8_t scalar[32]) {
  uint32_t wide[16];
  std::memset(wide, 0, sizeof(wide));
  std::memcpy(wide, scalar, 32);
  const sc v = sc_reduce_wide(wide);
  std::memcpy(reduced, v.w, 32);
  uint32_t d[8];
  sc_recode_radix16(d, v.w);
  for (int i = 0; i < 64; i++) digits[i] = (int8_t)(((int32_t)(d[i >> 3] << (28 - 4 * (i & 7)))) >> 28);
}

}  // extern "C"

#ifdef CPZT_PROVE_MANY_MAIN
#include <cstdio>

namespace {

int g_checked = 0, g_carried = 0;  // scalars checked; those with a carry from digit 31 into digit 32

// Whether sum d_i 16^i over the `count` digits at dg equals the 256-bit little-endian value `want`:
// the signed digits are carried into 80 nibbles, of which the low 64 must be want's and the rest
// zero (a negative sum leaves a carry and fails).
bool digits_value_is(const int8_t* dg, int count, const uint8_t want[32]) {
  int64_t acc[80] = {0};  // nibble accumulators, then carried
  for (int i = 0; i < count; i++) acc[i] = dg[i];
  int64_t carry = 0;
  uint8_t nib[80];
  for (int i = 0; i < 80; i++) {
    const int64_t t = acc[i] + carry;
    nib[i] = (uint8_t)(t & 15);
    carry = (t - nib[i]) / 16;
  }
  if (carry != 0) return false;
  for (int i = 0; i < 64; i++)
    if (nib[i] != ((want[i >> 1] >> (4 * (i & 1))) & 15)) return false;
  for (int i = 64; i < 80; i++)
    if (nib[i] != 0) return false;
  return true;
}

int check(const uint8_t scalar[32], const char* what) {
  int8_t dg[64];
  uint8_t red[32];
  cpzt_prove_many_digits(dg, red, scalar);
  for (int i = 0; i < 64; i++)
    if (dg[i] < -8 || dg[i] > 7) return std::printf("%s: digit %d = %d\n", what, i, dg[i]), 1;
  if (dg[63] < 0 || dg[63] > 2) return std::printf("%s: top digit %d\n", what, dg[63]), 1;
  if (!digits_value_is(dg, 64, red)) return std::printf("%s: the digits' value is not the scalar\n", what), 1;
  // the two halves the walk puts on B and on 2^128 B: digits 32..63 are (v >> 128) plus the carry out
  // of digit 31, which is the carry of (v mod 2^128) + 0x88..88 (8 added to every nibble, carries
  // passed on); digits 0..31 then hold v mod 2^128 less that carry times 2^128
  unsigned carry = 0;
  for (int i = 0; i < 16; i++) carry = (red[i] + 0x88u + carry) >> 8;
  uint8_t hi[32] = {0};
  unsigned c = carry;
  for (int i = 0; i < 16; i++) {
    const unsigned t = red[16 + i] + c;
    hi[i] = (uint8_t)t;
    c = t >> 8;
  }
  hi[16] = (uint8_t)c;
  if (!digits_value_is(dg + 32, 32, hi)) return std::printf("%s: digits 32..63 lost the carry of digit 31\n", what), 1;
  if (!carry) {  // no carry: the low digits are v mod 2^128 as they stand (with one their sum is negative)
    uint8_t lo[32] = {0};
    std::memcpy(lo, red, 16);
    if (!digits_value_is(dg, 32, lo)) return std::printf("%s: digits 0..31 are not v mod 2^128\n", what), 1;
  }
  g_carried += (int)carry;
  g_checked++;
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  uint8_t s[32];
  const int small[] = {0, 1, 7, 8, 9};
  for (int v : small) {
    std::memset(s, 0, 32);
    s[0] = (uint8_t)v;
    bad += check(s, "small");
  }
  std::memset(s, 0x77, 32);
  bad += check(s, "0x77..77");
  std::memset(s, 0x88, 32);
  bad += check(s, "0x88..88");
  std::memset(s, 0xff, 32);
  bad += check(s, "2^256-1");
  std::memset(s, 0, 32);
  std::memset(s, 0xff, 16);
  bad += check(s, "2^128-1");
  std::memset(s, 0, 32);
  s[16] = 1;
  bad += check(s, "2^128");
  s[0] = 8;
  bad += check(s, "2^128+8");
  std::memset(s, 0, 32);
  s[15] = 0x10;
  bad += check(s, "2^124");
  std::memset(s, 0, 32);
  s[31] = 0x10;
  bad += check(s, "2^252");
  const uint8_t l_minus_1[32] = {0xec, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
  bad += check(l_minus_1, "l-1");
  uint64_t x = 0x9e3779b97f4a7c15ull;  // xorshift64: any 32 bytes, the call reduces them
  for (int t = 0; t < 2000; t++) {
    for (int i = 0; i < 32; i++) {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      s[i] = (uint8_t)(x >> 32);
    }
    bad += check(s, "random");
  }
  if (bad) return std::printf("FAILED: %d\n", bad), 1;
  if (g_carried == 0 || g_carried == g_checked) return std::printf("FAILED: one side of the carry was never seen\n"), 1;
  std::printf("ok: %d scalars, %d with a carry from digit 31 into digit 32\n", g_checked, g_carried);
  return 0;
}
#endif
