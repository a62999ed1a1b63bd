// Host entry points for the mixed-pair prover's table walk (scalarmul.h pair_table_mul), part of
// the same CPU test library as hostlib.cpp: the walk runs with the limb-bound assertions on, over
// tables built here with the library's own small_mul / p3_to_niels and the level doublings.
#include <cstring>

#include "verify.h"

using namespace cpz;

extern "C" {

// Bytes of one pair's tables: [8 levels][g, h][128 entries] of ge_niels, the GenSet::tab layout.
int cpzt_pair_tables_bytes(void) { return (int)(2 * 8 * kNielsEntries * sizeof(ge_niels)); }
int cpzt_niels_bytes(void) { return (int)sizeof(ge_niels); }

// Fills `tab` (cpzt_pair_tables_bytes bytes) for the encodings g and h: part q's level,
// kNielsLevelOfPart[q], holds the multiples 1..128 of 2^(32 q) B.  Returns 0 when a point does not
// decode.
int cpzt_pair_tables(uint8_t* tab, const uint8_t* g, const uint8_t* h) {
  ge_niels* t = reinterpret_cast<ge_niels*>(tab);
  std::memset(tab, 0, (size_t)cpzt_pair_tables_bytes());
  for (int e = 0; e < 2; e++) {
    uint32_t w[8];
    std::memcpy(w, e ? h : g, 32);
    ge_p3 B;
    if (!ristretto_decode(B, w)) return 0;
    for (int q = 0; q < 8; q++) {
      ge_niels* dst = t + (2 * kNielsLevelOfPart[q] + e) * kNielsEntries;
      for (int k = 1; k <= kNielsEntries; k++) dst[k - 1] = p3_to_niels(small_mul(B, k));
      for (int d = 0; d < 32; d++) B = p1p1_to_p3(p3_dbl(B));
    }
  }
  return 1;
}

// What k_prove_points_pairs does with one scalar: `scalar` (32 little-endian bytes, any value)
// reduced mod l as prove_scalar reduces it, recoded by sc_recode_radix256, walked over `tab`;
// enc([d] g) and enc([d] h) to out_g / out_h, the 32 signed digits to digits.
void cpzt_pair_table_mul(uint8_t* out_g, uint8_t* out_h, int8_t* digits, const uint8_t* tab, const uint8_t* scalar) {
  uint32_t wide[16];
  std::memset(wide, 0, sizeof(wide));
  std::memcpy(wide, scalar, 32);
  const sc v = sc_reduce_wide(wide);
  uint32_t d[8];
  sc_recode_radix256(d, v.w);
  for (int j = 0; j < 32; j++) digits[j] = (int8_t)((d[j >> 2] >> (8 * (j & 3))) & 255u);
  ge_p3 G, H;
  pair_table_mul(G, H, reinterpret_cast<const ge_niels*>(tab), d);
  uint32_t o[8];
  ristretto_encode(o, G);
  std::memcpy(out_g, o, 32);
  ristretto_encode(o, H);
  std::memcpy(out_h, o, 32);
}

}  // extern "C"
