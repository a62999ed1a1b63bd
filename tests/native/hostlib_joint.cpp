// Host entry points for the per-proof path's joint table (scalar25519.h sc_recode_radix4_half,
// scalarmul.h build_joint_table / straus_half_joint), part of the same CPU test library as
// hostlib.cpp: the exact device code, with the limb-bound assertions, against the Python oracle.
#include <cstring>

#include "verify.h"

using namespace cpz;

namespace {

bool decode_from(ge_p3& P, const uint8_t* enc) {
  uint32_t w[8];
  std::memcpy(w, enc, 32);
  return ristretto_decode(P, w);
}

void encode_to(uint8_t* out, const ge_p3& P) {
  uint32_t o[8];
  ristretto_encode(o, P);
  std::memcpy(out, o, 32);
}

// Host stand-in for the device comb of one base: entry (k, j) = j * 2^(16 k) * B in affine
// Niels form, computed on demand.
struct JointHostComb {
  ge_p3 q[kCombWindows];
  void build(ge_p3 B) {
    for (int k = 0; k < kCombWindows; k++) {
      q[k] = B;
      for (int d = 0; d < 16; d++) B = p1p1_to_p3(p3_dbl(B));
    }
  }
  ge_niels lookup(int k, int digit) const {
    const int mag = digit < 0 ? -digit : digit;
    ge_niels r = ge_niels_identity();
    if (mag != 0) {
      ge_p3 acc = q[k];
      for (int bit = 30 - __builtin_clz((unsigned)mag); bit >= 0; bit--) {
        acc = p1p1_to_p3(p3_dbl(acc));
        if ((mag >> bit) & 1) acc = ge_add(acc, q[k]);
      }
      r = p3_to_niels(acc);
    }
    return ge_niels_cneg(r, digit < 0);
  }
};

}  // namespace

extern "C" {

// The packed radix-4 digits (4 words) of a 128-bit value below 3 * 2^125 (aborts above it).
void cpzt_recode_radix4(uint32_t out[4], const uint32_t in[4]) { sc_recode_radix4_half(out, in); }

// Window i (0..63) of the recoded pair (ud, vd) as the Straus loop reads it: the table slot and
// whether the entry is negated.
void cpzt_joint_window(const uint32_t ud[4], const uint32_t vd[4], int i, int* slot, int* neg) {
  const int s = i == 63 ? joint_top_window(ud[3], vd[3]) : joint_window(ud[i / 16], vd[i / 16], i % 16);
  *slot = s < 0 ? -s : s;
  *neg = s < 0;
}

// The joint table of two decodable points: the encodings of its 13 entries (through the
// completed form the Straus loop starts from), and per entry whether T2d is 2 d X Y / Z.
// Returns the number of entries, or -1 when a point does not decode.
int cpzt_joint_table(uint8_t* out, int* t2d_ok, const uint8_t* y, const uint8_t* r) {
  ge_p3 Y, R;
  if (!decode_from(Y, y) || !decode_from(R, r)) return -1;
  ge_cached tv[kJointSlots];
  build_joint_table(host_table(tv), Y, R);
  for (int e = 0; e < kJointSlots; e++) {
    const ge_p1p1 c = cached_to_p1p1(tv[e]);  // (2X, 2Y, 2Z, 2Z)
    encode_to(out + 32 * e, p1p1_to_p3(c));
    t2d_ok[e] = fe_equal(fe_mul(fe_mul(c.X, c.Y), FE_D()), fe_mul(c.Z, tv[e].T2d)) ? 1 : 0;
  }
  return kJointSlots;
}

// enc([s'] B + [u] Y + [v] R) by the per-proof path's loop: u, v 16 bytes each (< 3 * 2^125),
// sp 32 bytes (< 2^253).  Returns -1 when a point does not decode.
int cpzt_straus_joint(uint8_t* out, const uint8_t* base, const uint8_t* y, const uint8_t* r, const uint8_t* u,
                      const uint8_t* v, const uint8_t* sp) {
  ge_p3 B, Y, R;
  if (!decode_from(B, base) || !decode_from(Y, y) || !decode_from(R, r)) return -1;
  JointHostComb comb;
  comb.build(B);
  uint32_t uw[4], vw[4], sw[8], dig[16];
  std::memcpy(uw, u, 16);
  std::memcpy(vw, v, 16);
  std::memcpy(sw, sp, 32);
  sc_recode_radix4_half(dig, uw);
  sc_recode_radix4_half(dig + 4, vw);
  sc_recode_radix65536(dig + 8, sw);
  ge_cached tv[kJointSlots];
  build_joint_table(host_table(tv), Y, R);
  const DigitRef ud = host_digits(dig), vd = host_digits(dig + 4), sd = host_digits(dig + 8);
  encode_to(out, p1p1_to_p3(straus_half_joint(host_table(tv), comb, ud, vd, sd)));
  return 0;
}

}  // extern "C"
