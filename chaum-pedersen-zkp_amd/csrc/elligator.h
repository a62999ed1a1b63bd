// The ristretto255 one-way map (RFC 9496 section 4.3.4) for gfx950.
//
// Replaces curve25519-dalek 4.1.3's RistrettoPoint::from_uniform_bytes and
// elligator_ristretto_flavor, which the reference reaches in generator_h()
// (src/primitives/ristretto.rs:86-91); the same steps as oracle/pyoracle.py's _elligator_map and
// ristretto_from_uniform_bytes.
//
// Each 32-byte half of the uniform input is read little-endian with bit 255 cleared
// (fe_fromwords).  The value is not reduced first: a value in [p, 2^255) is accepted and stands
// for its residue, as dalek's FieldElement::from_bytes takes it.
//
// was_square only ever selects (fe_select): both arms of the map are computed by every lane, and
// no branch goes round the square-root chain.
#pragma once
#include "ristretto.h"

namespace cpz {

// MAP(t) as a completed point ((X:Z), (Y:T)) = ((w0:w1), (w2:w3)); p1p1_to_p3 gives the
// extended point (w0 w3 : w2 w1 : w1 w3 : w0 w2) of the RFC.
CPZ_HD ge_p1p1 elligator_map(const fe& t) {
  const fe one = fe_one();
  const fe r = fe_mul(FE_SQRT_M1(), fe_sq(t));
  const fe u = fe_mul(fe_add(r, one), FE_ONE_MINUS_D_SQ());
  const fe v = fe_mul(fe_sub(fe_neg(one), fe_mul(r, FE_D())), fe_add(r, FE_D()));
  fe s;
  const bool was_square = fe_sqrt_ratio_m1(s, u, v);
  const fe s_prime = fe_neg(fe_abs(fe_mul(s, t)));
  s = fe_select(s_prime, s, was_square);
  const fe c = fe_select(r, fe_neg(one), was_square);
  const fe n = fe_sub(fe_mul(fe_mul(c, fe_sub(r, one)), FE_D_MINUS_ONE_SQ()), v);
  const fe ss = fe_sq(s);
  ge_p1p1 out;
  out.X = fe_mul(fe_add(s, s), v);              // w0 = 2 s v
  out.Z = fe_mul(n, FE_SQRT_AD_MINUS_ONE());    // w1 = n sqrt(a d - 1)
  out.Y = fe_sub(one, ss);                      // w2 = 1 - s^2
  out.T = fe_add(one, ss);                      // w3 = 1 + s^2
  return out;
}

// One half of from_uniform_bytes: MAP of 8 little-endian words (bit 255 ignored).
CPZ_HD ge_p3 elligator_map_words(const uint32_t w[8]) { return p1p1_to_p3(elligator_map(fe_fromwords(w))); }

// RistrettoPoint::from_uniform_bytes of 16 little-endian words (64 bytes), encoded: MAP of the
// first half plus MAP of the second.
CPZ_HD void ristretto_from_uniform_words(uint32_t out[8], const uint32_t w[16]) {
  ristretto_encode(out, ge_add(elligator_map_words(w), elligator_map_words(w + 8)));
}

}  // namespace cpz
