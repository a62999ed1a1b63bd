// Host entry point for the joint table as check_equation builds it (scalarmul.h
// build_joint_table<false>: the slot no window reads left out), part of the same CPU test
// library as hostlib.cpp and hostlib_joint.cpp.
#include <cstring>

#include "verify.h"

using namespace cpz;

extern "C" {

// Builds the lean joint table of two decodable points into 13 entries pre-filled with `fill`
// bytes.  Per entry: untouched[e] = 1 when every byte still holds `fill`; otherwise out + 32 e
// gets the entry's encoding (through the completed form the Straus loop starts from) and
// t2d_ok[e] whether T2d is 2 d X Y / Z.  Returns the number of entries, or -1 when a point does
// not decode.
int cpzt_joint_table_lean(uint8_t* out, int* untouched, int* t2d_ok, const uint8_t* y, const uint8_t* r,
                          int fill) {
  ge_p3 Y, R;
  uint32_t w[8];
  std::memcpy(w, y, 32);
  if (!ristretto_decode(Y, w)) return -1;
  std::memcpy(w, r, 32);
  if (!ristretto_decode(R, w)) return -1;
  ge_cached tv[kJointSlots];
  std::memset(tv, fill, sizeof(tv));
  build_joint_table<false>(host_table(tv), Y, R);
  for (int e = 0; e < kJointSlots; e++) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&tv[e]);
    untouched[e] = 1;
    for (size_t k = 0; k < sizeof(ge_cached); k++)
      if (b[k] != (unsigned char)fill) untouched[e] = 0;
    t2d_ok[e] = 0;
    if (untouched[e]) continue;
    const ge_p1p1 c = cached_to_p1p1(tv[e]);  // (2X, 2Y, 2Z, 2Z)
    uint32_t o[8];
    ristretto_encode(o, p1p1_to_p3(c));
    std::memcpy(out + 32 * e, o, 32);
    t2d_ok[e] = fe_equal(fe_mul(fe_mul(c.X, c.Y), FE_D()), fe_mul(c.Z, tv[e].T2d)) ? 1 : 0;
  }
  return kJointSlots;
}

}  // extern "C"
