// Host entry points for the folded doubling of fe_sq2 (fe25519.h fe_sq2_fold) beside the form it
// replaces, on raw limbs so that loose operands can be given, and for the joint-table build over
// word columns (scalarmul.h
// build_joint_table_cols) beside build_joint_table<false>.  Part of the same CPU test library as
// hostlib.cpp (CPZ_BOUNDS_CHECK: a limb bound that is passed aborts the process).
#include <cstring>

#include "verify.h"

using namespace cpz;

namespace {

fe fe_limbs(const int32_t* v) {
  fe r;
  for (int i = 0; i < 10; i++) r.v[i] = v[i];
  return r;
}

}  // namespace

extern "C" {

int cpzt_loose_bound() { return kLooseBound; }

// 2 f^2 from ten limbs by both forms: the limbs as computed (before any canonicalisation) and
// the canonical bytes.  Returns 1 when the two results agree limb for limb.
int cpzt_fe_sq2_forms(int32_t* limbs_fold, int32_t* limbs_shift, uint8_t* bytes_fold, uint8_t* bytes_shift,
                      const int32_t* f) {
  const fe a = fe_sq2_fold(fe_limbs(f)), b = fe_sq2_shift(fe_limbs(f));
  int same = 1;
  for (int i = 0; i < 10; i++) {
    limbs_fold[i] = a.v[i];
    limbs_shift[i] = b.v[i];
    same &= a.v[i] == b.v[i];
  }
  fe_tobytes(bytes_fold, a);
  fe_tobytes(bytes_shift, b);
  return same;
}

// The canonical bytes of f (ten limbs, any the carry accepts).
void cpzt_fe_limbs_bytes(uint8_t* out, const int32_t* f) { fe_tobytes(out, fe_limbs(f)); }

// The lean joint table of two decodable points (negated as check_equation negates them when
// `negate`), once by build_joint_table<false> and once through word columns at the given stride
// (the identity, put_point twice, then build_joint_table_cols), both into tables pre-filled with `fill`.
// Returns the number of bytes in which the two tables differ (0: bit for bit the same, the
// unwritten slot included), or -1 when a point does not decode.
int cpzt_joint_table_cols_diff(const uint8_t* y, const uint8_t* r, int negate, int stride, int fill) {
  ge_p3 Y, R;
  uint32_t w[8];
  std::memcpy(w, y, 32);
  if (!ristretto_decode(Y, w)) return -1;
  std::memcpy(w, r, 32);
  if (!ristretto_decode(R, w)) return -1;
  if (negate) {
    Y = ge_neg(Y);
    R = ge_neg(R);
  }
  ge_cached ta[kJointSlots], tb[kJointSlots];
  std::memset(ta, fill, sizeof(ta));
  std::memset(tb, fill, sizeof(tb));
  build_joint_table<false>(host_table(ta), Y, R);
  uint32_t* words = new uint32_t[(size_t)kBuildWords * stride];
  std::memset(words, fill ^ 0x5a, sizeof(uint32_t) * kBuildWords * stride);
  const BuildCols cols{words, stride};
  host_table(tb).store(0, ge_cached_identity());  // the caller's part (verify_proof)
  cols.put_point(0, Y, host_table(tb));
  cols.put_point(1, R, host_table(tb));
  build_joint_table_cols(host_table(tb), cols, Y.T);
  delete[] words;
  int diff = 0;
  const unsigned char* a = reinterpret_cast<const unsigned char*>(ta);
  const unsigned char* b = reinterpret_cast<const unsigned char*>(tb);
  for (size_t k = 0; k < sizeof(ta); k++) diff += a[k] != b[k];
  return diff;
}

}  // extern "C"
