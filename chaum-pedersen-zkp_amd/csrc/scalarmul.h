// Variable-time scalar multiplication loops (verification inputs are public, so
// data-dependent digits are allowed; SIMT divergence is avoided by using fixed windows:
// every lane adds at every window, digit 0 adds the identity).
//
// Replaces the reference's Ristretto255::scalar_mul (ristretto.rs:153-155) as used in
// verify_one (batch.rs:216-222): instead of four independent constant-time
// multiplications, each equation is one Straus double-scalar loop
//     Q = [s] B + [c] V        (B = g or h fixed, V = -y1 or -y2 per proof)
// whose result is compared with r by ristretto equality.
#pragma once
#include "timing_only.h"
#include "ristretto.h"
#include "scalar25519.h"

// Per-proof path (build_joint_table, straus_half_joint, comb_add), each 0 for the form before it:
//   CPZ_LAZY_SIGN   the sign of a looked-up entry moves to the accumulator: the entry is added
//                   unmodified and X of the completed running point is negated when the sign changes
//   CPZ_TABLE_LEAN  check_equation builds the joint table without the slot no window reads and
//                   without squaring Z = 1
//   CPZ_BUILD_LDS   (kernels.hip) the verify kernels build that table with the Niels forms of Y'
//                   and R' in LDS columns (BuildCols, build_joint_table_cols below), not in
//                   registers that spill
//   CPZ_SQ2_FOLD    (fe25519.h) the factor 2 of fe_sq2 rides on the first operand's multiples
#ifndef CPZ_LAZY_SIGN
#define CPZ_LAZY_SIGN 1
#endif
#ifndef CPZ_TABLE_LEAN
#define CPZ_TABLE_LEAN 1
#endif

namespace cpz {

constexpr int kTableV = 8;     // cached multiples 1..8 of a variable base (radix-16 digits)
constexpr int kTableSlots = kTableV + 1;  // + the identity at slot 0 (digit 0 needs no select)
constexpr int kTableB = 128;   // Niels multiples 1..128 of a fixed base (radix-256 digits)

// Fixed-base comb: for each of the 16 radix-2^16 windows k, the affine Niels multiples
// j * 2^(16 k) * B, j = 0..2^15 (slot 0 the identity, so a zero digit needs no select), of one
// base (64 MiB per base in HBM).  [s] B for any s < 2^253 is then 16 mixed additions and no
// doubling.
constexpr int kCombWindows = 16;
constexpr int kCombEntries = 1 << 15;          // nonzero multiples per window
constexpr int kCombStride = kCombEntries + 1;  // + the identity at slot 0
constexpr int64_t kCombPerBase = (int64_t)kCombWindows * kCombStride;

// Device view of one base's comb (entries in global memory).
struct CombTable {
  const ge_niels* p;
  // entry mag (0..2^15) of window k as stored, no sign applied
  CPZ_HDM ge_niels lookup_mag(int k, int mag) const {
    const ge_niels* e = p + (int64_t)k * kCombStride + mag;
    ge_niels r;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4* s = reinterpret_cast<const uint4*>(e);
    uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
    for (int v = 0; v < (int)(sizeof(ge_niels) / 16); v++) d[v] = s[v];
#else
    r = *e;
#endif
    return r;
  }
  CPZ_HDM ge_niels lookup(int k, int digit) const {
    return ge_niels_cneg(lookup_mag(k, digit < 0 ? -digit : digit), digit < 0);
  }
};

// The unsigned entry of any comb: lookup_mag where the comb has one (CombTable), else lookup with
// the magnitude as its digit (the host stand-ins of the unit tests).
template <class Comb>
CPZ_HD auto comb_entry(const Comb& comb, int k, int mag, int) -> decltype(comb.lookup_mag(k, mag)) {
  return comb.lookup_mag(k, mag);
}
template <class Comb>
CPZ_HD ge_niels comb_entry(const Comb& comb, int k, int mag, long) {
  return comb.lookup(k, mag);
}

// Per-proof table of cached points (tab[0] = identity, tab[k] = k P), addressed as a base
// pointer plus a 32-bit byte offset per entry: entry e at col + 160 e, its 16-byte vectors
// contiguous.  The verify kernel keeps each thread's entries contiguous (col = the thread's
// slab slot).  Measured against two interleaved layouts in which one wave-wide load
// of a vector reads 1 KiB of consecutive slots (lane-interleaved over the whole slab, and
// wave-interleaved: 64 lanes per 184 KB region): 48.0 M and 48.2 M against 51.8 M proofs/s for
// the contiguous form (same gpurun call, two passes each) -- a lane's 9 entries in one 1.4 KB
// run beat full-line wave accesses spread over 10 separate 1-KiB rows per lookup.
constexpr int kCachedVecs = (int)(sizeof(ge_cached) / 16);

struct SlabTable {
  char* base;    // slab (wave-uniform)
  uint32_t col;  // byte offset of this thread's table (entry 0)
  static constexpr uint32_t kEntryBytes = kCachedVecs * 16;
  // entry e: one 32-bit offset per lookup; the 16-byte vectors of the entry are then
  // addressed as immediate offsets from it (computing base + 32-bit offset + 16 v in 32 bits
  // per vector made the compiler hoist one address register per (entry, vector) out of the
  // loops and spill)
  CPZ_HDM const char* entry(int e) const { return base + (col + (uint32_t)e * kEntryBytes); }
  // the table that starts e0 entries further on
  CPZ_HDM SlabTable shifted(int e0) const { return SlabTable{base, col + (uint32_t)e0 * kEntryBytes}; }
  CPZ_HDM ge_cached load(int e) const {
    ge_cached r;
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
    const char* p = entry(e);
#pragma unroll
    for (int v = 0; v < kCachedVecs; v++) {
#if defined(__HIP_DEVICE_COMPILE__)
      const uint4 x = *reinterpret_cast<const uint4*>(p + 16 * v);
      d[4 * v] = x.x; d[4 * v + 1] = x.y; d[4 * v + 2] = x.z; d[4 * v + 3] = x.w;
#else
      const uint32_t* s = reinterpret_cast<const uint32_t*>(p + 16 * v);
      for (int k = 0; k < 4; k++) d[4 * v + k] = s[k];
#endif
    }
    return r;
  }
  CPZ_HDM void store(int e, const ge_cached& c) const {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&c);
    char* p = const_cast<char*>(entry(e));
#pragma unroll
    for (int v = 0; v < kCachedVecs; v++) {
#if defined(__HIP_DEVICE_COMPILE__)
      *reinterpret_cast<uint4*>(p + 16 * v) = make_uint4(s[4 * v], s[4 * v + 1], s[4 * v + 2], s[4 * v + 3]);
#else
      uint32_t* d = reinterpret_cast<uint32_t*>(p + 16 * v);
      for (int k = 0; k < 4; k++) d[k] = s[4 * v + k];
#endif
    }
  }
};

// Digit words of a scalar multiplication held outside the registers: word k at p[k * stride].
// The verify kernel keeps them in LDS (one column per thread, conflict-free), which takes 16
// words per proof out of the Straus loop's register budget; the host build uses a plain array.
struct DigitRef {
  const uint32_t* p;
  int stride;
  CPZ_HDM uint32_t operator[](int k) const { return p[k * stride]; }
};
CPZ_HD DigitRef host_digits(const uint32_t* a) { return DigitRef{a, 1}; }

// A host array of cached points as a table (unit tests).
CPZ_HD SlabTable host_table(ge_cached* p) { return SlabTable{reinterpret_cast<char*>(p), 0u}; }

CPZ_HD ge_niels niels_lookup(const ge_niels* tab, int digit) {
  const int mag = digit < 0 ? -digit : digit;
  const ge_niels e = tab[(mag == 0 ? 1 : mag) - 1];
  const ge_niels r = mag == 0 ? ge_niels_identity() : e;
  return ge_niels_cneg(r, digit < 0);
}

// tab[0] is the identity, tab[k] = k P: one load and a conditional negation.
CPZ_HD ge_cached cached_lookup(const SlabTable& tab, int digit) {
  const int mag = digit < 0 ? -digit : digit;
  return ge_cached_cneg(tab.load(mag), digit < 0);
}
// Four doublings of a pending completed point.
CPZ_HD ge_p1p1 dbl4(const ge_p1p1& cur) {
  ge_p1p1 t = cur;
#pragma unroll 1
  for (int d = 0; d < 4; d++) t = p2_dbl(p1p1_to_p2(t));
  return t;
}

CPZ_HD ge_p1p1 p1p1_identity() {
  ge_p1p1 cur;
  cur.X = fe_zero(); cur.Y = fe_one(); cur.Z = fe_one(); cur.T = fe_one();
  return cur;
}

// Writes the identity and the cached multiples 1..8 of an AFFINE P (Z = 1, as decoded) to
// tab[0..8]: 1 doubling + 6 mixed additions of P in Niels form (3M each instead of 4M for a
// cached addition).
// (An unrolled 4-doubling / 3-addition schedule saves a few more multiplications but keeps
// three extended points live and measured slower from the extra spills.)
CPZ_HD void build_cached_table(const SlabTable& tab, const ge_p3& P) {
  ge_niels n1;
  n1.ypx = fe_add(P.Y, P.X);
  n1.ymx = fe_sub(P.Y, P.X);
  n1.xy2d = fe_mul(P.T, FE_D2());
  tab.store(0, ge_cached_identity());
  {
    ge_cached c1;
    c1.YpX = n1.ypx;
    c1.YmX = n1.ymx;
    c1.Z = P.Z;
    c1.T2d = n1.xy2d;
    tab.store(1, c1);
  }
  ge_p3 acc = p1p1_to_p3(p3_dbl(P));
  tab.store(2, p3_to_cached(acc));
#pragma unroll 1
  for (int k = 3; k <= kTableV; k++) {
    acc = p1p1_to_p3(ge_add_niels(acc, n1));
    tab.store(k, p3_to_cached(acc));
  }
}

// Q = [s] B + [c] V.  tab_v: cached multiples 1..8 of V; tab_b: Niels multiples 1..128
// of B; cdig: radix-16 signed digits of c; sdig: radix-256 signed digits of s.
// 63 x 4 doublings, 64 cached additions, 32 Niels additions.
CPZ_HD ge_p3 straus_vartime(const SlabTable& tab_v, const ge_niels* tab_b, const uint32_t cdig_in[8],
                            const uint32_t sdig_in[8]) {
  uint32_t cdig[8], sdig[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { cdig[j] = cdig_in[j]; sdig[j] = sdig_in[j]; }
  ge_p1p1 cur = p1p1_identity();
#pragma unroll 1
  for (int j = 7; j >= 0; j--) {
    const uint32_t wc = cdig[7], wg = sdig[7];
#pragma unroll
    for (int t = 7; t > 0; t--) { cdig[t] = cdig[t - 1]; sdig[t] = sdig[t - 1]; }
#pragma unroll 1
    for (int m = 7; m >= 0; m--) {
      const int dc = ((int32_t)(wc << (28 - 4 * m))) >> 28;
      const ge_cached ev = cached_lookup(tab_v, dc);
      if (j != 7 || m != 7) cur = dbl4(cur);
      cur = ge_add_cached(p1p1_to_p3(cur), ev);
      if ((m & 1) == 0) {
        const int dg = ((int32_t)(wg << (24 - 8 * (m >> 1)))) >> 24;
        cur = ge_add_niels(p1p1_to_p3(cur), niels_lookup(tab_b, dg));
      }
    }
  }
  return p1p1_to_p3(cur);
}

// Adds [s] B to a pending completed point through the comb (16 mixed additions).
// sdig: 16 radix-2^16 signed digits (sc_recode_radix65536).
// Lazy sign: the sum is kept as sigma * cur, sigma = the sign of the last digit added (`sign` on
// entry: the point handed in is cur when sign >= 0, -cur when sign < 0).  A digit d of sign tau
// adds the stored entry |d| to (sigma tau) * cur: sigma (cur) + tau E = tau (sigma tau cur + E).
// The returned point carries its true sign.
template <class Comb, class Dig>
CPZ_HD ge_p1p1 comb_add(ge_p1p1 cur, const Comb& comb, const Dig& sd, int32_t sign = 0) {
#pragma unroll 1
  for (int j = 0; j < 8; j++) {
    const uint32_t w = sd[j];
    // (requesting both entries of the pair before the first addition measured 2 % slower:
    // 30 more live VGPRs)
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const int d = (int32_t)(w << (16 - 16 * m)) >> 16;
#if CPZ_LAZY_SIGN
      const ge_niels e = comb_entry(comb, 2 * j + m, d < 0 ? -d : d, 0);
      cur = ge_add_niels(p1p1_to_p3(ge_p1p1_cneg(cur, d ^ sign)), e);
      sign = d;
#else
      cur = ge_add_niels(p1p1_to_p3(cur), comb.lookup(2 * j + m, d));
#endif
    }
  }
  return ge_p1p1_cneg(cur, sign);
}

// Joint table of one equation (see verify.h): the 13 cached combinations a Y' + b R' with
// a in 0..2, b in -2..2 at slot 5 a + b, slot 0 the identity.  A window's signed digit pair
// (a, b) is the entry |5 a + b|, negated when 5 a + b < 0 (|b| <= 2 < 5: that is a < 0, or a = 0
// and b < 0).
constexpr int kJointSlots = 13;
CPZ_HD constexpr int joint_slot(int a, int b) { return 5 * a + b; }
// Signed slot of window m < 16 of a digit-word pair (wu, wv), and the top window's (unsigned).
CPZ_HD int joint_window(uint32_t wu, uint32_t wv, int m) { return joint_slot(radix4_digit(wu, m), radix4_digit(wv, m)); }
CPZ_HD int joint_top_window(uint32_t wu3, uint32_t wv3) {
  return joint_slot(radix4_top_digit(wu3), radix4_top_digit(wv3));
}

// Writes the joint table of AFFINE Y, R (Z = 1, as decoded): 70 M + 16 S, 13 stores.
//   (1, 0), (0, 1)   the points themselves, their 2 d T one product each;
//   (1, s)           Y + s R, a mixed addition (s = +1, -1);
//   (1, 2 s)         (1, s) + s R;
//   (2, s)           (1, s) + Y;
//   (2, 2 s)         2 (1, s);
//   (2, 0), (0, 2)   2 Y, 2 R.
// One copy of the addition code (the rolled loops over s and j) and one of the doubling code
// (the loop over d); beside the two affine inputs at most two extended points are live: (1, s)
// and the one being stored.  (The compiler spills in this function, not in the Straus loop.)
//
// kFull = false (what check_equation builds, CPZ_TABLE_LEAN) leaves out what no verdict needs,
// 5 M + 6 S of the 70 M + 16 S:
//   slot (2, -2) is neither computed nor stored: no window selects it (a = 2 only stands for
//     a negated a = -2, whose b is then in -1..2; the top window's digits are not negative);
//   2 Y and 2 R take 2 Z^2 = 2 instead of squaring Z = 1.  Their doubling is a second copy of the
//     code, outside the rolled loop: selecting 2 Z^2 inside the one copy cost 100 more spilled
//     VGPRs (scratch 300 -> 692 B per lane), the peeled form spills less than the full build
//     (268 B).
// (Y + R and Y - R also share the product T_Y * 2dT_R, 1 M.  Kept across the loop over s it
// spilled 4 more VGPRs in the form it was tried in, so it is computed twice.)
template <bool kFull = true>
CPZ_HD void build_joint_table(const SlabTable& tab, const ge_p3& Y, const ge_p3& R) {
  ge_niels nY, nR;
  nY.ypx = fe_add(Y.Y, Y.X);
  nY.ymx = fe_sub(Y.Y, Y.X);
  nY.xy2d = fe_mul(Y.T, FE_D2());
  nR.ypx = fe_add(R.Y, R.X);
  nR.ymx = fe_sub(R.Y, R.X);
  nR.xy2d = fe_mul(R.T, FE_D2());
  tab.store(0, ge_cached_identity());
  tab.store(joint_slot(1, 0), ge_cached{nY.ypx, nY.ymx, Y.Z, nY.xy2d});
  tab.store(joint_slot(0, 1), ge_cached{nR.ypx, nR.ymx, R.Z, nR.xy2d});
#pragma unroll 1
  for (int neg = 0; neg < 2; neg++) {
    const int s = neg ? -1 : 1;
    const ge_niels nRs = ge_niels_cneg(nR, neg != 0);
    ge_p3 A = Y;
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
      // j = 0: Y + s R = (1, s), kept in A;  j = 1: A + s R = (1, 2 s);  j = 2: A + Y = (2, s)
      const ge_p3 Q = p1p1_to_p3(ge_add_niels(A, j == 2 ? nY : nRs));
      tab.store(j == 0 ? joint_slot(1, s) : (j == 1 ? joint_slot(1, 2 * s) : joint_slot(2, s)), p3_to_cached(Q));
      if (j == 0) A = Q;
    }
    if constexpr (kFull) {
#pragma unroll 1
      for (int d = 0; d < 2; d++) {
        // d = 0: 2 A = (2, 2 s);  d = 1: 2 Y = (2, 0) in the first pass over s, 2 R = (0, 2) in the second
        const ge_p3& P = d == 0 ? A : (neg ? R : Y);
        const int slot = d == 0 ? joint_slot(2, 2 * s) : (neg ? joint_slot(0, 2) : joint_slot(2, 0));
        tab.store(slot, p3_to_cached(p1p1_to_p3(p2_dbl(ge_p2{P.X, P.Y, P.Z}))));
      }
    } else {
      // 2 A = (2, 2) in the first pass only: (2, -2) is the slot no window reads
      if (!neg) tab.store(joint_slot(2, 2), p3_to_cached(p1p1_to_p3(p2_dbl(ge_p2{A.X, A.Y, A.Z}))));
      // 2 Y = (2, 0) in the first pass, 2 R = (0, 2) in the second: affine points, 2 Z^2 = 2
      const ge_p3& P = neg ? R : Y;
      const ge_p1p1 D = p2_dbl_zz2(P.X, P.Y, fe_add(fe_one(), fe_one()));
      tab.store(neg ? joint_slot(0, 2) : joint_slot(2, 0), p3_to_cached(p1p1_to_p3(D)));
    }
  }
}

// The lean build with its long-lived operands outside the registers (CPZ_BUILD_LDS, verify.h
// check_equation): the affine Niels forms of Y' and R' as six field elements in word columns, word
// w at p[w * stride] -- in the verify kernels one LDS column per thread, conflict-free as the digit
// words are (DigitRef); the host build uses a plain array.  Field f: 0..2 = (y + x, y - x, 2 d x y)
// of Y', 3..5 of R'.  A limb is read where a product or a sum consumes it; beside the running
// (1, +-1) point only T of Y' stays in registers.
constexpr int kBuildFields = 6;
constexpr int kBuildWords = 10 * kBuildFields;
struct BuildCols {
  uint32_t* p;
  int stride;
  CPZ_HDM fe load(int f) const {
    const uint32_t* q = p + 10 * f * stride;
    fe r;
#pragma unroll
    for (int k = 0; k < 10; k++) r.v[k] = (int32_t)q[k * stride];
    return r;
  }
  CPZ_HDM void store(int f, const fe& x) const {
    uint32_t* q = p + 10 * f * stride;
#pragma unroll
    for (int k = 0; k < 10; k++) q[k * stride] = (uint32_t)x.v[k];
  }
  // x and y of the affine point whose Niels form is fields f0, f0 + 1: y + x and y - x are exact
  // limb sums, so their half difference and half sum are the decoded limbs themselves.
  CPZ_HDM void affine(int f0, fe& X, fe& Y) const {
    const fe ypx = load(f0), ymx = load(f0 + 1);
#pragma unroll
    for (int k = 0; k < 10; k++) {
      X.v[k] = (ypx.v[k] - ymx.v[k]) >> 1;
      Y.v[k] = (ypx.v[k] + ymx.v[k]) >> 1;
    }
  }
  // The point's Niels form into fields 3 which .. 3 which + 2 and its cached form (Z = 1) into
  // the table: what build_joint_table writes to slots (1, 0) and (0, 1).
  CPZ_HDM void put_point(int which, const ge_p3& P, const SlabTable& tab) const {
    ge_cached c;
    c.YpX = fe_add(P.Y, P.X);
    c.YmX = fe_sub(P.Y, P.X);
    c.Z = P.Z;
    c.T2d = fe_mul(P.T, FE_D2());
    store(3 * which, c.YpX);
    store(3 * which + 1, c.YmX);
    store(3 * which + 2, c.T2d);
    tab.store(which ? joint_slot(0, 1) : joint_slot(1, 0), c);
  }
};

// The remaining nine entries of build_joint_table<false> after put_point(0, Y') and
// put_point(1, R'), with the same products in the same order on the same limbs: with the identity
// at slot 0, which the caller stores (once for both equations of a proof: they share the slots),
// the table is bit for bit the one build_joint_table<false> writes.  YT: T of Y'.
//   A = Y' at the head of a pass is (x, y) from the columns, Z = 1 and YT;
//   s R' is R' with fields 3 and 4 swapped and field 5 negated (ge_niels_cneg);
//   2 Y', 2 R' take x, y from the columns.
// The field index of every read depends on the loop counters, so no read is hoisted out of the
// rolled loops into registers that would have to live across them.
CPZ_HD void build_joint_table_cols(const SlabTable& tab, const BuildCols& cols, const fe& YT) {
#pragma unroll 1
  for (int neg = 0; neg < 2; neg++) {
    const int s = neg ? -1 : 1;
    ge_p3 A;
    cols.affine(0, A.X, A.Y);
    A.Z = fe_one();
    A.T = YT;
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
      // j = 0: Y + s R = (1, s), kept in A;  j = 1: A + s R = (1, 2 s);  j = 2: A + Y = (2, s)
      const int f0 = j == 2 ? 0 : 3, swap = j == 2 ? 0 : neg;
      const fe PP = fe_mul(fe_add(A.Y, A.X), cols.load(f0 + swap));
      const fe MM = fe_mul(fe_sub(A.Y, A.X), cols.load(f0 + 1 - swap));
      const fe Txy2d = fe_mul(A.T, fe_cneg(cols.load(f0 + 2), -swap));
      const fe Z2 = fe_add(A.Z, A.Z);
      ge_p1p1 r;
      r.X = fe_sub(PP, MM);
      r.Y = fe_add(PP, MM);
      r.Z = fe_add(Z2, Txy2d);
      r.T = fe_sub(Z2, Txy2d);
      const ge_p3 Q = p1p1_to_p3(r);
      tab.store(j == 0 ? joint_slot(1, s) : (j == 1 ? joint_slot(1, 2 * s) : joint_slot(2, s)), p3_to_cached(Q));
      if (j == 0) A = Q;
    }
    // 2 A = (2, 2) in the first pass only: (2, -2) is the slot no window reads
    if (!neg) tab.store(joint_slot(2, 2), p3_to_cached(p1p1_to_p3(p2_dbl(ge_p2{A.X, A.Y, A.Z}))));
    // 2 Y = (2, 0) in the first pass, 2 R = (0, 2) in the second: affine points, 2 Z^2 = 2
    fe PX, PY;
    cols.affine(neg ? 3 : 0, PX, PY);
    const ge_p1p1 D = p2_dbl_zz2(PX, PY, fe_add(fe_one(), fe_one()));
    tab.store(neg ? joint_slot(0, 2) : joint_slot(2, 0), p3_to_cached(p1p1_to_p3(D)));
  }
}

// The completed form ((X:Z), (Y:T)) of a cached entry: x = (YpX - YmX) / 2Z, y = (YpX + YmX) / 2Z.
// No product, and the limbs are exactly 2 X, 2 Y, 2 Z of the tight point the entry was made from.
CPZ_HD ge_p1p1 cached_to_p1p1(const ge_cached& e) {
  ge_p1p1 r;
  r.X = fe_sub(e.YpX, e.YmX);
  r.Y = fe_add(e.YpX, e.YmX);
  r.Z = fe_add(e.Z, e.Z);
  r.T = r.Z;
  return r;
}

// Half-size per-proof check with the comb (see verify.h):
//   Q = [u] Y' + [v] R' (joint Straus: 63 x 2 doublings, 63 cached additions) + [s'] B (comb),
// returned as a completed point (callers only test it for the identity).
// tab: the joint table of Y', R'; ud, vd: the radix-4 digits of u, |v| < 3 * 2^125
// (sc_recode_radix4_half); sdig: 16 radix-2^16 signed digits of s' < 2^253.
// The top window (unsigned digits, nothing to double yet) starts the sum from its entry in
// completed form, which the next window's doublings take as it is.
template <class Comb, class Dig>
CPZ_HD ge_p1p1 straus_half_joint(const SlabTable& tab, const Comb& comb, const Dig& ud, const Dig& vd,
                                 const Dig& sdig) {
  ge_p1p1 cur = cached_to_p1p1(tab.load(joint_top_window(ud[3], vd[3])));
  // Lazy sign: the sum so far is sigma * cur, sigma = the sign of the last window's slot (the
  // top window's is +, and so is slot 0's).  A window of sign tau adds the stored entry to
  // (sigma tau) * 4 cur -- doublings commute with the sign -- and leaves sigma = tau:
  //   sigma (4 cur) + tau E = tau (sigma tau (4 cur) + E).
  // Negating X of the completed point negates X and T of its extended form, the point's negative.
  int32_t sign = 0;
#pragma unroll 1
  for (int j = 3; j >= 0; j--) {
    const uint32_t wu = ud[j], wv = vd[j];
#pragma unroll 1
    for (int m = j == 3 ? 14 : 15; m >= 0; m--) {
      // the table load issued before the two doublings, which hide part of its latency
      // (the table lives in the HBM-backed scratch slab)
      const int slot = joint_window(wu, wv, m);
#if CPZ_LAZY_SIGN
      const ge_cached e = tab.load(slot < 0 ? -slot : slot);
#else
      const ge_cached e = cached_lookup(tab, slot);
#endif
      cur = p2_dbl(p1p1_to_p2(cur));
      cur = p2_dbl(p1p1_to_p2(cur));
#if CPZ_LAZY_SIGN
      cur.X = fe_cneg(cur.X, slot ^ sign);
      sign = slot;
#endif
#if defined(CPZ_EXP_NIELS_TABLES)
      // timing experiment only (timing_only.h: wrong verdicts): the entry added as an affine
      // Niels point, Z never read -- the best case of normalised per-proof tables
      cur = ge_add_niels(p1p1_to_p3(cur), ge_niels{e.YpX, e.YmX, e.T2d, {0, 0}});
#else
      cur = ge_add_cached(p1p1_to_p3(cur), e);
#endif
    }
  }
  return comb_add(cur, comb, sdig, sign);
}

// [s] B through the comb (prover path): 16 mixed additions.
template <class Comb>
CPZ_HD ge_p3 comb_mul(const Comb& comb, const uint32_t sdig[8]) {
  return p1p1_to_p3(comb_add(p1p1_identity(), comb, host_digits(sdig)));
}

// [s] B by Horner over radix-256 signed digits (prover path).
CPZ_HD ge_p3 fixed_base_mul(const ge_niels* tab_b, const uint32_t sdig_in[8]) {
  uint32_t sdig[8];
#pragma unroll
  for (int j = 0; j < 8; j++) sdig[j] = sdig_in[j];
  ge_p1p1 cur = p1p1_identity();
#pragma unroll 1
  for (int j = 7; j >= 0; j--) {
    const uint32_t wg = sdig[7];
#pragma unroll
    for (int t = 7; t > 0; t--) sdig[t] = sdig[t - 1];
#pragma unroll 1
    for (int m = 3; m >= 0; m--) {
      if (j != 7 || m != 3) {
        cur = dbl4(cur);
        cur = dbl4(cur);
      }
      const int dg = ((int32_t)(wg << (24 - 8 * m))) >> 24;
      cur = ge_add_niels(p1p1_to_p3(cur), niels_lookup(tab_b, dg));
    }
  }
  return p1p1_to_p3(cur);
}

// One (g, h) pair's Niels tables (GenSet::tab; k_niels_bases / k_build_niels): multiples 1..128 of
// 2^(32 m) g and 2^(32 m) h, m = 0..7, as [level][generator][128 entries] with the levels in the
// order m = 0, 4, 2, 6, 1, 3, 5, 7 (cpz_kernels.h, niels_level_doublings).
constexpr int kNielsEntries = kTableB;   // radix-256 signed digits: |d| <= 128
// the level holding 2^(32 q) B: part q (word q) of a 256-bit scalar
constexpr int kNielsLevelOfPart[8] = {0, 4, 2, 5, 1, 6, 3, 7};

CPZ_HD ge_niels niels_entry(const ge_niels* e) {
  ge_niels r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s = reinterpret_cast<const uint4*>(e);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (int v = 0; v < (int)(sizeof(ge_niels) / 16); v++) d[v] = s[v];
#else
  r = *e;
#endif
  return r;
}

// [d] g and [d] h together from one pair's tables (mixed-pair prover, k_prove_points_pairs).
// dig: the radix-256 signed digits of d < 2^253 (sc_recode_radix256: 32 bytes in [-128, 127],
// digit j at weight 2^(8 j), four per word).  Digit 4 q + b sits at weight 2^(8 b) on 2^(32 q) B,
// so for window b = 3..0: 8 doublings of both sums (none before the first window), then for
// part q = 0..7 the entry |digit| - 1 of part q's table of g and of h, negated for a negative
// digit; a zero digit adds nothing.  24 doublings and at most 32 additions per product, one
// digit decode for both.
// Lazy sign (as comb_add): each sum is kept as sigma * cur, sigma = the sign of the last
// non-zero digit; a digit of sign tau adds the stored entry to (sigma tau) * cur.  Doublings
// commute with the sign, and both sums see the same digits, so they share sigma.
CPZ_HD void pair_table_mul(ge_p3& G, ge_p3& H, const ge_niels* tab, const uint32_t dig_in[8]) {
  uint32_t dig[8];
#pragma unroll
  for (int q = 0; q < 8; q++) dig[q] = dig_in[q];
  ge_p1p1 cg = p1p1_identity(), ch = p1p1_identity();
  int32_t sign = 0;
#pragma unroll 1
  for (int b = 3; b >= 0; b--) {
    if (b != 3) {
#pragma unroll 1
      for (int k = 0; k < 8; k++) {
        cg = p2_dbl(p1p1_to_p2(cg));
        ch = p2_dbl(p1p1_to_p2(ch));
      }
    }
#pragma unroll 1
    for (int q = 0; q < 8; q++) {
      // byte 3 of word 0 is digit 4 q + 3, the top one; the words rotate so that no runtime index
      // selects a register
      const uint32_t w = dig[0];
#pragma unroll
      for (int t = 0; t < 7; t++) dig[t] = dig[t + 1];
      dig[7] = w << 8;
      const int32_t d = (int32_t)w >> 24;
      if (d == 0) continue;
      const ge_niels* e = tab + (2 * kNielsLevelOfPart[q]) * kNielsEntries + ((d < 0 ? -d : d) - 1);
      const ge_niels eg = niels_entry(e), eh = niels_entry(e + kNielsEntries);
      const int32_t flip = d ^ sign;
      cg = ge_add_niels(p1p1_to_p3(ge_p1p1_cneg(cg, flip)), eg);
      ch = ge_add_niels(p1p1_to_p3(ge_p1p1_cneg(ch, flip)), eh);
      sign = d;
    }
  }
  G = p1p1_to_p3(ge_p1p1_cneg(cg, sign));
  H = p1p1_to_p3(ge_p1p1_cneg(ch, sign));
}

// k * B for 1 <= k <= 255 by double-and-add (table construction).
CPZ_HD ge_p3 small_mul(const ge_p3& B, int k) {
  ge_p3 acc = ge_identity();
#pragma unroll 1
  for (int bit = 7; bit >= 0; bit--) {
    acc = p1p1_to_p3(p3_dbl(acc));
    if ((k >> bit) & 1) acc = ge_add(acc, B);
  }
  return acc;
}

}  // namespace cpz
