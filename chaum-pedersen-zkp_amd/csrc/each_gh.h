// Per-proof verification with a (g, h) pair per entry (cpz_verify_each_gh): the parts shared by
// the kernels (kernels.hip: k_challenge_gh, k_verify_quad_gh) and the host build of the CPU unit
// tests (tests/native/hostlib_gh.cpp) -- the entry's challenge, the generator verdict and where a
// quad's four tables lie in the launch's scratch.
#pragma once
#include "verify.h"

namespace cpz {

constexpr uint8_t kStBadGenerator = 6;  // CPZ_STATUS_BAD_GENERATOR

// The challenge of an entry under its own pair (batch.rs:188-206): `s` holds the state after
// Transcript::new(), which no pair enters; then the context if the entry has one, generator-g /
// generator-h, and the statement, commitment and challenge of transcript_challenge.
template <class Acc>
CPZ_HD sc challenge_gh(Strobe<Acc>& s, bool has_ctx, const uint8_t* ctx, uint32_t ctx_len, const uint32_t g[8],
                       const uint32_t h[8], const uint32_t y1[8], const uint32_t y2[8], const uint32_t r1[8],
                       const uint32_t r2[8]) {
  if (has_ctx) transcript_context(s, ctx, ctx_len);
  transcript_parameters(s, g, h);
  return transcript_challenge(s, y1, y2, r1, r2);
}

// Parameters::with_generators(g, h) would fail (gadgets.rs:77-103): a generator does not decode,
// one is the identity (the all-zero encoding), or the two are equal -- encodings are canonical,
// so the words decide.  dec: both encodings decoded.
CPZ_HD bool gh_generators_bad(bool dec, const uint32_t g[8], const uint32_t h[8]) {
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= g[k] ^ h[k];
  return !dec || words8_zero(g) || words8_zero(h) || diff == 0;
}

// A quad of k_verify_quad_gh keeps four tables of kGhTableInts ints (quad_table's layout: 9
// entries of 4 fields x 10 limbs) in the launch's scratch: the cached multiples 0..8 of -Y, of
// -+R, of B and of 2^128 B (B = g for the proof's first quad, h for its second), in that order
// from int gh_quad_tab(slot) on, slot = the quad's number in the launch.  A proof's two quads
// take 2 x 4 tables: twice k_verify_quad's kQuadProofScratch bytes.
constexpr int kGhTableInts = 9 * 40;
constexpr int kGhQuadTables = 4;
constexpr int kGhTabY = 0, kGhTabR = 1, kGhTabB = 2, kGhTabB2 = 3;
CPZ_HD int64_t gh_quad_tab(int64_t slot, int table = 0) {
  return (slot * kGhQuadTables + table) * (int64_t)kGhTableInts;
}
constexpr int64_t kGhProofScratch = 2 * (int64_t)kGhQuadTables * kGhTableInts * 4;  // bytes

}  // namespace cpz
