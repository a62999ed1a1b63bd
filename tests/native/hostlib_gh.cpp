// Host entry points for the parts of cpz_verify_each_gh that csrc/each_gh.h shares between the
// kernels and this CPU build (the same test library as hostlib.cpp): the entry's challenge from the
// one snapshot no pair enters, the generator verdict, and where a quad's four tables lie in a
// launch's scratch.
// With CPZT_GH_MAIN the file is a program of its own (for a sanitizer build): it runs the three
// over fixed inputs -- every context shape, every bad-generator kind, every quad of a full launch.
#include <cstring>
#include <vector>

#include "each_gh.h"

using namespace cpz;

extern "C" {

// c_out: the 32-byte challenge of one entry under (g, h); has_ctx = 0: no context (None), else the
// ctx_len bytes at ctx (Some, possibly empty).  The sponge starts from Transcript::new()'s state, as
// the kernel's does from the snapshot the runtime passes it.
void cpzt_gh_challenge(uint8_t c_out[32], const uint8_t g[32], const uint8_t h[32], const uint8_t y1[32],
                       const uint8_t y2[32], const uint8_t r1[32], const uint8_t r2[32], int has_ctx,
                       const uint8_t* ctx, uint32_t ctx_len) {
  uint32_t w[6][8];
  const uint8_t* src[6] = {g, h, y1, y2, r1, r2};
  for (int k = 0; k < 6; k++) std::memcpy(w[k], src[k], 32);
  ArrayState st;
  Strobe<ArrayState> s = transcript_new(st);
  const sc c = challenge_gh(s, has_ctx != 0, ctx, ctx_len, w[0], w[1], w[2], w[3], w[4], w[5]);
  std::memcpy(c_out, c.w, 32);
}

// 1 if gh_generators_bad rejects rows (g, h), given decode flags computed here by ristretto_decode.
// (In the kernel the flags come from lane 2 of each quad and travel in bit 1 of the word the quads
// exchange; that packing and its reduction run on the GPU only and are covered by the GPU tests.)
int cpzt_gh_generators_bad(const uint8_t g[32], const uint8_t h[32]) {
  uint32_t gw[8], hw[8];
  std::memcpy(gw, g, 32);
  std::memcpy(hw, h, 32);
  ge_p3 P;
  const bool dg = ristretto_decode(P, gw), dh = ristretto_decode(P, hw);
  return gh_generators_bad(dg && dh, gw, hw) ? 1 : 0;
}

// The int offset of table `table` (0..3: -Y, -+R, B, 2^128 B) of quad `slot` of a launch.
long long cpzt_gh_quad_tab(long long slot, int table) { return (long long)gh_quad_tab(slot, table); }
int cpzt_gh_table_ints(void) { return kGhTableInts; }
long long cpzt_gh_proof_scratch(void) { return (long long)kGhProofScratch; }

}  // extern "C"

#ifdef CPZT_GH_MAIN
#include <cstdio>

int main() {
  int bad = 0;
  // the basepoint's encoding and the encoding of 2 B decode; 32 x 0xff does not
  const uint8_t B[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                         0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
  uint8_t B2[32], zero[32] = {0}, ff[32];
  std::memset(ff, 0xff, 32);
  {
    uint32_t w[8], o[8];
    std::memcpy(w, B, 32);
    ge_p3 P;
    if (!ristretto_decode(P, w)) return std::printf("FAILED: the basepoint does not decode\n"), 1;
    ristretto_encode(o, p1p1_to_p3(p3_dbl(P)));
    std::memcpy(B2, o, 32);
  }
  bad += cpzt_gh_generators_bad(B, B2) != 0;
  bad += cpzt_gh_generators_bad(B2, B) != 0;
  bad += cpzt_gh_generators_bad(ff, B) != 1;
  bad += cpzt_gh_generators_bad(B, ff) != 1;
  bad += cpzt_gh_generators_bad(zero, B) != 1;
  bad += cpzt_gh_generators_bad(B, zero) != 1;
  bad += cpzt_gh_generators_bad(B, B) != 1;
  // challenges: the four context shapes run, and differ from one another
  uint8_t c[4][32];
  std::vector<uint8_t> ctx(33, 0x5a);
  cpzt_gh_challenge(c[0], B, B2, B, B2, B2, B, 0, nullptr, 0);
  cpzt_gh_challenge(c[1], B, B2, B, B2, B2, B, 1, ctx.data(), 0);
  cpzt_gh_challenge(c[2], B, B2, B, B2, B2, B, 1, ctx.data(), 32);
  cpzt_gh_challenge(c[3], B, B2, B, B2, B2, B, 1, ctx.data(), 33);
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++) bad += std::memcmp(c[a], c[b], 32) == 0;
  // tables: consecutive, disjoint, and a launch of p proofs ends at p * kGhProofScratch bytes
  const long long proofs = 8192;
  long long next = 0;
  for (long long slot = 0; slot < 2 * proofs; slot++)
    for (int t = 0; t < kGhQuadTables; t++) {
      bad += cpzt_gh_quad_tab(slot, t) != next;
      next += kGhTableInts;
    }
  bad += next * 4 != proofs * kGhProofScratch;
  if (bad) return std::printf("FAILED: %d\n", bad), 1;
  std::printf("ok\n");
  return 0;
}
#endif
