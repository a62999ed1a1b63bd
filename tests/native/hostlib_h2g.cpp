// Host entry points for hash-to-group (csrc/sha512.h, csrc/elligator.h), part of the same CPU test
// library as hostlib.cpp: the code k_sha512_rows and k_from_uniform run per thread, here under
// CPZ_BOUNDS_CHECK, for tests/test_hash_to_group_host.py to hold against hashlib and the oracle.
// With CPZT_H2G_MAIN the file is a program of its own (for a sanitizer build): it hashes messages
// of every length 0..300 and 4096 that end exactly at the end of a heap block, so that a read past
// a message is a fault there, and checks two known answers.
#include <cstring>

#include "elligator.h"
#include "sha512.h"

using namespace cpz;

extern "C" {

// SHA-512 of blob[off .. off + len) -> 64 digest bytes.
void cpzt_sha512(uint8_t digest[64], const uint8_t* blob, uint64_t off, uint64_t len) {
  uint32_t w[16];
  sha512_words(w, blob + off, len);
  std::memcpy(digest, w, 64);
}

// MAP(t) of one 32-byte half (bit 255 ignored) -> canonical X, Y, Z, T (4 x 32 bytes).
void cpzt_elligator_map(uint8_t xyzt[128], const uint8_t half[32]) {
  uint32_t w[8];
  std::memcpy(w, half, 32);
  const ge_p3 p = elligator_map_words(w);
  fe_tobytes(xyzt, p.X);
  fe_tobytes(xyzt + 32, p.Y);
  fe_tobytes(xyzt + 64, p.Z);
  fe_tobytes(xyzt + 96, p.T);
}

// RistrettoPoint::from_uniform_bytes(uniform).compress()
void cpzt_from_uniform(uint8_t point[32], const uint8_t uniform[64]) {
  uint32_t w[16], out[8];
  std::memcpy(w, uniform, 64);
  ristretto_from_uniform_words(out, w);
  std::memcpy(point, out, 32);
}

// from_uniform_bytes(SHA-512(msg[0 .. len))).compress(): generator_h()'s construction
void cpzt_hash_to_group(uint8_t point[32], const uint8_t* msg, uint64_t len) {
  uint32_t w[16], out[8];
  sha512_words(w, msg, len);
  ristretto_from_uniform_words(out, w);
  std::memcpy(point, out, 32);
}

}  // extern "C"

#ifdef CPZT_H2G_MAIN
#include <cstdio>
#include <cstdlib>

namespace {

int expect_hex(const uint8_t* got, int n, const char* hex, const char* what) {
  for (int i = 0; i < n; i++) {
    unsigned v = 0;
    std::sscanf(hex + 2 * i, "%2x", &v);
    if (got[i] != v) return std::printf("%s: byte %d is %02x\n", what, i, got[i]), 1;
  }
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  uint8_t digest[64], point[32];
  // every length, the message flush with the end of its allocation
  uint8_t sum = 0;
  for (int k = 0; k <= 301; k++) {
    const int len = k <= 300 ? k : 4096;
    uint8_t* m = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    for (int i = 0; i < len; i++) m[i] = (uint8_t)(i * 7 + len);
    cpzt_sha512(digest, m + (len ? 0 : 1), 0, (uint64_t)len);
    sum ^= digest[0];
    std::free(m);
  }
  const char abc[] = "abc";
  cpzt_sha512(digest, reinterpret_cast<const uint8_t*>(abc), 0, 3);
  bad += expect_hex(digest, 64,
                    "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
                    "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
                    "SHA-512(abc)");
  const char dst[] = "chaum-pedersen-zkp-v1.0.0-generator-h";
  cpzt_hash_to_group(point, reinterpret_cast<const uint8_t*>(dst), sizeof(dst) - 1);
  bad += expect_hex(point, 32, "c8db6f46e1b91e7e93ace69eab46976efebe07deaf5b9a2a7442fd0236401623", "generator h");
  const char rfc[] = "Ristretto is traditionally a short shot of espresso coffee";
  cpzt_hash_to_group(point, reinterpret_cast<const uint8_t*>(rfc), sizeof(rfc) - 1);
  bad += expect_hex(point, 32, "3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46", "RFC 9496 A.3");
  if (bad) return std::printf("FAILED: %d\n", bad), 1;
  std::printf("ok: lengths 0..300 and 4096 hashed (%02x), three known answers\n", sum);
  return 0;
}
#endif
