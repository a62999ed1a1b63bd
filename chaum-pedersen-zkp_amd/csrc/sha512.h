// SHA-512 (FIPS 180-4) over a byte range, one thread per message.
//
// Replaces the sha2 crate's Sha512 as the reference reaches it in generator_h()
// (src/primitives/ristretto.rs:86-91): the 64 digest bytes are the uniform input of
// RistrettoPoint::from_uniform_bytes (elligator.h).
//
// The message is read with byte loads: messages start at arbitrary byte offsets of a blob.
// The 80 rounds of a block are unrolled, so that every index into the 16-word schedule and into
// the eight working variables is a compile-time constant and both stay in registers (a
// runtime-indexed array would go to scratch); the loop over a message's blocks stays rolled.
//
// __host__ __device__ like the field arithmetic: tests/test_hash_to_group_host.py runs the same
// code on the CPU against hashlib.
#pragma once
#include <stdint.h>

#include "fe25519.h"

namespace cpz {

CPZ_HD uint64_t sha512_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// Byte `pos` of the padded message: the message, 0x80, zeros, then the bit length as a 128-bit
// big-endian number in the last 16 bytes of the last block (`total` bytes in all; len < 2^61).
CPZ_HD uint32_t sha512_padded_byte(const uint8_t* msg, uint64_t len, uint64_t total, uint64_t pos) {
  if (pos < len) return msg[pos];
  if (pos == len) return 0x80u;
  if (pos + 8 >= total) return (uint32_t)(((len << 3) >> (8 * (total - 1 - pos))) & 0xffu);
  return 0u;
}

// One block: the schedule W (16 words, in place) into the state.
CPZ_HD void sha512_block(uint64_t st[8], uint64_t w[16]) {
  constexpr uint64_t K[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
      0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
      0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
      0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
      0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
      0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
      0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
      0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
      0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
      0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
      0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
      0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
      0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
  uint64_t v[8];
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = st[i];
  // round t keeps a..h at v[(0 - t) & 7] .. v[(7 - t) & 7]: the rotation of the working variables
  // is a renaming, and t is a constant in every unrolled round
#pragma unroll
  for (int t = 0; t < 80; t++) {
    if (t >= 16) {
      const uint64_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
      w[t & 15] += (sha512_rotr(w15, 1) ^ sha512_rotr(w15, 8) ^ (w15 >> 7)) + w[(t - 7) & 15] +
                   (sha512_rotr(w2, 19) ^ sha512_rotr(w2, 61) ^ (w2 >> 6));
    }
    const uint64_t a = v[(0 - t) & 7], b = v[(1 - t) & 7], c = v[(2 - t) & 7];
    const uint64_t e = v[(4 - t) & 7], f = v[(5 - t) & 7], g = v[(6 - t) & 7];
    const uint64_t t1 = v[(7 - t) & 7] + (sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41)) +
                        ((e & f) ^ (~e & g)) + K[t] + w[t & 15];
    const uint64_t t2 = (sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
    v[(3 - t) & 7] += t1;       // d becomes the next round's e
    v[(7 - t) & 7] = t1 + t2;   // h's slot holds the next round's a
  }
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] += v[i];
}

// SHA-512 of msg[0 .. len): the eight state words (the digest is their big-endian bytes).
CPZ_HD void sha512_state(uint64_t st[8], const uint8_t* msg, uint64_t len) {
  st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull;
  st[3] = 0xa54ff53a5f1d36f1ull; st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full;
  st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
  // the message, one 0x80 byte and the 16-byte length, rounded up to whole blocks
  const uint64_t total = (len + 17 + 127) / 128 * 128;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint64_t base = 0; base < total; base += 128) {
    uint64_t w[16];
    if (base + 128 <= len) {  // a block of message bytes alone
#pragma unroll
      for (int j = 0; j < 16; j++) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) x = (x << 8) | msg[base + 8 * j + k];
        w[j] = x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) x = (x << 8) | sha512_padded_byte(msg, len, total, base + 8 * j + k);
        w[j] = x;
      }
    }
    sha512_block(st, w);
  }
}

CPZ_HD uint32_t sha512_bswap32(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

// The digest as 16 little-endian words of its 64 bytes: the two 32-byte halves are then the
// word rows fe_fromwords reads (elligator.h).
CPZ_HD void sha512_words(uint32_t out[16], const uint8_t* msg, uint64_t len) {
  uint64_t st[8];
  sha512_state(st, msg, len);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[2 * i] = sha512_bswap32((uint32_t)(st[i] >> 32));
    out[2 * i + 1] = sha512_bswap32((uint32_t)st[i]);
  }
}

}  // namespace cpz
