// Hash-to-group kernels for gfx950: labels -> ristretto255 points, generator_h()'s construction
// (src/primitives/ristretto.rs:27, 86-91) for any number of messages.
//
//   k_sha512_rows    SHA-512 of n messages of a blob, a thread per message (sha512.h)
//   k_from_uniform   RistrettoPoint::from_uniform_bytes of n rows of 64 bytes, encoded
//                    (elligator.h): a lane pair per point
//
// k_from_uniform's shape: the two Elligator maps of a point are independent and each holds a
// whole square-root chain (fe_pow22523, ~250 squarings), as long as the encoding's own.  Lane 2 i
// maps the first half of row i and lane 2 i + 1 the second; one exchange of the 40 limbs
// (__shfl_xor 1) hands each lane its partner's point, then both add and encode and the even lane
// stores.  Two chains deep where a lane per point is three, and twice the lanes for a call of a
// few thousand points, which fills a fraction of the device either way.
//
// Wave safety: no lane leaves before the exchange.  A lane past the last point (odd n, n = 1, the
// last wave's tail) clamps its row to n - 1 and recomputes that point without storing, so every
// lane an exchange reads is active, and was_square is a select inside elligator_map.
#include <hip/hip_runtime.h>

#include "../../include/cpz.h"
#include "cpz_kernels.h"
#include "elligator.h"
#include "sha512.h"

namespace cpz {

// One wave per block: a call of 8192 points is 256 blocks, one per CU.
constexpr int kH2gBlock = 64;

__global__ void __launch_bounds__(kH2gBlock) k_sha512_rows(int64_t n, const uint8_t* blob, const uint64_t* off,
                                                           uint32_t* digest) {
  const int64_t i = (int64_t)blockIdx.x * kH2gBlock + threadIdx.x;
  if (i >= n) return;  // no cross-lane step below
  const uint64_t o0 = off[i], o1 = off[i + 1];
  // the length is clamped: offsets from the device cannot make the block loop unbounded
  const uint64_t len = o1 > o0 ? (o1 - o0 < (uint64_t)CPZ_HASH_MAX_MSG ? o1 - o0 : (uint64_t)CPZ_HASH_MAX_MSG) : 0;
  uint32_t w[16];
  sha512_words(w, blob + o0, len);
  uint4* out = reinterpret_cast<uint4*>(digest + 16 * i);
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

__global__ void __launch_bounds__(kH2gBlock) k_from_uniform(int64_t n, const uint8_t* uniform, uint32_t* points) {
  const int64_t t = (int64_t)blockIdx.x * kH2gBlock + threadIdx.x;
  const int half = (int)(t & 1);
  const bool live = (t >> 1) < n;
  const int64_t i = live ? (t >> 1) : n - 1;  // a tail lane recomputes the last point and stores nothing
  const uint8_t* src = uniform + 64 * i + 32 * half;
  uint32_t w[8];
  if ((reinterpret_cast<uintptr_t>(uniform) & 15u) == 0) {  // the same for every lane
    const uint4 a = reinterpret_cast<const uint4*>(src)[0], b = reinterpret_cast<const uint4*>(src)[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++)
      w[k] = (uint32_t)src[4 * k] | ((uint32_t)src[4 * k + 1] << 8) | ((uint32_t)src[4 * k + 2] << 16) |
             ((uint32_t)src[4 * k + 3] << 24);
  }
  const ge_p3 mine = elligator_map_words(w);
  ge_p3 other;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    other.X.v[k] = __shfl_xor(mine.X.v[k], 1);
    other.Y.v[k] = __shfl_xor(mine.Y.v[k], 1);
    other.Z.v[k] = __shfl_xor(mine.Z.v[k], 1);
    other.T.v[k] = __shfl_xor(mine.T.v[k], 1);
  }
  uint32_t enc[8];
  ristretto_encode(enc, ge_add(mine, other));
  if (live && half == 0) {
    uint4* out = reinterpret_cast<uint4*>(points + 8 * i);
    out[0] = make_uint4(enc[0], enc[1], enc[2], enc[3]);
    out[1] = make_uint4(enc[4], enc[5], enc[6], enc[7]);
  }
}

hipError_t launch_sha512_rows(int64_t n, const uint8_t* blob, const uint64_t* off, uint32_t* digest, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha512_rows, dim3((unsigned)((n + kH2gBlock - 1) / kH2gBlock)), dim3(kH2gBlock), 0, st, n, blob,
                     off, digest);
  return hipGetLastError();
}

hipError_t launch_from_uniform(int64_t n, const uint8_t* uniform, uint32_t* points, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_from_uniform, dim3((unsigned)((2 * n + kH2gBlock - 1) / kH2gBlock)), dim3(kH2gBlock), 0, st, n,
                     uniform, points);
  return hipGetLastError();
}

}  // namespace cpz
