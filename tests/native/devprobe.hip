// Test-only device probes: the product's device-only arithmetic, one operation per launch.
//
// csrc/fe16.h (16-lane row field and point arithmetic), csrc/keccak_wave.h (wave-spread
// Keccak) and the device arm of sc_half_split32<true> (csrc/scalar25519.h) cannot be compiled
// for a CPU, so tests/native/hostlib.cpp never reaches them.  This unit includes those headers
// unchanged and exports plain C entry points over host pointers; tests/test_gpu_row_arith.py
// compares what they return with Python big integers and the Python oracle.  Every entry point
// allocates, copies in, launches once, synchronises, copies back, frees, and returns the
// hipError_t.  Every kernel is one wave per workgroup with all 64 lanes active (the DPP /
// permlane code and sc_half_split32<true> need that); indices past n are clamped for the loads
// and only the stores are guarded.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fe25519.h"
#include "ristretto.h"
#include "scalar25519.h"
#include "transcript.h"
#include "fe16.h"
#include "keccak_wave.h"

using namespace cpz;

namespace {

// ---- r16::mul (a different element on each row) / r16::mul_pair (one element per row pair) ----
template <bool kPair>
__global__ void __launch_bounds__(64) k_row_mul(int n, const int32_t* x, const int32_t* y, int32_t* out) {
  const r16::Lane L = r16::lane_of((int)threadIdx.x);
  // mul: element 4 b + row -> out[e][16]; mul_pair: element 2 b + row / 2 -> out[e][row & 1][16]
  const int e = kPair ? 2 * (int)blockIdx.x + (L.row >> 1) : 4 * (int)blockIdx.x + L.row;
  const int ec = e < n ? e : n - 1;
  const int xv = x[16 * ec + L.k], yv = y[16 * ec + L.k];
  const int r = kPair ? r16::mul_pair(xv, yv, L) : r16::mul(xv, yv, L);
  if (e < n) out[kPair ? (32 * e + 16 * (L.row & 1) + L.k) : (16 * e + L.k)] = r;
}

// ---- r16::to_words, is_zero, is_negative: one element per wave, on every row ------------------
// out[e][row][10]: 8 words, is_zero, is_negative; row r's answer is taken from lane 5 r of the row
__global__ void __launch_bounds__(64) k_row_words(const int32_t* x, uint32_t* out) {
  const r16::Lane L = r16::lane_of((int)threadIdx.x);
  const int e = (int)blockIdx.x;
  const int xv = x[16 * e + L.k];
  uint32_t w[8];
  r16::to_words(w, xv);
  const bool z = r16::is_zero(xv), ng = r16::is_negative(xv);
  if (L.k == 5 * L.row) {
    uint32_t* o = out + 40 * e + 10 * L.row;
    for (int i = 0; i < 8; i++) o[i] = w[i];
    o[8] = z ? 1u : 0u;
    o[9] = ng ? 1u : 0u;
  }
}

// ---- r16::invsqrt_m1: out[e][row][17] = was_square, 16 limbs ------------------------------------
__global__ void __launch_bounds__(64) k_row_invsqrt(const int32_t* v, int32_t* out) {
  const r16::Lane L = r16::lane_of((int)threadIdx.x);
  const int e = (int)blockIdx.x;
  int r;
  const bool sq = r16::invsqrt_m1(r, v[16 * e + L.k], L);
  int32_t* o = out + 68 * e + 17 * L.row;
  if (L.k == 0) o[0] = sq ? 1 : 0;
  o[1 + L.k] = r;
}

__device__ __forceinline__ void store_p4(int32_t* o, const r16::P4& p, const r16::Lane& L) {
  o[L.k] = p.X;
  o[16 + L.k] = p.Y;
  o[32 + L.k] = p.Z;
  o[48 + L.k] = p.T;
}

__device__ __forceinline__ bool decode_at(r16::P4& p, const uint32_t* enc, int e, const r16::Lane& L) {
  uint32_t wu[8];
  for (int i = 0; i < 8; i++) wu[i] = enc[8 * e + i];
  return r16::decode(p, enc + 8 * e, wu, L);
}

// ---- r16::decode: out[e][row][65] = ok, X, Y, Z, T limbs ------------------------------------------
__global__ void __launch_bounds__(64) k_row_decode(const uint32_t* enc, int32_t* out) {
  const r16::Lane L = r16::lane_of((int)threadIdx.x);
  const int e = (int)blockIdx.x;
  r16::P4 p;
  const bool ok = decode_at(p, enc, e, L);
  int32_t* o = out + 260 * e + 65 * L.row;
  if (L.k == 0) o[0] = ok ? 1 : 0;
  store_p4(o + 1, p, L);
}

// ---- point operations: out[e][row][kPointWords] ------------------------------------------------------
// words 0..3: both decoded, is_identity(A - A), is_identity(A + B), 0; then six points of 64 limbs:
// 2 A, A + B, A - B, -A, A - A, and the chain: round r = (four doublings when r > 0, then
// + B, + A, - B, - A for r mod 4 = 0, 1, 2, 3) -- k_verify_wide's Straus loop shape, so the operands
// reach the looseness the kernel feeds back.
constexpr int kPointWords = 4 + 6 * 64;
__global__ void __launch_bounds__(64) k_row_point(const uint32_t* encA, const uint32_t* encB, int rounds,
                                                  int32_t* out) {
  const r16::Lane L = r16::lane_of((int)threadIdx.x);
  const int e = (int)blockIdx.x;
  r16::P4 A, B;
  const bool okA = decode_at(A, encA, e, L);
  const bool okB = decode_at(B, encB, e, L);
  const r16::C4 cA = r16::to_cached(A, L), cB = r16::to_cached(B, L);
  const r16::P4 d = r16::dbl(A, L);
  const r16::P4 s = r16::add_b(A, r16::cached_b(cB, false, L), L);
  const r16::P4 m = r16::add_b(A, r16::cached_b(cB, true, L), L);
  const r16::P4 na = r16::neg(A);
  const r16::P4 z = r16::add_b(A, r16::cached_b(cA, true, L), L);
  r16::P4 acc = r16::identity(L);
#pragma unroll 1
  for (int r = 0; r < rounds; r++) {
    if (r > 0) {
      acc = r16::dbl(acc, L);
      acc = r16::dbl(acc, L);
      acc = r16::dbl(acc, L);
      acc = r16::dbl(acc, L);
    }
    const bool useA = (r & 1) != 0, ng = (r & 2) != 0;
    const int bA = r16::cached_b(cA, ng, L), bB = r16::cached_b(cB, ng, L);
    acc = r16::add_b(acc, useA ? bA : bB, L);
  }
  const bool idz = r16::is_identity(z), ids = r16::is_identity(s);
  int32_t* o = out + (4 * e + L.row) * kPointWords;
  if (L.k == 0) {
    o[0] = (okA && okB) ? 1 : 0;
    o[1] = idz ? 1 : 0;
    o[2] = ids ? 1 : 0;
    o[3] = 0;
  }
  store_p4(o + 4, d, L);
  store_p4(o + 4 + 64, s, L);
  store_p4(o + 4 + 128, m, L);
  store_p4(o + 4 + 192, na, L);
  store_p4(o + 4 + 256, z, L);
  store_p4(o + 4 + 320, acc, L);
}

// ---- the challenge split: one challenge per wave, every lane the same words -----------------------
// which = 0: sc_half_split32<true>, 1: sc_half_split32<false>, 2: sc_half_split
// out[e][2][9]: u (4 words), |v| (4 words), sign, as lane 0 and as lane 63 hold them
template <int kWhich>
__global__ void __launch_bounds__(64) k_split(const uint32_t* c, uint32_t* out) {
  const int e = (int)blockIdx.x;
  uint32_t cw[8], u[4], va[4];
  for (int i = 0; i < 8; i++) cw[i] = c[8 * e + i];
  bool vneg;
  if constexpr (kWhich == 0)
    sc_half_split32<true>(cw, u, va, vneg);
  else if constexpr (kWhich == 1)
    sc_half_split32<false>(cw, u, va, vneg);
  else
    sc_half_split(cw, u, va, vneg);
  if (threadIdx.x == 0 || threadIdx.x == 63) {
    uint32_t* o = out + 18 * e + (threadIdx.x == 0 ? 0 : 9);
    for (int i = 0; i < 4; i++) {
      o[i] = u[i];
      o[4 + i] = va[i];
    }
    o[8] = vneg ? 1u : 0u;
  }
}

// ---- PermRows on a 50-word image: out[e][2][50] as lane 0 and as lane 63 see it -------------------
__global__ void __launch_bounds__(64) k_keccak(const uint32_t* state, uint32_t* out) {
  __shared__ uint32_t lds[50];
  const int e = (int)blockIdx.x;
  uint32_t st[50];
  for (int k = 0; k < 50; k++) st[k] = state[50 * e + k];
  PermRows{lds, (int)threadIdx.x}(st);
  if (threadIdx.x == 0 || threadIdx.x == 63) {
    uint32_t* o = out + 100 * e + (threadIdx.x == 0 ? 0 : 50);
    for (int k = 0; k < 50; k++) o[k] = st[k];
  }
}

// ---- per-lane field arithmetic (fe25519.h as gfx950 compiles it): out[e][5][32] bytes --------------
// fe_mul(a, b), fe_sq(a), fe_sq2(a), fe_add(a, b), fe_sub(a, b), each through fe_tobytes
__global__ void __launch_bounds__(64) k_fe(int n, const uint32_t* a, const uint32_t* b, uint8_t* out) {
  const int e = (int)(blockIdx.x * 64 + threadIdx.x);
  const int ec = e < n ? e : n - 1;
  uint32_t aw[8], bw[8];
  for (int i = 0; i < 8; i++) {
    aw[i] = a[8 * ec + i];
    bw[i] = b[8 * ec + i];
  }
  const fe fa = fe_fromwords(aw), fb = fe_fromwords(bw);
  const fe r[5] = {fe_mul(fa, fb), fe_sq(fa), fe_sq2(fa), fe_add(fa, fb), fe_sub(fa, fb)};
  if (e >= n) return;
  for (int j = 0; j < 5; j++) {
    uint8_t s[32];
    fe_tobytes(s, r[j]);
    for (int i = 0; i < 32; i++) out[160 * (size_t)e + 32 * j + i] = s[i];
  }
}

// Device copies of host buffers for one launch; everything is freed by the destructor.
struct Buffers {
  static constexpr int kMax = 4;
  void* dev[kMax] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t err = hipSuccess;
  int used = 0;
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = out<T>(count);
    if (err == hipSuccess) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t count) {
    if (err != hipSuccess || used == kMax) {
      if (err == hipSuccess) err = hipErrorOutOfMemory;
      return nullptr;
    }
    err = hipMalloc(&dev[used], count * sizeof(T));
    if (err == hipSuccess) err = hipMemset(dev[used], 0, count * sizeof(T));
    return err == hipSuccess ? static_cast<T*>(dev[used++]) : nullptr;
  }
  // after the launch: wait, copy `count` elements back, report the first error
  template <class T>
  int finish(T* host, const T* d, size_t count) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost);
    return (int)err;
  }
  ~Buffers() {
    for (int i = 0; i < used; i++) (void)hipFree(dev[i]);
  }
};

}  // namespace

extern "C" {

// x, y: int32[n][16] raw limbs.  pair = 0: out int32[n][16] (r16::mul); pair = 1: out
// int32[n][2][16] (r16::mul_pair, both rows of the pair).
int probe_row_mul(int n, const int32_t* x, const int32_t* y, int pair, int32_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const size_t no = (size_t)n * (pair ? 32 : 16);
  const int32_t* dx = b.in(x, (size_t)n * 16);
  const int32_t* dy = b.in(y, (size_t)n * 16);
  int32_t* dout = b.out<int32_t>(no);
  if (b.err == hipSuccess) {
    if (pair)
      k_row_mul<true><<<(n + 1) / 2, 64>>>(n, dx, dy, dout);
    else
      k_row_mul<false><<<(n + 3) / 4, 64>>>(n, dx, dy, dout);
  }
  return b.finish(out, dout, no);
}

// x: int32[n][16]; out: uint32[n][4][10]
int probe_row_words(int n, const int32_t* x, uint32_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const int32_t* dx = b.in(x, (size_t)n * 16);
  uint32_t* dout = b.out<uint32_t>((size_t)n * 40);
  if (b.err == hipSuccess) k_row_words<<<n, 64>>>(dx, dout);
  return b.finish(out, dout, (size_t)n * 40);
}

// v: int32[n][16]; out: int32[n][4][17]
int probe_row_invsqrt(int n, const int32_t* v, int32_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const int32_t* dv = b.in(v, (size_t)n * 16);
  int32_t* dout = b.out<int32_t>((size_t)n * 68);
  if (b.err == hipSuccess) k_row_invsqrt<<<n, 64>>>(dv, dout);
  return b.finish(out, dout, (size_t)n * 68);
}

// enc: uint32[n][8] (32-byte encodings); out: int32[n][4][65]
int probe_row_decode(int n, const uint32_t* enc, int32_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const uint32_t* de = b.in(enc, (size_t)n * 8);
  int32_t* dout = b.out<int32_t>((size_t)n * 260);
  if (b.err == hipSuccess) k_row_decode<<<n, 64>>>(de, dout);
  return b.finish(out, dout, (size_t)n * 260);
}

// encA, encB: uint32[n][8]; out: int32[n][4][4 + 6 * 64]
int probe_row_point(int n, const uint32_t* encA, const uint32_t* encB, int rounds, int32_t* out) {
  if (n <= 0 || rounds < 0 || rounds > 64) return (int)hipErrorInvalidValue;
  Buffers b;
  const uint32_t* da = b.in(encA, (size_t)n * 8);
  const uint32_t* db = b.in(encB, (size_t)n * 8);
  int32_t* dout = b.out<int32_t>((size_t)n * 4 * kPointWords);
  if (b.err == hipSuccess) k_row_point<<<n, 64>>>(da, db, rounds, dout);
  return b.finish(out, dout, (size_t)n * 4 * kPointWords);
}

// c: uint32[n][8] canonical challenges; out: uint32[n][2][9]
int probe_split(int n, const uint32_t* c, int which, uint32_t* out) {
  if (n <= 0 || which < 0 || which > 2) return (int)hipErrorInvalidValue;
  Buffers b;
  const uint32_t* dc = b.in(c, (size_t)n * 8);
  uint32_t* dout = b.out<uint32_t>((size_t)n * 18);
  if (b.err == hipSuccess) {
    if (which == 0)
      k_split<0><<<n, 64>>>(dc, dout);
    else if (which == 1)
      k_split<1><<<n, 64>>>(dc, dout);
    else
      k_split<2><<<n, 64>>>(dc, dout);
  }
  return b.finish(out, dout, (size_t)n * 18);
}

// state: uint32[n][50]; out: uint32[n][2][50]
int probe_keccak(int n, const uint32_t* state, uint32_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const uint32_t* ds = b.in(state, (size_t)n * 50);
  uint32_t* dout = b.out<uint32_t>((size_t)n * 100);
  if (b.err == hipSuccess) k_keccak<<<n, 64>>>(ds, dout);
  return b.finish(out, dout, (size_t)n * 100);
}

// a, b: uint32[n][8]; out: uint8[n][5][32]
int probe_fe(int n, const uint32_t* a, const uint32_t* bb, uint8_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const uint32_t* da = b.in(a, (size_t)n * 8);
  const uint32_t* db = b.in(bb, (size_t)n * 8);
  uint8_t* dout = b.out<uint8_t>((size_t)n * 160);
  if (b.err == hipSuccess) k_fe<<<(n + 63) / 64, 64>>>(n, da, db, dout);
  return b.finish(out, dout, (size_t)n * 160);
}

}  // extern "C"
