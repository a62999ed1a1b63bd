// Test-only probes of the RLC batch check's prepare stage and of the device scalar arithmetic
// (csrc/rlc.hip, rlc_dev.h, scalar25519.h) on hand-made inputs.
//
// The public ABI reaches the prepare only inside whole batch checks on proofs it made itself, whose
// one observable is a 32-byte partial or a status list.  This unit includes rlc.hip textually and
// unchanged, so that its kernels are visible, and exports plain C entry points over host pointers:
// either prepare kernel (one lane or four lanes per proof, single-pair or pair mode) or the
// library's own launcher on a caller's rows, seed, first index and response statuses;
// k_rlc_extra on a caller's block sums; k_rlc_extra_pairs on a caller's products and pair indices;
// and sc_mul, sc_add, sc_neg, sc_reduce_wide, sc_is_canonical, rlc_weight and recode16 one lane
// per vector.  tests/test_gpu_prep_probe.py compares what they return with Python integers
// (tests/prep_model.py, tests/scalar_vectors.py) and the Python oracle.  Every entry point
// allocates, copies in, launches, synchronises, copies back, frees, and returns the hipError_t;
// every device buffer is filled with 0xff first, so an unwritten slot shows.  Never linked into
// the product library.
#include "rlc.hip"

using namespace cpz;

namespace {

// one lane per vector; out is 8 words per vector whatever the operation (unused words stay 0xff)
__global__ void __launch_bounds__(64) k_probe_scalar(int op, int64_t m, const uint32_t* a, const uint32_t* b,
                                                     uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= m) return;
  uint32_t* o = out + 8 * i;
  if (op == 3) {  // sc_reduce_wide: 16 words in
    uint32_t x[16];
    for (int k = 0; k < 16; k++) x[k] = a[16 * i + k];
    const sc r = sc_reduce_wide(x);
    for (int k = 0; k < 8; k++) o[k] = r.w[k];
    return;
  }
  if (op == 5) {  // rlc_weight: 4 words in
    uint32_t u[4];
    for (int k = 0; k < 4; k++) u[k] = a[4 * i + k];
    const sc r = rlc_weight(u);
    for (int k = 0; k < 8; k++) o[k] = r.w[k];
    return;
  }
  sc x, y, r;
  for (int k = 0; k < 8; k++) {
    x.w[k] = a[8 * i + k];
    y.w[k] = op < 2 ? b[8 * i + k] : 0u;
  }
  if (op == 0) {
    r = sc_mul(x, y);
  } else if (op == 1) {
    r = sc_add(x, y);
  } else if (op == 2) {
    r = sc_neg(x);
  } else if (op == 4) {
    o[0] = sc_is_canonical(x.w) ? 1u : 0u;
    return;
  } else {  // 6: recode16, digit w in half w % 2 of word w / 2
    int16_t d[kRlcWindows];
    recode16(d, x.w);
    for (int k = 0; k < 8; k++) r.w[k] = (uint32_t)(uint16_t)d[2 * k] | ((uint32_t)(uint16_t)d[2 * k + 1] << 16);
  }
  for (int k = 0; k < 8; k++) o[k] = r.w[k];
}

// Device buffers of one entry point; everything is freed by the destructor.
struct Pool {
  static constexpr int kMax = 32;
  void* dev[kMax];
  hipError_t err = hipSuccess;
  int used = 0;
  template <class T>
  T* out(size_t count) {  // 0xff-filled
    if (count == 0) count = 1;
    if (err != hipSuccess || used == kMax) {
      if (err == hipSuccess) err = hipErrorOutOfMemory;
      return nullptr;
    }
    err = hipMalloc(&dev[used], count * sizeof(T));
    if (err != hipSuccess) return nullptr;
    used++;
    err = hipMemset(dev[used - 1], 0xff, count * sizeof(T));
    return err == hipSuccess ? static_cast<T*>(dev[used - 1]) : nullptr;
  }
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = out<T>(count);
    if (err == hipSuccess && count) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  template <class T>
  void back(T* host, const T* d, size_t count) {
    if (err == hipSuccess && count) err = hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  void step(hipError_t e) {
    if (err == hipSuccess) err = e;
  }
  ~Pool() {
    for (int i = 0; i < used; i++) (void)hipFree(dev[i]);
  }
};

constexpr int64_t kProbeMaxProofs = 1 << 17;   // bounds the probe's buffers (the tests stop at 32,769)
constexpr int64_t kProbeMaxStride = 1 << 20;   // digit columns of the extras' entry points
constexpr int64_t kProbeMaxSums = 1 << 16;
constexpr int64_t kProbeMaxVectors = 1 << 20;

// the runtime's rounding of the digit rows (4 n points, 4 extra slots, whole 16-byte loads), and
// eight spare columns that nothing may write
int64_t dstride_of(int64_t n) { return ((4 * n + 4 + 7) & ~(int64_t)7) + 8; }

}  // namespace

extern "C" {

// The constants the tests need, by index (tests/prep_model.py names them).
long long prepprobe_const(int which) {
  switch (which) {
    case 0: return kRlcWindows;
    case 1: return kRlcPrepBlock;
    case 2: return kRlcSumBlock;
    case 3: return kRlcPrepWideMax;
    case 4: return kNielsEntriesRlc;
    case 5: return (long long)sizeof(ge_niels);
    case 6: return kStOk;
    case 7: return kStEqFail;
    case 8: return kStBadPoint;
    case 9: return kStBadScalar;
    case 10: return kStIdentity;
    case 11: return kStZeroS;
    case 12: return kStBadChallenge;
    default: return -1;
  }
}

long long prepprobe_dstride(long long n) { return n >= 1 && n <= kProbeMaxProofs ? dstride_of(n) : -1; }

// One prepare of n proofs.
//   form   0: the one-lane kernel (k_rlc_prepare / k_rlc_prepare_pairs) launched directly at any n
//          1: the four-lane kernel (k_rlc_prepare4 + k_rlc_bsum4, or k_rlc_prepare4_pairs)
//          2: the library's launcher (launch_rlc_prepare / launch_rlc_prepare_pairs)
//   pairs  0 / 1: single-pair or pair mode
//   seed uint32[8]; y1, y2, r1, r2, s, c uint32[n][8]; status_in uint8[n]
// Out (all 0xff-filled before the launch except any_bad, which is zeroed as the runtime zeroes it):
//   status uint8[n], pts ge_niels[4 n], digits int16[16][prepprobe_dstride(n)],
//   block_sums uint32[2 ceil(n / 256)][2][8], prod uint32[n][2][8], quarter_sums
//   uint32[ceil(n / 64)][2][8], any_bad int[1].  Every buffer is handed to the kernels in both
//   modes, so what a mode must not touch comes back 0xff.
int prepprobe_prepare(int form, int pairs, long long n, unsigned long long first_index, const uint32_t* seed,
                      const uint32_t* y1, const uint32_t* y2, const uint32_t* r1, const uint32_t* r2,
                      const uint32_t* s, const uint32_t* c, const uint8_t* status_in, int eq_only,
                      uint8_t* status_out, void* pts_out, int16_t* digits_out, uint32_t* block_sums_out,
                      uint32_t* prod_out, uint32_t* quarter_out, int* any_bad_out) {
  if (form < 0 || form > 2 || (pairs != 0 && pairs != 1) || n < 1 || n > kProbeMaxProofs || !seed || !y1 || !y2 ||
      !r1 || !r2 || !s || !c || !status_in || !status_out || !pts_out || !digits_out || !block_sums_out ||
      !prod_out || !quarter_out || !any_bad_out || (eq_only != 0 && eq_only != 1))
    return (int)hipErrorInvalidValue;
  const int64_t blocks = (n + kRlcPrepBlock - 1) / kRlcPrepBlock, nq = (n + 63) / 64;
  Pool p;
  RlcPrepArgs a{};
  a.n = n;
  a.first_index = first_index;
  for (int k = 0; k < 8; k++) a.seed[k] = seed[k];
  a.y1 = p.in(y1, (size_t)n * 8);
  a.y2 = p.in(y2, (size_t)n * 8);
  a.r1 = p.in(r1, (size_t)n * 8);
  a.r2 = p.in(r2, (size_t)n * 8);
  a.s = p.in(s, (size_t)n * 8);
  a.c = p.in(c, (size_t)n * 8);
  a.status = p.in(status_in, (size_t)n);
  a.pts = p.out<ge_niels>((size_t)4 * n);
  a.dstride = dstride_of(n);
  a.digits = p.out<int16_t>((size_t)kRlcWindows * a.dstride);
  a.block_sums = p.out<sc>((size_t)4 * blocks);
  a.quarter_sums = p.out<sc>((size_t)2 * nq);
  a.prod = p.out<sc>((size_t)2 * n);
  a.any_bad = p.out<int>(1);
  a.eq_only = eq_only;
  if (p.err != hipSuccess) return (int)p.err;
  p.step(hipMemset(a.any_bad, 0, sizeof(int)));
  if (p.err != hipSuccess) return (int)p.err;
  if (form == 2) {
    p.step(pairs ? launch_rlc_prepare_pairs(a, nullptr) : launch_rlc_prepare(a, nullptr));
  } else if (form == 0) {
    if (pairs)
      hipLaunchKernelGGL(k_rlc_prepare_pairs, dim3((unsigned)blocks), dim3(kRlcPrepBlock), 0, nullptr, a);
    else
      hipLaunchKernelGGL(k_rlc_prepare, dim3((unsigned)blocks), dim3(kRlcPrepBlock), 0, nullptr, a);
  } else if (pairs) {
    hipLaunchKernelGGL(k_rlc_prepare4_pairs, dim3((unsigned)nq), dim3(256), 0, nullptr, a);
  } else {
    hipLaunchKernelGGL(k_rlc_prepare4, dim3((unsigned)nq), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_rlc_bsum4, dim3((unsigned)((4 * blocks + 63) / 64)), dim3(64), 0, nullptr, a.quarter_sums,
                       nq, a.block_sums, 2 * blocks);
  }
  p.sync();
  p.back(status_out, a.status, (size_t)n);
  p.back(static_cast<ge_niels*>(pts_out), a.pts, (size_t)4 * n);
  p.back(digits_out, a.digits, (size_t)kRlcWindows * a.dstride);
  p.back(reinterpret_cast<sc*>(block_sums_out), a.block_sums, (size_t)4 * blocks);
  p.back(reinterpret_cast<sc*>(prod_out), a.prod, (size_t)2 * n);
  p.back(reinterpret_cast<sc*>(quarter_out), a.quarter_sums, (size_t)2 * nq);
  p.back(any_bad_out, a.any_bad, 1);
  return (int)p.err;
}

// k_rlc_extra over block_sums uint32[nsum][2][8], sum blocks [b0, b1), the two points at columns
// e0, e0 + 1 of digits int16[16][dstride].  g_niels / h_niels are sizeof(ge_niels) bytes each, laid
// at entries 0 and kNielsEntriesRlc of a 0xff-filled table of 2 kNielsEntriesRlc entries.
// Out: pts ge_niels[2] (entries e0, e0 + 1), digits int16[16][dstride] whole.
int prepprobe_extra(long long nsum, const uint32_t* block_sums, long long b0, long long b1, long long e0,
                    long long dstride, const void* g_niels, const void* h_niels, void* pts_out,
                    int16_t* digits_out) {
  if (nsum < 1 || nsum > kProbeMaxSums || !block_sums || b0 < 0 || b1 < b0 || b1 > nsum || e0 < 0 ||
      dstride > kProbeMaxStride || e0 + 2 > dstride || !g_niels || !h_niels || !pts_out || !digits_out)
    return (int)hipErrorInvalidValue;
  Pool p;
  RlcMsmArgs a{};
  a.e0 = e0;
  a.nextra = 2;
  a.dstride = dstride;
  a.pts = p.out<ge_niels>((size_t)e0 + 2);
  a.digits = p.out<int16_t>((size_t)kRlcWindows * dstride);
  const sc* d_sums = p.in(reinterpret_cast<const sc*>(block_sums), (size_t)2 * nsum);
  ge_niels* tab = p.out<ge_niels>((size_t)2 * kNielsEntriesRlc);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(hipMemcpy(tab, g_niels, sizeof(ge_niels), hipMemcpyHostToDevice));
  p.step(hipMemcpy(tab + kNielsEntriesRlc, h_niels, sizeof(ge_niels), hipMemcpyHostToDevice));
  if (p.err != hipSuccess) return (int)p.err;
  hipLaunchKernelGGL(k_rlc_extra, dim3(1), dim3(256), 0, nullptr, a, d_sums, (int64_t)b0, (int64_t)b1, tab);
  p.sync();
  p.back(static_cast<ge_niels*>(pts_out), a.pts + e0, 2);
  p.back(digits_out, a.digits, (size_t)kRlcWindows * dstride);
  return (int)p.err;
}

// k_rlc_extra_pairs over prod uint32[n][2][8] and pair_idx uint32[n], entries [lo, hi), npairs
// workgroups, gh ge_niels[2 npairs]; pair p's points at columns e0 + 2 p, e0 + 2 p + 1.
// Out: pts ge_niels[2 npairs] (entries e0 ..), digits int16[16][dstride] whole.
int prepprobe_extra_pairs(long long n, const uint32_t* prod, const uint32_t* pair_idx, long long lo, long long hi,
                          int npairs, const void* gh, long long e0, long long dstride, void* pts_out,
                          int16_t* digits_out) {
  if (n < 1 || n > kProbeMaxProofs || !prod || !pair_idx || lo < 0 || hi < lo || hi > n || npairs < 1 ||
      npairs > kPairBucketMaxPairs || !gh || e0 < 0 || dstride > kProbeMaxStride || e0 + 2 * npairs > dstride ||
      !pts_out || !digits_out)
    return (int)hipErrorInvalidValue;
  Pool p;
  RlcMsmArgs a{};
  a.e0 = e0;
  a.nextra = 2 * npairs;
  a.dstride = dstride;
  a.pts = p.out<ge_niels>((size_t)e0 + 2 * npairs);
  a.digits = p.out<int16_t>((size_t)kRlcWindows * dstride);
  RlcPairExtra x{};
  x.prod = p.in(reinterpret_cast<const sc*>(prod), (size_t)2 * n);
  x.pair_idx = p.in(pair_idx, (size_t)n);
  x.lo = lo;
  x.hi = hi;
  x.gh = p.in(static_cast<const ge_niels*>(gh), (size_t)2 * npairs);
  x.npairs = npairs;
  if (p.err != hipSuccess) return (int)p.err;
  hipLaunchKernelGGL(k_rlc_extra_pairs, dim3((unsigned)npairs), dim3(256), 0, nullptr, a, x);
  p.sync();
  p.back(static_cast<ge_niels*>(pts_out), a.pts + e0, (size_t)2 * npairs);
  p.back(digits_out, a.digits, (size_t)kRlcWindows * dstride);
  return (int)p.err;
}

// One lane per vector.  op 0: sc_mul(a, b), 1: sc_add(a, b), 2: sc_neg(a), 3: sc_reduce_wide(a),
// a of 16 words, 4: sc_is_canonical(a) in word 0, 5: rlc_weight(a), a of 4 words, 6: recode16(a) as
// 16 int16.  Other inputs are 8 words per vector; out is uint32[m][8], words not written stay 0xff.
int prepprobe_scalar(int op, long long m, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (op < 0 || op > 6 || m < 1 || m > kProbeMaxVectors || !a || (op < 2 && !b) || !out)
    return (int)hipErrorInvalidValue;
  const size_t aw = op == 3 ? 16 : (op == 5 ? 4 : 8);
  Pool p;
  const uint32_t* d_a = p.in(a, (size_t)m * aw);
  const uint32_t* d_b = op < 2 ? p.in(b, (size_t)m * 8) : nullptr;
  uint32_t* d_out = p.out<uint32_t>((size_t)m * 8);
  if (p.err != hipSuccess) return (int)p.err;
  hipLaunchKernelGGL(k_probe_scalar, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, nullptr, op, (int64_t)m, d_a, d_b,
                     d_out);
  p.sync();
  p.back(out, d_out, (size_t)m * 8);
  return (int)p.err;
}

}  // extern "C"
