// Test-only probe of the per-pair sums of a mixed-pair batch over more than CPZ_PAIRS_MAX pairs
// (csrc/rlc.hip: k_pair_hist, k_pair_scan, k_pair_scatter, k_pair_unit_sums, k_pair_finish).
//
// The public ABI reaches these kernels only with seed-derived products.  This unit includes
// rlc.hip textually and unchanged and exports one plain C entry point over host pointers: the
// bucketing of a caller's pair indices, then the sums of a caller's products over a range and the
// extras they become.  tests/test_gpu_pairsum_probe.py compares what comes back with Python
// integers mod l (tests/pair_sum_model.py).  The entry point allocates, copies in, launches,
// synchronises, copies back, frees, and returns the hipError_t; every device buffer is filled
// with 0xff first, so an unwritten slot shows.  Never linked into the product library.
#include "rlc.hip"

#include <vector>

using namespace cpz;

namespace {

struct Pool {
  static constexpr int kMax = 16;
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

constexpr int64_t kProbeMaxEntries = 1 << 20;
constexpr int64_t kProbeE0 = 8;  // the extras do not start the point array

}  // namespace

extern "C" {

// 0: kPairSumUnit (U), 1: kPairBucketMaxPairs, 2: sizeof(ge_niels), 3: kRlcWindows, 4: kPairBucketChunk
long long pairsumprobe_const(int which) {
  switch (which) {
    case 0: return kPairSumUnit;
    case 1: return kPairBucketMaxPairs;
    case 2: return (long long)sizeof(ge_niels);
    case 3: return kRlcWindows;
    case 4: return kPairBucketChunk;
    default: return -1;
  }
}

// launch_pair_bucket over pair_idx[0 .. n), then launch_pair_sums over [lo, hi).
//   pair_idx  uint32[n], every value below npairs (checked here: the kernels trust them)
//   prod      uint32[n][2][8]  a_i s_i, b_i s_i, each below l
//   gh        bytes[2 npairs][sizeof(ge_niels)]  any pattern: the kernels copy them
// Out: list uint32[n], start / ustart uint32[npairs + 1], digits int16[kRlcWindows][2 npairs]
// (column 2 p + k: pair p's sum k), pts bytes[2 npairs][sizeof(ge_niels)].
int pairsumprobe_run(long long n, int npairs, const uint32_t* pair_idx, const uint32_t* prod, const uint8_t* gh,
                     long long lo, long long hi, uint32_t* list_out, uint32_t* start_out, uint32_t* ustart_out,
                     int16_t* digits_out, uint8_t* pts_out) {
  if (n < 1 || n > kProbeMaxEntries || npairs < 1 || npairs > kPairBucketMaxPairs || lo < 0 || hi < lo || hi > n ||
      !pair_idx || !prod || !gh || !list_out || !start_out || !ustart_out || !digits_out || !pts_out)
    return (int)hipErrorInvalidValue;
  for (long long i = 0; i < n; i++)
    if (pair_idx[i] >= (uint32_t)npairs) return (int)hipErrorInvalidValue;
  Pool p;
  const size_t np1 = (size_t)npairs + 1;
  const uint32_t* d_idx = p.in(pair_idx, (size_t)n);
  const sc* d_prod = reinterpret_cast<const sc*>(p.in(prod, (size_t)n * 16));
  const ge_niels* d_gh = reinterpret_cast<const ge_niels*>(p.in(gh, (size_t)2 * npairs * sizeof(ge_niels)));
  uint32_t* d_list = p.out<uint32_t>((size_t)n);
  uint32_t* d_start = p.out<uint32_t>(np1);
  uint32_t* d_ustart = p.out<uint32_t>(np1);
  uint32_t* d_cursor = p.out<uint32_t>(np1);
  RlcPairExtra x{};
  x.prod = d_prod;
  x.pair_idx = d_idx;
  x.lo = lo;
  x.hi = hi;
  x.gh = d_gh;
  x.npairs = npairs;
  x.max_units = pair_sum_max_units(n, npairs);
  x.upart = p.out<sc>((size_t)x.max_units * 2);
  RlcMsmArgs a{};
  a.e0 = kProbeE0;
  a.nextra = 2 * npairs;
  a.dstride = (kProbeE0 + 2 * (int64_t)npairs + 7) & ~(int64_t)7;
  a.pts = p.out<ge_niels>((size_t)(kProbeE0 + 2 * npairs));
  a.digits = p.out<int16_t>((size_t)kRlcWindows * a.dstride);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(launch_pair_bucket(d_idx, n, npairs, d_list, d_start, d_ustart, d_cursor, nullptr));
  p.sync();
  p.back(list_out, d_list, (size_t)n);
  p.back(start_out, d_start, np1);
  p.back(ustart_out, d_ustart, np1);
  if (p.err != hipSuccess) return (int)p.err;
  // the sums read through these: they run only on a partition of [0, n) and ids below n
  if (start_out[0] != 0 || start_out[npairs] != (uint32_t)n || ustart_out[0] != 0 ||
      (int64_t)ustart_out[npairs] > x.max_units)
    return (int)hipErrorInvalidValue;
  for (int q = 0; q < npairs; q++)
    if (start_out[q] > start_out[q + 1] ||
        ustart_out[q + 1] - ustart_out[q] != pair_sum_units(start_out[q + 1] - start_out[q]))
      return (int)hipErrorInvalidValue;
  for (long long i = 0; i < n; i++)
    if (list_out[i] >= (uint32_t)n) return (int)hipErrorInvalidValue;
  x.list = d_list;
  x.start = d_start;
  x.ustart = d_ustart;
  p.step(launch_pair_sums(a, x, nullptr));
  p.sync();
  for (int w = 0; w < kRlcWindows; w++)
    p.back(digits_out + (size_t)w * 2 * npairs, a.digits + (size_t)w * a.dstride + kProbeE0, (size_t)2 * npairs);
  p.back(pts_out, reinterpret_cast<const uint8_t*>(a.pts + kProbeE0), (size_t)2 * npairs * sizeof(ge_niels));
  return (int)p.err;
}

}  // extern "C"
