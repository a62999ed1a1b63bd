// Test-only probes of the Pippenger MSM's sort and reduction (csrc/rlc.hip) on hand-made digits.
//
// The public ABI reaches these kernels only with scalars (cpz_msm: p0 = 0, two extras with zero
// digits) or with seed-derived weights (the batch checks).  This unit includes rlc.hip textually
// and unchanged, so that its kernels are visible, and exports plain C entry points over host
// pointers: the sort alone (k_rlc_hist .. k_rlc_fine) on a caller's digit rows, point range and
// extras, and the accumulation and reduction alone (k_rlc_bucket .. both finals) on a caller's
// offsets and sorted ids.  tests/test_gpu_msm_probe.py compares what they return with Python
// integers (tests/msm_model.py) and the Python oracle.  Every entry point allocates, copies in,
// launches, synchronises, copies back, frees, and returns the hipError_t; every device buffer is
// filled with 0xff first, so an unwritten slot shows.  Never linked into the product library.
#include "rlc.hip"

using namespace cpz;

namespace {

// enc[i] -> affine Niels, not negated (k_msm_load's form), at out[i]
__global__ void __launch_bounds__(64) k_probe_decode_niels(int64_t n, const uint32_t* enc, ge_niels* out, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = enc[8 * i + k];
  ge_p3 P;
  if (!ristretto_decode(P, w)) *bad = 1;
  store_niels(out + i, niels_from_p3_affine(P, false));
}

__global__ void __launch_bounds__(64) k_probe_encode(int64_t n, const ge_p3* in, uint32_t* enc) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ristretto_encode(w, load_p3(in + i));
  for (int k = 0; k < 8; k++) enc[8 * i + k] = w[k];
}

// window w's sum from its k_rlc_window_sparse partials (what rlc_final_windows adds on the fly)
__global__ void __launch_bounds__(64) k_probe_sparse_windows(const ge_p3* part, int sgroups, ge_p3* win) {
  const int w = threadIdx.x;
  if (w >= kRlcWindows) return;
  ge_p3 T = load_p3(part + (int64_t)w * kRlcSparseMaxGroups);
  for (int g = 1; g < sgroups; g++) T = ge_add(T, load_p3(part + (int64_t)w * kRlcSparseMaxGroups + g));
  store_p3(win + w, T);
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

unsigned grid64(int64_t n) { return (unsigned)((n + 63) / 64); }

constexpr int64_t kProbeMaxPoints = 1 << 20;  // far below kRlcMaxMsmPoints; bounds the probe's buffers

// the range checks both entry points share: a point range, then the extras at or after its end
bool ranges_ok(long long np, long long nextra, long long p0, long long e0) {
  return np >= 0 && nextra >= 0 && np + nextra >= 1 && np + nextra <= kProbeMaxPoints && p0 >= 0 &&
         e0 >= p0 + np && e0 + nextra <= 4 * kProbeMaxPoints;
}

int64_t istride_of(int64_t npts) { return (npts + 4095) & ~(int64_t)4095; }

}  // namespace

extern "C" {

// The constants the tests need, by index (tests/msm_model.py names them).
long long msmprobe_const(int which) {
  switch (which) {
    case 0: return kRlcWindows;
    case 1: return kRlcBuckets;
    case 2: return kRlcSegLen;
    case 3: return kRlcSortBlock;
    case 4: return kRlcSortGroups;
    case 5: return kRlcSortChunk;
    case 6: return kRlcChunk;
    case 7: return kRlcMinChunk;
    case 8: return kRlcMinHeads;
    case 9: return kRlcSparsePts;
    case 10: return kRlcCoarse;
    case 11: return kRlcTile;
    case 12: return kRlcFineCap;
    case 13: return kRlcWinQuads;
    case 14: return kRlcSparseMaxGroups;
    default: return -1;
  }
}

// rlc_sort_geometry(npts): out = groups, chunk, echunk.  Host only.
int msmprobe_geometry(long long npts, long long* out) {
  if (npts < 1 || !out) return (int)hipErrorInvalidValue;
  RlcMsmArgs a{};
  rlc_sort_geometry(a, npts);
  out[0] = a.groups;
  out[1] = a.chunk;
  out[2] = a.echunk;
  return 0;
}

// The digit rows' stride both entry points assume: the last row position used, rounded up to
// whole 16-byte loads.
long long msmprobe_dstride(long long np, long long nextra, long long p0, long long e0) {
  (void)np;
  (void)p0;
  return (e0 + nextra + 7) & ~7ll;
}

// The sort alone: k_rlc_hist, k_rlc_bscan, k_rlc_scan, k_rlc_coarse, k_rlc_fine over the np points
// at p0.. and the nextra extras at e0.. of
//   digits   int16[16][dstride], dstride = msmprobe_dstride(..)
// k_rlc_extra is never launched: the extras' digits are the caller's.
// Out: offsets uint32[16][kRlcBuckets + 1], idx uint32[16][np + nextra] (each row's first
// offsets[w][kRlcBuckets] entries are the sorted ids; the rest stay 0xffffffff).
int msmprobe_sort(long long np, long long nextra, long long p0, long long e0, const int16_t* digits,
                  uint32_t* offsets_out, uint32_t* idx_out) {
  if (!ranges_ok(np, nextra, p0, e0) || !digits || !offsets_out || !idx_out) return (int)hipErrorInvalidValue;
  const int64_t npts = np + nextra;
  Pool p;
  RlcMsmArgs a{};
  a.p0 = p0;
  a.p1 = p0 + np;
  a.e0 = e0;
  a.nextra = (int)nextra;
  a.pts = nullptr;  // the sort reads digits only
  a.dstride = msmprobe_dstride(np, nextra, p0, e0);
  a.digits = const_cast<int16_t*>(p.in(digits, (size_t)kRlcWindows * a.dstride));
  rlc_sort_geometry(a, npts);
  if ((int64_t)a.groups * a.chunk < npts || a.groups > kRlcSortGroups) return (int)hipErrorInvalidValue;
  a.istride = istride_of(npts);
  a.counts = p.out<uint32_t>((size_t)kRlcWindows * kRlcBuckets);
  a.offsets = p.out<uint32_t>((size_t)kRlcWindows * (kRlcBuckets + 1));
  a.bhist = p.out<uint32_t>((size_t)kRlcWindows * a.groups * kRlcBuckets);
  a.idx = p.out<uint32_t>((size_t)kRlcWindows * a.istride);
  a.inter = p.out<uint32_t>((size_t)kRlcWindows * a.istride);
  if (p.err != hipSuccess) return (int)p.err;
  const size_t lds = sizeof(uint32_t) * kRlcBuckets;
  p.step(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rlc_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds));
  const int64_t nb = (int64_t)kRlcWindows * kRlcBuckets;
  if (p.err == hipSuccess) {
    hipLaunchKernelGGL(k_rlc_hist, dim3(a.groups, kRlcWindows), dim3(kRlcSortBlock), lds, nullptr, a);
    hipLaunchKernelGGL(k_rlc_bscan, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_rlc_scan, dim3(kRlcWindows), dim3(1024), 0, nullptr, a);
  }
  p.sync();
  // The scatter writes through these offsets: it runs only if they stay inside the rows.
  {
    static_assert(sizeof(uint32_t) == 4, "");
    uint32_t* h = offsets_out;
    p.back(h, a.offsets, (size_t)kRlcWindows * (kRlcBuckets + 1));
    if (p.err != hipSuccess) return (int)p.err;
    for (int w = 0; w < kRlcWindows; w++) {
      const uint32_t* o = h + (size_t)w * (kRlcBuckets + 1);
      if (o[0] != 0 || o[kRlcBuckets] > (uint32_t)npts) return (int)hipErrorInvalidValue;
      for (int b = 0; b < kRlcBuckets; b++)
        if (o[b] > o[b + 1]) return (int)hipErrorInvalidValue;
    }
  }
  hipLaunchKernelGGL(k_rlc_coarse, dim3(a.groups, kRlcWindows), dim3(kRlcSortBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rlc_fine, dim3(kRlcCoarse, kRlcWindows), dim3(kRlcSortBlock), 0, nullptr, a);
  p.sync();
  for (int w = 0; w < kRlcWindows; w++)
    p.back(idx_out + (size_t)w * npts, a.idx + (size_t)w * a.istride, (size_t)npts);
  return (int)p.err;
}

// The accumulation and reduction alone, on offsets and sorted ids from the host.
//   enc       uint32[np + nextra][8]  the np points, then the extras, encoded
//   offsets   uint32[16][kRlcBuckets + 1]
//   idx       uint32[16][np + nextra]  (row w: its first offsets[w][kRlcBuckets] entries are read)
//   echunk    sorted entries per k_rlc_bucket thread: a power of two in [kRlcMinChunk, kRlcChunk]
//   use_sparse  1: k_rlc_window_sparse (np + nextra <= kRlcSparsePts), 0: k_rlc_segment + k_rlc_window
// Nothing is launched unless every offsets row starts at 0, is monotone and ends at most at
// np + nextra, and every id read (bit 31 masked) names one of the supplied points.
// Out: win_enc uint32[16][8] the window sums T_w; partial uint32[8] / identity int[1] of
// k_rlc_final; partial16 / identity16 of k_rlc_final16.
int msmprobe_reduce(long long np, long long nextra, long long p0, long long e0, const uint32_t* enc,
                    const uint32_t* offsets, const uint32_t* idx, int echunk, int use_sparse, uint32_t* win_enc,
                    uint32_t* partial, int* identity, uint32_t* partial16, int* identity16) {
  if (!ranges_ok(np, nextra, p0, e0) || !enc || !offsets || !idx || !win_enc || !partial || !identity ||
      !partial16 || !identity16)
    return (int)hipErrorInvalidValue;
  const int64_t npts = np + nextra;
  if (echunk < kRlcMinChunk || echunk > kRlcChunk || (echunk & (echunk - 1))) return (int)hipErrorInvalidValue;
  if (use_sparse != 0 && use_sparse != 1) return (int)hipErrorInvalidValue;
  if (use_sparse && npts > kRlcSparsePts) return (int)hipErrorInvalidValue;
  for (int w = 0; w < kRlcWindows; w++) {
    const uint32_t* o = offsets + (size_t)w * (kRlcBuckets + 1);
    if (o[0] != 0 || o[kRlcBuckets] > (uint32_t)npts) return (int)hipErrorInvalidValue;
    for (int b = 0; b < kRlcBuckets; b++)
      if (o[b] > o[b + 1]) return (int)hipErrorInvalidValue;
    const uint32_t* row = idx + (size_t)w * npts;
    for (uint32_t e = 0; e < o[kRlcBuckets]; e++) {
      const int64_t id = row[e] & 0x7fffffffu;
      const bool point = id >= p0 && id < p0 + np, extra = id >= e0 && id < e0 + nextra;
      if (!point && !extra) return (int)hipErrorInvalidValue;
    }
  }
  Pool p;
  RlcMsmArgs a{};
  a.p0 = p0;
  a.p1 = p0 + np;
  a.e0 = e0;
  a.nextra = (int)nextra;
  a.echunk = echunk;
  a.sparse = use_sparse;
  a.sgroups = (int)std::min<int64_t>(kRlcSparseMaxGroups, std::max<int64_t>(4, (npts + 127) / 128));  // launch_rlc_msm's
  a.istride = istride_of(npts);
  a.hstride = (npts + echunk - 1) / echunk;
  const uint32_t* d_enc = p.in(enc, (size_t)npts * 8);
  int* d_bad = p.out<int>(1);
  a.pts = p.out<ge_niels>((size_t)(e0 + nextra));
  a.offsets = const_cast<uint32_t*>(p.in(offsets, (size_t)kRlcWindows * (kRlcBuckets + 1)));
  a.idx = p.out<uint32_t>((size_t)kRlcWindows * a.istride);
  a.buckets = p.out<ge_p3>((size_t)kRlcWindows * kRlcBuckets);
  a.heads = p.out<ge_p3>((size_t)kRlcWindows * a.hstride);
  const size_t nseg = (size_t)kRlcWindows * (kRlcBuckets / kRlcSegLen);
  static_assert(kRlcBuckets / kRlcSegLen >= kRlcSparseMaxGroups, "the sparse partials live in seg_s");
  a.seg_s = p.out<ge_p3>(nseg);
  a.seg_w = p.out<ge_p3>(nseg);
  a.win = p.out<ge_p3>(kRlcWindows);
  ge_p3* d_win = use_sparse ? p.out<ge_p3>(kRlcWindows) : a.win;
  uint32_t* d_win_enc = p.out<uint32_t>(kRlcWindows * 8);
  uint32_t* d_partial = p.out<uint32_t>(16);
  int* d_identity = p.out<int>(2);
  if (p.err != hipSuccess) return (int)p.err;
  for (int w = 0; w < kRlcWindows && p.err == hipSuccess; w++) {
    const size_t cnt = offsets[(size_t)w * (kRlcBuckets + 1) + kRlcBuckets];
    if (cnt)
      p.step(hipMemcpy(a.idx + (size_t)w * a.istride, idx + (size_t)w * npts, cnt * sizeof(uint32_t),
                       hipMemcpyHostToDevice));
  }
  p.step(hipMemset(d_bad, 0, sizeof(int)));
  if (p.err == hipSuccess) {
    if (np) k_probe_decode_niels<<<grid64(np), 64>>>(np, d_enc, a.pts + p0, d_bad);
    if (nextra) k_probe_decode_niels<<<grid64(nextra), 64>>>(nextra, d_enc + 8 * np, a.pts + e0, d_bad);
  }
  p.sync();
  int bad = 0;
  p.back(&bad, d_bad, 1);
  if (p.err != hipSuccess) return (int)p.err;
  if (bad) return (int)hipErrorInvalidValue;
  const int64_t nb = (int64_t)kRlcWindows * kRlcBuckets;
  const int64_t chunks = (npts + echunk - 1) / echunk;
  hipLaunchKernelGGL(k_rlc_bucket, dim3((unsigned)((chunks + 255) / 256), kRlcWindows), dim3(256), 0, nullptr, a);
  hipLaunchKernelGGL(k_rlc_bucket_fix, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, nullptr, a);
  if (use_sparse) {
    hipLaunchKernelGGL(k_rlc_window_sparse, dim3((unsigned)a.sgroups, kRlcWindows), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_probe_sparse_windows, dim3(1), dim3(64), 0, nullptr, a.seg_s, a.sgroups, d_win);
  } else {
    hipLaunchKernelGGL(k_rlc_segment, dim3((unsigned)((4 * (int64_t)nseg + 255) / 256)), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_rlc_window, dim3(kRlcWindows), dim3(4 * kRlcWinQuads), 0, nullptr, a);
  }
  hipLaunchKernelGGL(k_probe_encode, dim3(1), dim3(64), 0, nullptr, (int64_t)kRlcWindows, d_win, d_win_enc);
  p.sync();
  if (p.err != hipSuccess) return (int)p.err;
  a.partial_out = d_partial;
  a.identity_out = d_identity;
  hipLaunchKernelGGL(k_rlc_final, dim3(1), dim3(64), 0, nullptr, a);
  a.partial_out = d_partial + 8;
  a.identity_out = d_identity + 1;
  hipLaunchKernelGGL(k_rlc_final16, dim3(1), dim3(64), 0, nullptr, a);
  p.sync();
  p.back(win_enc, d_win_enc, (size_t)kRlcWindows * 8);
  p.back(partial, d_partial, 8);
  p.back(partial16, d_partial + 8, 8);
  p.back(identity, d_identity, 1);
  p.back(identity16, d_identity + 1, 1);
  return (int)p.err;
}

}  // extern "C"
