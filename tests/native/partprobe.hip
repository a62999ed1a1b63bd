// Test-only probes of the partitioned batch check (csrc/part.hip) on hand-made inputs.
//
// The public ABI reaches part.hip only from batches of 2^19 proofs or more, with every MSM
// scalar derived from the seed.  This unit includes part.hip textually and unchanged, so that
// its kernels are visible and each combine variant can be launched by name, and exports plain C
// entry points over host pointers; tests/test_gpu_part_probe.py compares what they return with
// Python integers (tests/part_model.py) and the Python oracle.  Every entry point allocates,
// copies in, launches, synchronises, copies back, frees, and returns the hipError_t; every
// output buffer is filled with 0xff first, so an unwritten byte shows.  Never linked into the
// product library.
#include "part.hip"

using namespace cpz;

namespace {

// enc[i] -> ge_p3 (Z = 1); *bad is set if an encoding does not decode
__global__ void __launch_bounds__(64) k_probe_decode_p3(int64_t n, const uint32_t* enc, ge_p3* out, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = enc[8 * i + k];
  ge_p3 P;
  if (!ristretto_decode(P, w)) *bad = 1;
  store_p3(out + i, P);
}

// enc[i] -> affine Niels, not negated, at out[i * stride]
__global__ void __launch_bounds__(64) k_probe_decode_niels(int64_t n, const uint32_t* enc, ge_niels* out,
                                                           int64_t stride, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = enc[8 * i + k];
  ge_p3 P;
  if (!ristretto_decode(P, w)) *bad = 1;
  store_niels(out + i * stride, niels_from_p3_affine(P, false));
}

__global__ void __launch_bounds__(64) k_probe_encode(int64_t n, const ge_p3* in, uint32_t* enc) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ristretto_encode(w, load_p3(in + i));
  for (int k = 0; k < 8; k++) enc[8 * i + k] = w[k];
}

// one wave; lane l takes cases l, l + 64, ...
__global__ void __launch_bounds__(64) k_probe_weight_digits(int n, const uint32_t* u, const int64_t* j, int16_t* out) {
  for (int i = (int)threadIdx.x; i < n; i += 64) {
    uint32_t uw[4];
    for (int k = 0; k < 4; k++) uw[k] = u[4 * i + k];
    int16_t d[kRlcWindows];
    index_weight_digits(d, uw, j[i]);
    for (int w = 0; w < kRlcWindows; w++) out[kRlcWindows * i + w] = d[w];
  }
}

// Device buffers of one entry point; everything is freed by the destructor.
struct Pool {
  static constexpr int kMax = 24;
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
    if (err == hipSuccess) err = hipMemset(dev[used], 0xff, count * sizeof(T));
    return err == hipSuccess ? static_cast<T*>(dev[used++]) : nullptr;
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

}  // namespace

extern "C" {

// The constants the tests need, by index (tests/part_model.py names them).
long long partprobe_const(int which) {
  switch (which) {
    case 0: return kPartProofs;
    case 1: return kPartTopBuckets;
    case 2: return kPartLocJ0;
    case 3: return kPartLocLanes;
    case 4: return kPartListCap;
    case 5: return kPartOffs;
    case 6: return kPartUnits;
    case 7: return kPartNoLoc;
    case 8: return kPartTreeMaxBlocks;
    case 9: return kPartLaneMinBlocks;
    case 10: return kRlcSumBlock;
    case 11: return kPartWindows;
    case 12: return kPartBuckets;
    case 13: return kRlcWindows;
    case 14: return kPartSumRun;
    default: return -1;
  }
}

// The block partials of nblk blocks over n proofs (the last block may be partial).
//   pts_enc   uint32[nprep * 4 kPartProofs][8]  encoded points of the nprep prepared blocks
//             (nprep = nblk without a pmap)
//   digits    int16[16][dstride], dstride >= 4 kPartProofs nblk and a multiple of 4
//   sums      uint32[nblk * kPartProofs / kRlcSumBlock][2][8]
//   gh_enc    uint32[2][8]
//   pmap      uint32[nblk] or null
//   per_launch  blocks per sort / walk launch (blk0 = 0, per_launch, ...)
//   combine   0: launch_part_combine's choice, 1: k_part_combine, 2: k_part_combine_lane,
//             3: k_part_combine_tree, each over all nblk blocks in one launch
// Out: part_enc uint32[nblk][8], fail uint8[nblk], lists uint16[nblk][kPartListCap],
// offs uint16[nblk][kPartOffs], assign uint16[nblk][kPartUnits], partial uint32[8], identity int[1].
int partprobe_blocks(long long nblk, long long n, long long nprep, const uint32_t* pts_enc, const int16_t* digits,
                     long long dstride, const uint32_t* sums, const uint32_t* gh_enc, const uint32_t* pmap,
                     long long per_launch, int combine, uint32_t* part_enc, uint8_t* fail, uint16_t* lists,
                     uint16_t* offs, uint16_t* assign, uint32_t* partial, int* identity) {
  constexpr int R = kPartProofs / kRlcSumBlock;
  if (nblk <= 0 || n <= (nblk - 1) * kPartProofs || n > nblk * kPartProofs || per_launch <= 0 || combine < 0 ||
      combine > 3 || dstride < 4 * kPartProofs * nblk || (dstride & 3) || nprep < (pmap ? 1 : nblk))
    return (int)hipErrorInvalidValue;
  if (pmap)
    for (long long b = 0; b < nblk; b++)
      if ((long long)pmap[b] >= nprep) return (int)hipErrorInvalidValue;
  Pool p;
  const int64_t npts = (int64_t)nprep * 4 * kPartProofs;
  const int64_t chunk = nblk < per_launch ? nblk : per_launch;
  const uint32_t* d_enc = p.in(pts_enc, (size_t)npts * 8);
  const uint32_t* d_gh = p.in(gh_enc, 16);
  int* d_bad = p.out<int>(1);
  ge_niels* d_pts = p.out<ge_niels>((size_t)npts);
  ge_niels* d_tab = p.out<ge_niels>(kNielsEntriesRlc + 1);
  PartArgs a;
  a.n = n;
  a.pts = d_pts;
  a.digits = p.in(digits, (size_t)kRlcWindows * dstride);
  a.dstride = dstride;
  a.block_sums = reinterpret_cast<const sc*>(p.in(sums, (size_t)nblk * R * 16));
  a.tab = d_tab;
  a.lists = p.out<uint16_t>((size_t)chunk * kPartListCap);
  a.assign = p.out<uint16_t>((size_t)chunk * kPartUnits);
  a.offs = p.out<uint16_t>((size_t)chunk * kPartOffs);
  a.wsum = p.out<ge_p3>((size_t)nblk * kPartWsum);
  a.part = p.out<ge_p3>((size_t)nblk);
  a.fail = p.out<uint8_t>((size_t)nblk);
  a.pmap = pmap ? p.in(pmap, (size_t)nblk) : nullptr;
  ge_p3* d_tmp = p.out<ge_p3>((size_t)((nblk + 63) / 64 + 16));
  uint32_t* d_part_enc = p.out<uint32_t>((size_t)nblk * 8);
  uint32_t* d_partial = p.out<uint32_t>(8);
  int* d_identity = p.out<int>(1);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(hipMemset(d_bad, 0, sizeof(int)));
  if (p.err == hipSuccess) {
    k_probe_decode_niels<<<grid64(npts), 64>>>(npts, d_enc, d_pts, 1, d_bad);
    k_probe_decode_niels<<<1, 64>>>(2, d_gh, d_tab, kNielsEntriesRlc, d_bad);
  }
  p.sync();
  int bad = 0;
  p.back(&bad, d_bad, 1);
  if (p.err == hipSuccess && bad) return (int)hipErrorInvalidValue;
  for (int64_t b0 = 0; b0 < nblk && p.err == hipSuccess; b0 += chunk) {
    a.blk0 = b0;
    a.nblk = chunk < nblk - b0 ? chunk : nblk - b0;
    if (b0 > 0) {  // the launch's own buffers are reused: nothing of the previous launch may show
      p.step(hipMemset(a.lists, 0xff, (size_t)chunk * kPartListCap * sizeof(uint16_t)));
      p.step(hipMemset(a.offs, 0xff, (size_t)chunk * kPartOffs * sizeof(uint16_t)));
      p.step(hipMemset(a.assign, 0xff, (size_t)chunk * kPartUnits * sizeof(uint16_t)));
    }
    if (p.err == hipSuccess) p.step(launch_part_sort(a, nullptr));
    if (p.err == hipSuccess) p.step(launch_part_acc(a, nullptr));
    p.sync();
    p.back(lists + b0 * kPartListCap, a.lists, (size_t)a.nblk * kPartListCap);
    p.back(offs + b0 * kPartOffs, a.offs, (size_t)a.nblk * kPartOffs);
    p.back(assign + b0 * kPartUnits, a.assign, (size_t)a.nblk * kPartUnits);
  }
  if (p.err != hipSuccess) return (int)p.err;
  a.blk0 = 0;
  a.nblk = nblk;
  if (combine == 0) {
    p.step(launch_part_combine(a, nullptr));
  } else if (combine == 1) {
    k_part_combine<<<(unsigned)((nblk + 15) / 16), 64>>>(a);
  } else if (combine == 2) {
    k_part_combine_lane<<<(unsigned)((nblk + 255) / 256), 256>>>(a);
  } else {
    k_part_combine_tree<<<(unsigned)nblk, 4 * kPartWindows>>>(a);
  }
  p.sync();
  if (p.err == hipSuccess) p.step(launch_part_sum(a.part, nblk, d_tmp, d_partial, d_identity, nullptr));
  if (p.err == hipSuccess) k_probe_encode<<<grid64(nblk), 64>>>(nblk, a.part, d_part_enc);
  p.sync();
  p.back(part_enc, d_part_enc, (size_t)nblk * 8);
  p.back(fail, a.fail, (size_t)nblk);
  p.back(partial, d_partial, 8);
  p.back(identity, d_identity, 1);
  return (int)p.err;
}

// launch_part_sum over nblk encoded points.  Out: partial uint32[8], identity int[1].
int partprobe_sum(long long nblk, const uint32_t* enc, uint32_t* partial, int* identity) {
  if (nblk <= 0) return (int)hipErrorInvalidValue;
  Pool p;
  const uint32_t* d_enc = p.in(enc, (size_t)nblk * 8);
  int* d_bad = p.out<int>(1);
  ge_p3* d_part = p.out<ge_p3>((size_t)nblk);
  ge_p3* d_tmp = p.out<ge_p3>((size_t)((nblk + 63) / 64 + 16));
  uint32_t* d_partial = p.out<uint32_t>(8);
  int* d_identity = p.out<int>(1);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(hipMemset(d_bad, 0, sizeof(int)));
  if (p.err == hipSuccess) k_probe_decode_p3<<<grid64(nblk), 64>>>(nblk, d_enc, d_part, d_bad);
  p.sync();
  int bad = 0;
  p.back(&bad, d_bad, 1);
  if (p.err == hipSuccess && bad) return (int)hipErrorInvalidValue;
  if (p.err == hipSuccess) p.step(launch_part_sum(d_part, nblk, d_tmp, d_partial, d_identity, nullptr));
  p.sync();
  p.back(partial, d_partial, 8);
  p.back(identity, d_identity, 1);
  return (int)p.err;
}

// launch_part_index_digits over nblk listed blocks of a prepared batch of n proofs.
//   blocks uint32[nblk], seed uint32[8], s / c uint32[n][8], status uint8[n]
// Out: digits int16[16][dstride] (dstride >= 4 kPartProofs nblk),
// sums uint32[nblk * kPartProofs / kRlcSumBlock][2][8].
int partprobe_index_digits(long long nblk, long long n, const uint32_t* blocks, unsigned long long first_index,
                           const uint32_t* seed, const uint32_t* s, const uint32_t* c, const uint8_t* status,
                           long long dstride, int16_t* digits, uint32_t* sums) {
  constexpr int R = kPartProofs / kRlcSumBlock;
  if (nblk <= 0 || n <= 0 || dstride < 4 * kPartProofs * nblk) return (int)hipErrorInvalidValue;
  Pool p;
  PartIdxArgs a;
  a.nblk = nblk;
  a.n = n;
  a.blocks = p.in(blocks, (size_t)nblk);
  a.first_index = first_index;
  for (int k = 0; k < 8; k++) a.seed[k] = seed[k];
  a.s = p.in(s, (size_t)n * 8);
  a.c = p.in(c, (size_t)n * 8);
  a.status = p.in(status, (size_t)n);
  a.digits = p.out<int16_t>((size_t)kRlcWindows * dstride);
  a.dstride = dstride;
  uint32_t* d_sums = p.out<uint32_t>((size_t)nblk * R * 16);
  a.block_sums = reinterpret_cast<sc*>(d_sums);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(launch_part_index_digits(a, nullptr));
  p.sync();
  p.back(digits, a.digits, (size_t)kRlcWindows * dstride);
  p.back(sums, d_sums, (size_t)nblk * R * 16);
  return (int)p.err;
}

// index_weight_digits(u[i], j[i]) for i < n.  u uint32[n][4], j int64[n]; out int16[n][16].
int partprobe_weight_digits(int n, const uint32_t* u, const long long* j, int16_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  Pool p;
  const uint32_t* du = p.in(u, (size_t)n * 4);
  const int64_t* dj = reinterpret_cast<const int64_t*>(p.in(j, (size_t)n));
  int16_t* dout = p.out<int16_t>((size_t)n * kRlcWindows);
  if (p.err != hipSuccess) return (int)p.err;
  k_probe_weight_digits<<<1, 64>>>(n, du, dj, dout);
  p.sync();
  p.back(out, dout, (size_t)n * kRlcWindows);
  return (int)p.err;
}

// launch_part_locate over nblk listed blocks.  part_enc uint32[npart][8], lpart_enc
// uint32[nblk][8], lfail uint8[nblk], blocks uint32[nblk] (< npart).  Out: loc uint16[nblk].
int partprobe_locate(long long nblk, long long npart, const uint32_t* part_enc, const uint32_t* lpart_enc,
                     const uint8_t* lfail, const uint32_t* blocks, uint16_t* loc) {
  if (nblk <= 0 || npart <= 0) return (int)hipErrorInvalidValue;
  for (long long b = 0; b < nblk; b++)
    if ((long long)blocks[b] >= npart) return (int)hipErrorInvalidValue;
  Pool p;
  const uint32_t* d_pe = p.in(part_enc, (size_t)npart * 8);
  const uint32_t* d_le = p.in(lpart_enc, (size_t)nblk * 8);
  int* d_bad = p.out<int>(1);
  ge_p3* d_part = p.out<ge_p3>((size_t)npart);
  ge_p3* d_lpart = p.out<ge_p3>((size_t)nblk);
  PartLocArgs a;
  a.nblk = nblk;
  a.blocks = p.in(blocks, (size_t)nblk);
  a.part = d_part;
  a.lpart = d_lpart;
  a.lfail = p.in(lfail, (size_t)nblk);
  a.loc = p.out<uint16_t>((size_t)nblk);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(hipMemset(d_bad, 0, sizeof(int)));
  if (p.err == hipSuccess) {
    k_probe_decode_p3<<<grid64(npart), 64>>>(npart, d_pe, d_part, d_bad);
    k_probe_decode_p3<<<grid64(nblk), 64>>>(nblk, d_le, d_lpart, d_bad);
  }
  p.sync();
  int bad = 0;
  p.back(&bad, d_bad, 1);
  if (p.err == hipSuccess && bad) return (int)hipErrorInvalidValue;
  if (p.err == hipSuccess) p.step(launch_part_locate(a, nullptr));
  p.sync();
  p.back(loc, a.loc, (size_t)nblk);
  return (int)p.err;
}

}  // extern "C"
