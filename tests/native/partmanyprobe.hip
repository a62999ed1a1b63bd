// Test-only probes of the partitioned check's many mode (csrc/part.hip) on hand-made inputs.
//
// The public ABI reaches the many-mode kernels only with seed-derived scalars.  This unit includes
// part.hip textually and unchanged and exports plain C entry points over host pointers that run
// k_part_sort_many, k_part_acc_many, the combine, k_part_index_digits_many and k_part_locate on
// caller-made digit rows, product rows, pair indices, slot tables and points;
// tests/test_gpu_part_many_probe.py compares what they return with Python integers
// (tests/part_many_model.py) and the Python oracle.  Every entry point allocates, copies in,
// launches, synchronises, copies back, frees, and returns the hipError_t; every output buffer is
// filled with 0xff first, so an unwritten byte shows.  Never linked into the product library.
#include "part.hip"

using namespace cpz;

namespace {

// enc[i] -> ge_p3 (Z = 1); *bad is set if an encoding does not decode
__global__ void __launch_bounds__(64) k_mprobe_decode_p3(int64_t n, const uint32_t* enc, ge_p3* out, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = enc[8 * i + k];
  ge_p3 P;
  if (!ristretto_decode(P, w)) *bad = 1;
  store_p3(out + i, P);
}

// enc[i] -> affine Niels, not negated, at out[i]
__global__ void __launch_bounds__(64) k_mprobe_decode_niels(int64_t n, const uint32_t* enc, ge_niels* out, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = enc[8 * i + k];
  ge_p3 P;
  if (!ristretto_decode(P, w)) *bad = 1;
  store_niels(out + i, niels_from_p3_affine(P, false));
}

__global__ void __launch_bounds__(64) k_mprobe_encode(int64_t n, const ge_p3* in, uint32_t* enc) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ristretto_encode(w, load_p3(in + i));
  for (int k = 0; k < 8; k++) enc[8 * i + k] = w[k];
}

// Device buffers of one entry point; everything is freed by the destructor.
struct Pool {
  static constexpr int kMax = 28;
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

// A slot table names pairs below npairs, or kPartNoPair.
bool slots_ok(const uint16_t* slots, long long rows, int npairs) {
  for (long long i = 0; i < rows * kPartProofs; i++)
    if (slots[i] != kPartNoPair && slots[i] >= npairs) return false;
  return true;
}

}  // namespace

extern "C" {

// The many-mode constants, by index (tests/part_many_model.py names them).
long long partmanyprobe_const(int which) {
  switch (which) {
    case 0: return kPartListCapMany;
    case 1: return kPairBucketMaxPairs;
    case 2: return kPartProofs;
    case 3: return kPartWindows;
    case 4: return kPartNoPair;
    default: return -1;
  }
}

// The many-mode block partials of nblk blocks over n proofs (the last block may be partial).
//   pts_enc   uint32[nprep * 4 kPartProofs][8]  encoded points of the nprep prepared blocks
//   digits    int16[16][dstride], dstride >= 4 kPartProofs nblk and a multiple of 4
//   prod      uint32[prod_rows][2][8] with pair_idx uint32[prod_rows], prod_rows >= n (the rows
//             past n are there to show that they are not read): the first pass, which assigns the
//             slots and writes slots_out uint16[nblk][kPartProofs]; or, with pair_idx null, the
//             locate pass: prod holds the sums by slot, uint32[nblk][kPartProofs][2][8] (prod_rows =
//             nblk * kPartProofs), pmap is required and slots_in uint16[nprep][kPartProofs] are the
//             prepared blocks' tables
//   gh_enc    uint32[2 npairs][8]
//   pmap      uint32[nblk] or null
//   per_launch  blocks per sort / walk launch (blk0 = 0, per_launch, ...)
// Out: part_enc uint32[nblk][8], fail uint8[nblk], lists uint16[nblk][kPartListCapMany],
// offs uint16[nblk][kPartOffs], assign uint16[nblk][kPartUnits], partial uint32[8], identity int[1].
int partmanyprobe_blocks(long long nblk, long long n, long long nprep, const uint32_t* pts_enc, const int16_t* digits,
                         long long dstride, const uint32_t* prod, const uint32_t* pair_idx, long long prod_rows,
                         const uint32_t* gh_enc, int npairs, const uint32_t* pmap, const uint16_t* slots_in,
                         long long per_launch, uint32_t* part_enc, uint8_t* fail, uint16_t* lists, uint16_t* offs,
                         uint16_t* assign, uint32_t* partial, int* identity, uint16_t* slots_out) {
  if (nblk <= 0 || n <= (nblk - 1) * kPartProofs || n > nblk * kPartProofs || per_launch <= 0 ||
      dstride < 4 * kPartProofs * nblk || (dstride & 3) || nprep < (pmap ? 1 : nblk) || npairs < 1 ||
      npairs > kPairBucketMaxPairs || !prod || prod_rows < (pair_idx ? n : nblk * kPartProofs))
    return (int)hipErrorInvalidValue;
  if (pair_idx ? (pmap || !slots_out) : (!pmap || !slots_in || !slots_ok(slots_in, nprep, npairs)))
    return (int)hipErrorInvalidValue;
  if (pmap)
    for (long long b = 0; b < nblk; b++)
      if ((long long)pmap[b] >= nprep) return (int)hipErrorInvalidValue;
  if (pair_idx)
    for (long long i = 0; i < prod_rows; i++)
      if (pair_idx[i] >= (uint32_t)npairs) return (int)hipErrorInvalidValue;
  Pool p;
  const int64_t npts = (int64_t)nprep * 4 * kPartProofs;
  const int64_t chunk = nblk < per_launch ? nblk : per_launch;
  const uint32_t* d_enc = p.in(pts_enc, (size_t)npts * 8);
  const uint32_t* d_gh = p.in(gh_enc, (size_t)16 * npairs);
  int* d_bad = p.out<int>(1);
  ge_niels* d_pts = p.out<ge_niels>((size_t)npts);
  ge_niels* d_ghn = p.out<ge_niels>((size_t)2 * npairs);
  PartArgs a;
  a.n = n;
  a.pts = d_pts;
  a.digits = p.in(digits, (size_t)kRlcWindows * dstride);
  a.dstride = dstride;
  a.block_sums = nullptr;
  a.tab = nullptr;
  a.prod = reinterpret_cast<const sc*>(p.in(prod, (size_t)prod_rows * 16));
  a.pair_idx = pair_idx ? p.in(pair_idx, (size_t)prod_rows) : nullptr;
  a.gh = d_ghn;
  a.npairs = npairs;
  a.slots = pair_idx ? p.out<uint16_t>((size_t)nblk * kPartProofs)
                     : const_cast<uint16_t*>(p.in(slots_in, (size_t)nprep * kPartProofs));
  a.lists = p.out<uint16_t>((size_t)chunk * kPartListCapMany);
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
    k_mprobe_decode_niels<<<grid64(npts), 64>>>(npts, d_enc, d_pts, d_bad);
    k_mprobe_decode_niels<<<grid64(2 * npairs), 64>>>(2 * npairs, d_gh, d_ghn, d_bad);
  }
  p.sync();
  int bad = 0;
  p.back(&bad, d_bad, 1);
  if (p.err == hipSuccess && bad) return (int)hipErrorInvalidValue;
  for (int64_t b0 = 0; b0 < nblk && p.err == hipSuccess; b0 += chunk) {
    a.blk0 = b0;
    a.nblk = chunk < nblk - b0 ? chunk : nblk - b0;
    if (b0 > 0) {  // the launch's own buffers are reused: nothing of the previous launch may show
      p.step(hipMemset(a.lists, 0xff, (size_t)chunk * kPartListCapMany * sizeof(uint16_t)));
      p.step(hipMemset(a.offs, 0xff, (size_t)chunk * kPartOffs * sizeof(uint16_t)));
      p.step(hipMemset(a.assign, 0xff, (size_t)chunk * kPartUnits * sizeof(uint16_t)));
    }
    if (p.err == hipSuccess) p.step(launch_part_sort(a, nullptr));
    if (p.err == hipSuccess) p.step(launch_part_acc(a, nullptr));
    p.sync();
    p.back(lists + b0 * kPartListCapMany, a.lists, (size_t)a.nblk * kPartListCapMany);
    p.back(offs + b0 * kPartOffs, a.offs, (size_t)a.nblk * kPartOffs);
    p.back(assign + b0 * kPartUnits, a.assign, (size_t)a.nblk * kPartUnits);
  }
  if (p.err != hipSuccess) return (int)p.err;
  a.blk0 = 0;
  a.nblk = nblk;
  p.step(launch_part_combine(a, nullptr));
  p.sync();
  if (p.err == hipSuccess) p.step(launch_part_sum(a.part, nblk, d_tmp, d_partial, d_identity, nullptr));
  if (p.err == hipSuccess) k_mprobe_encode<<<grid64(nblk), 64>>>(nblk, a.part, d_part_enc);
  p.sync();
  p.back(part_enc, d_part_enc, (size_t)nblk * 8);
  p.back(fail, a.fail, (size_t)nblk);
  p.back(partial, d_partial, 8);
  p.back(identity, d_identity, 1);
  if (pair_idx) p.back(slots_out, a.slots, (size_t)nblk * kPartProofs);
  return (int)p.err;
}

// launch_part_index_digits in many mode over nblk listed blocks of a prepared batch of n proofs.
//   blocks uint32[nblk] (< nprep), seed uint32[8], c uint32[n][8], status uint8[n],
//   prod uint32[n][2][8], pair_idx uint32[n], slots uint16[nprep][kPartProofs]
// Out: digits int16[16][dstride] (dstride >= 4 kPartProofs nblk), pair_sums
// uint32[nblk][kPartProofs][2][8].
int partmanyprobe_index_digits(long long nblk, long long n, long long nprep, const uint32_t* blocks,
                               unsigned long long first_index, const uint32_t* seed, const uint32_t* c,
                               const uint8_t* status, const uint32_t* prod, const uint32_t* pair_idx, int npairs,
                               const uint16_t* slots, long long dstride, int16_t* digits, uint32_t* pair_sums) {
  if (nblk <= 0 || n <= 0 || nprep <= 0 || n > nprep * kPartProofs || dstride < 4 * kPartProofs * nblk || npairs < 1 ||
      npairs > kPairBucketMaxPairs || !slots || !slots_ok(slots, nprep, npairs))
    return (int)hipErrorInvalidValue;
  for (long long b = 0; b < nblk; b++)
    if ((long long)blocks[b] >= nprep) return (int)hipErrorInvalidValue;
  for (long long i = 0; i < n; i++)
    if (pair_idx[i] >= (uint32_t)npairs) return (int)hipErrorInvalidValue;
  Pool p;
  PartIdxArgs a;
  a.nblk = nblk;
  a.n = n;
  a.blocks = p.in(blocks, (size_t)nblk);
  a.first_index = first_index;
  for (int k = 0; k < 8; k++) a.seed[k] = seed[k];
  a.s = nullptr;  // the pair modes read the products instead
  a.c = p.in(c, (size_t)n * 8);
  a.status = p.in(status, (size_t)n);
  a.digits = p.out<int16_t>((size_t)kRlcWindows * dstride);
  a.dstride = dstride;
  a.block_sums = nullptr;
  a.prod = reinterpret_cast<const sc*>(p.in(prod, (size_t)n * 16));
  a.pair_idx = p.in(pair_idx, (size_t)n);
  a.npairs = npairs;
  a.slots = p.in(slots, (size_t)nprep * kPartProofs);
  uint32_t* d_sums = p.out<uint32_t>((size_t)nblk * kPartProofs * 16);
  a.pair_sums = reinterpret_cast<sc*>(d_sums);
  if (p.err != hipSuccess) return (int)p.err;
  p.step(launch_part_index_digits(a, nullptr));
  p.sync();
  p.back(digits, a.digits, (size_t)kRlcWindows * dstride);
  p.back(pair_sums, d_sums, (size_t)nblk * kPartProofs * 16);
  return (int)p.err;
}

// launch_part_locate over nblk listed blocks.  part_enc uint32[npart][8], lpart_enc
// uint32[nblk][8], lfail uint8[nblk], blocks uint32[nblk] (< npart).  Out: loc uint16[nblk].
int partmanyprobe_locate(long long nblk, long long npart, const uint32_t* part_enc, const uint32_t* lpart_enc,
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
    k_mprobe_decode_p3<<<grid64(npart), 64>>>(npart, d_pe, d_part, d_bad);
    k_mprobe_decode_p3<<<grid64(nblk), 64>>>(nblk, d_le, d_lpart, d_bad);
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

// The launchers refuse what they cannot serve: more pairs than the slot tables can name, and a
// locate-pass sort without pmap.  Returns the two hipError_t values, nothing is launched.
int partmanyprobe_refusals(int* too_many_pairs, int* presummed_without_pmap) {
  PartArgs a{};
  a.nblk = 1;
  a.n = 1;
  a.prod = reinterpret_cast<const sc*>(&a);   // never read: the launcher returns first
  a.gh = reinterpret_cast<const ge_niels*>(&a);
  a.slots = reinterpret_cast<uint16_t*>(&a);
  a.pair_idx = reinterpret_cast<const uint32_t*>(&a);
  a.npairs = kPairBucketMaxPairs + 1;
  *too_many_pairs = (int)launch_part_sort(a, nullptr);
  a.npairs = 2;
  a.pair_idx = nullptr;
  a.pmap = nullptr;
  *presummed_without_pmap = (int)launch_part_sort(a, nullptr);
  return 0;
}

}  // extern "C"
