// Test-only probes of the small per-pair generator tables of cpz_verify_each_pairs_many
// (csrc/kernels.hip: k_pair_micro, pair_micro_window) on hand-made inputs.
//
// The public ABI reaches these tables only inside whole verifications, where the digits of
// s' = +-v s mod l are fixed by the transcript and the one observable is a status.  This unit
// includes kernels.hip textually and unchanged, so that its kernels are visible, and exports plain
// C entry points over host pointers: the product's own table build (launch_pair_micro) on a
// caller's pairs, returning the tables, and [k] g, [k] h for a caller's 256-bit k by the
// 32-window loop of k_verify_quad with the generator additions alone (pair_micro_window, the
// function the kernel calls).  tests/test_gpu_pair_micro_probe.py compares both with the Python
// oracle.  Every entry point allocates, copies in, launches, synchronises, copies back, frees, and
// returns the hipError_t; the table buffer is filled with 0xff first, so an unwritten slot shows.
// Never linked into the product library.
#include <cstring>
#include <vector>

#include "kernels.hip"

using namespace cpz;

namespace {

// quad (v, e): [k_v] B for B = generator e of pair pair_of[v], as k_verify_quad's kMicro arm walks
// the digits of s' (window w: digit w on B, digit 32 + w on 2^128 B); lane 0 encodes the result
__global__ void __launch_bounds__(64) k_probe_micro_mul(int m, const int32_t* __restrict__ micro,
                                                        const uint32_t* __restrict__ pair_of,
                                                        const uint32_t* __restrict__ k, uint32_t* __restrict__ out) {
  const int quad = blockIdx.x * 16 + (threadIdx.x >> 2), q = threadIdx.x & 3;
  const int v = quad >> 1, e = quad & 1;
  if (v >= m) return;  // whole quads
  uint32_t kw[8], sd[8];
  for (int j = 0; j < 8; j++) kw[j] = k[8 * v + j];
  sc_recode_radix16(sd, kw);
  const int32_t* tb = micro + (int64_t)pair_of[v] * kPairMicroInts + 2 * e * kPairMicroTableInts;
  ge_p3 acc = ge_identity();
#pragma unroll 1
  for (int w = 31; w >= 0; w--) {
    const int dg = ((int32_t)(sd[w >> 3] << (28 - 4 * (w & 7)))) >> 28;
    const int dg2 = ((int32_t)(sd[4 + (w >> 3)] << (28 - 4 * (w & 7)))) >> 28;
    if (w != 31) acc = p3_dbl_n_quad(acc, 4, q);
    acc = pair_micro_window(acc, tb, dg, dg2, q);
  }
  if (q != 0) return;
  uint32_t enc[8];
  ristretto_encode(enc, acc);
  for (int j = 0; j < 8; j++) out[16 * v + 8 * e + j] = enc[j];
}

struct Bufs {
  PairDesc* desc = nullptr;
  int32_t* micro = nullptr;
  uint32_t *pair_of = nullptr, *k = nullptr, *out = nullptr;
  ~Bufs() {
    (void)hipFree(desc);
    (void)hipFree(micro);
    (void)hipFree(pair_of);
    (void)hipFree(k);
    (void)hipFree(out);
  }
};

#define PROBE_HIP(x)                    \
  do {                                  \
    const hipError_t e_ = (x);          \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// descriptor rows with the generator words alone (all k_pair_micro reads), then the product's build
int build_tables(Bufs& b, int npairs, const uint8_t* pairs) {
  std::vector<PairDesc> desc((size_t)npairs);
  std::memset(desc.data(), 0, desc.size() * sizeof(PairDesc));
  for (int p = 0; p < npairs; p++) std::memcpy(desc[(size_t)p].gh_words, pairs + 64 * p, 64);
  const size_t bytes = (size_t)npairs * kPairMicroBytes;
  PROBE_HIP(hipMalloc(&b.desc, desc.size() * sizeof(PairDesc)));
  PROBE_HIP(hipMalloc(&b.micro, bytes));
  PROBE_HIP(hipMemset(b.micro, 0xff, bytes));
  PROBE_HIP(hipMemcpy(b.desc, desc.data(), desc.size() * sizeof(PairDesc), hipMemcpyHostToDevice));
  PROBE_HIP(launch_pair_micro(b.desc, npairs, b.micro, nullptr));
  PROBE_HIP(hipDeviceSynchronize());
  return 0;
}

}  // namespace

extern "C" {

// out[0..4): kPairMicroInts, kPairMicroTableInts, kPairMicroTables, sizeof(PairDesc)
void microprobe_consts(int* out) {
  out[0] = kPairMicroInts;
  out[1] = kPairMicroTableInts;
  out[2] = kPairMicroTables;
  out[3] = (int)sizeof(PairDesc);
}

// The small tables of npairs pairs (64-byte rows, g then h): npairs * kPairMicroInts ints out.
int microprobe_tables(int npairs, const uint8_t* pairs, int32_t* out) {
  if (npairs < 1 || npairs > 4096 || !pairs || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  if (int rc = build_tables(b, npairs, pairs)) return rc;
  PROBE_HIP(hipMemcpy(out, b.micro, (size_t)npairs * kPairMicroBytes, hipMemcpyDeviceToHost));
  return 0;
}

// out[64 v ..): the encodings of [k_v] g and [k_v] h under pairs[pair_of[v]]; k: m x 8 words, each
// below 2^255 (sc_recode_radix16's range).  Every pair_of[v] must be below npairs (checked here).
int microprobe_mul(int npairs, const uint8_t* pairs, int m, const uint32_t* pair_of, const uint32_t* k, uint8_t* out) {
  if (npairs < 1 || npairs > 4096 || m < 1 || m > 65536 || !pairs || !pair_of || !k || !out)
    return (int)hipErrorInvalidValue;
  for (int v = 0; v < m; v++)
    if (pair_of[v] >= (uint32_t)npairs || (k[8 * v + 7] >> 31)) return (int)hipErrorInvalidValue;
  Bufs b;
  if (int rc = build_tables(b, npairs, pairs)) return rc;
  PROBE_HIP(hipMalloc(&b.pair_of, (size_t)m * 4));
  PROBE_HIP(hipMalloc(&b.k, (size_t)m * 32));
  PROBE_HIP(hipMalloc(&b.out, (size_t)m * 64));
  PROBE_HIP(hipMemset(b.out, 0xff, (size_t)m * 64));
  PROBE_HIP(hipMemcpy(b.pair_of, pair_of, (size_t)m * 4, hipMemcpyHostToDevice));
  PROBE_HIP(hipMemcpy(b.k, k, (size_t)m * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe_micro_mul, dim3((unsigned)((2 * m + 15) / 16)), dim3(64), 0, nullptr, m, b.micro, b.pair_of,
                     b.k, b.out);
  PROBE_HIP(hipGetLastError());
  PROBE_HIP(hipDeviceSynchronize());
  PROBE_HIP(hipMemcpy(out, b.out, (size_t)m * 64, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
