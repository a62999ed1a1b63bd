// CPU build of csrc/pair_sum.h behind plain C entry points: the unit partition of the per-pair
// sums and the run cutter of cpz_verify_batch_pairs_many's per-proof leaves, for
// tests/test_pair_sum_model.py (checked against tests/pair_sum_model.py).
#include <chrono>
#include <cstdint>
#include <vector>

#include "pair_sum.h"
#include "verify.h"

extern "C" {

int pairsum_unit() { return cpz::kPairSumUnit; }

uint32_t pairsum_units(uint32_t count) { return cpz::pair_sum_units(count); }

long long pairsum_max_units(long long n, long long npairs) { return cpz::pair_sum_max_units(n, npairs); }

int pairsum_find(const uint32_t* ustart, int npairs, uint32_t u) { return cpz::pair_sum_find(ustart, npairs, u); }

// [lo, hi) cut into runs as pairs_many_leaf cuts it: ends[r] the end of run r, counts[r] its
// distinct pairs, firsts[r] the first pair it met (room for hi - lo runs each).  Returns the
// number of runs.
long long pairsum_runs(const uint32_t* pair_idx, long long lo, long long hi, int npairs, int max_pairs,
                       long long* ends, int* counts, uint32_t* firsts) {
  std::vector<uint32_t> stamp((size_t)npairs, 0), run((size_t)max_pairs);
  uint32_t tag = 0;
  long long r = 0;
  for (int64_t a = lo; a < hi; r++) {
    int k = 0;
    a = cpz::pair_run_end(pair_idx, a, hi, stamp.data(), ++tag, max_pairs, run.data(), &k);
    ends[r] = a;
    counts[r] = k;
    firsts[r] = run[0];
  }
  return r;
}

// The per-pair work of cpz_verify_batch_pairs_ex's host descriptor loop -- the recording sponge
// of challenge_masks_ctx32 -- over npairs pairs (gh: 16 words each), in milliseconds of this CPU
// build: what tools/batch_pairs_many_ab.py extrapolates to 4096 pairs.  *acc receives a word of
// the masks so that the loop is not optimised away.
double pairsum_host_masks_ms(int npairs, const uint32_t* gh, uint32_t* acc) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t x = 0;
  for (int p = 0; p < npairs; p++) {
    uint32_t m[3][50];
    if (cpz::challenge_masks_ctx32(m, gh + 16 * p, gh + 16 * p + 8)) x ^= m[2][7] ^ m[0][3];
  }
  *acc = x;
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // extern "C"
