// Per-pair sums of a mixed-pair batch with more than CPZ_PAIRS_MAX pairs (rlc.hip's k_pair_*
// kernels, cpz_verify_batch_pairs_many): the partition of the pairs' entry lists into work units
// of bounded length, and the host's cutting of a range into runs of at most CPZ_PAIRS_MAX
// distinct pairs.  Host and device share these functions; tests/pair_sum_model.py models them.
#pragma once

#include <cstdint>

#include "fe25519.h"  // CPZ_HD

namespace cpz {

// Entries per work unit of k_pair_unit_sums: one wave adds a unit's products, four entries a
// lane, so no wave's loop is longer than that whatever share of the batch one pair holds.
constexpr int kPairSumUnit = 256;

// Units of a pair with `count` entries in the batch (none for an empty pair).
CPZ_HD uint32_t pair_sum_units(uint32_t count) { return (count + (uint32_t)kPairSumUnit - 1) / (uint32_t)kPairSumUnit; }

// Upper bound of the units of n entries over npairs pairs: every pair ends with at most one
// partial unit.
CPZ_HD int64_t pair_sum_max_units(int64_t n, int64_t npairs) { return n / kPairSumUnit + npairs; }

// The pair that owns unit u < ustart[npairs], ustart being the exclusive scan of the pairs'
// unit counts (npairs + 1 entries): the largest p with ustart[p] <= u, which has at least one
// unit because ustart[p + 1] > u.
CPZ_HD int pair_sum_find(const uint32_t* ustart, int npairs, uint32_t u) {
  int lo = 0, hi = npairs;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (ustart[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// The run of entries that starts at lo: the largest e <= hi such that pair_idx[lo .. e) holds at
// most max_pairs distinct values.  stamp: one word per pair, zero before the first call and
// marked with `tag` here (a non-zero value no earlier run used); the run's distinct pairs go to
// run_pairs (room for max_pairs) in the order they first appear, their number to *nrun.
CPZ_HD int64_t pair_run_end(const uint32_t* pair_idx, int64_t lo, int64_t hi, uint32_t* stamp, uint32_t tag,
                            int max_pairs, uint32_t* run_pairs, int* nrun) {
  int k = 0;
  int64_t e = lo;
  for (; e < hi; e++) {
    const uint32_t p = pair_idx[e];
    if (stamp[p] == tag) continue;
    if (k == max_pairs) break;
    stamp[p] = tag;
    run_pairs[k++] = p;
  }
  *nrun = k;
  return e;
}

}  // namespace cpz
