// BatchVerifier::set_merge_groups (include/cpz_batch.hpp): the same batch through the default
// per-group call sequence and through the merged dispatch -- the small Parameters groups in one
// cpz_verify_each_pairs_ex call -- must give the same Result per entry, and the merged log must
// hold one Dispatch carrying all the groups.  Self-checking; driven by tests/test_gpu_pairs_cpp.py:
//   merge_groups_test <groups> <entries>
// Pairs and proofs are made on the device (Prover): pair j is (g_j, h_j) = ([a_j] B, [a_j] h_0),
// the statement of witness a_j under the default pair.  Entry i belongs to group i % groups and
// carries a context of i % 3 == 0: none, 1: 32 bytes, 2: 3 bytes; every 7th entry is forged
// (s of its neighbour) and must be rejected.  Prints "ok ..." and exits 0 when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <vector>

#include "cpz_batch.hpp"

using namespace chaum_pedersen;

static Bytes32 scalar(uint32_t tag, uint32_t i) {
  Bytes32 b{};
  for (int k = 0; k < 31; k++) b[k] = (uint8_t)(tag * 131u + i * 29u + k * 7u + 1u);  // < 2^248: canonical
  return b;
}

static int fail(const char* what, std::size_t i) {
  std::fprintf(stderr, "merge_groups_test: %s (%zu): %s\n", what, i, cpz_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::size_t groups = (std::size_t)std::atoi(argv[1]), n = (std::size_t)std::atoi(argv[2]);
  if (groups < 2 || groups > n || n > MAX_BATCH_SIZE) return 2;
  Device dev(0);
  if (!dev.ok()) return fail("no device", 0);
  std::vector<Parameters> pairs;
  for (std::size_t j = 0; j < groups; j++) {
    Statement st;
    Proof unused;
    if (Prover(dev, Parameters(), scalar(1, (uint32_t)j)).prove_with_transcript(scalar(2, (uint32_t)j), std::nullopt,
                                                                                &unused, &st).is_err())
      return fail("pair", j);
    pairs.push_back(Parameters(st.y1, st.y2));
  }
  BatchVerifier b(dev);
  std::vector<Proof> proofs(n);
  std::vector<Statement> sts(n);
  std::vector<std::optional<std::vector<uint8_t>>> ctxs(n);
  for (std::size_t i = 0; i < n; i++) {
    if (i % 3 == 1) ctxs[i] = std::vector<uint8_t>(32, (uint8_t)i);
    if (i % 3 == 2) ctxs[i] = std::vector<uint8_t>{1, 2, (uint8_t)i};
    if (Prover(dev, pairs[i % groups], scalar(3, (uint32_t)i)).prove_with_transcript(scalar(4, (uint32_t)i), ctxs[i],
                                                                                     &proofs[i], &sts[i]).is_err())
      return fail("prove", i);
  }
  for (std::size_t i = 0; i < n; i++) {
    Proof pr = proofs[i];
    if (i % 7 == 3) pr.s = proofs[(i + 1) % n].s;
    if (b.add_with_context(pairs[i % groups], sts[i], pr, ctxs[i]).is_err()) return fail("add", i);
  }
  Result overall;
  std::vector<BatchVerifier::Dispatch> log_each, log_merged;
  const std::vector<Result> each = b.verify(BatchVerifier::os_rng, &overall, &log_each);
  if (overall.is_err()) return fail("verify", 0);
  b.set_merge_groups(true);
  const std::vector<Result> merged = b.verify(BatchVerifier::os_rng, &overall, &log_merged);
  if (overall.is_err()) return fail("merged verify", 0);
  if (each.size() != n || merged.size() != n) return fail("result count", merged.size());
  for (std::size_t i = 0; i < n; i++) {
    if (each[i].is_ok() != (i % 7 != 3)) return fail("per-group result", i);
    if (merged[i].kind != each[i].kind || merged[i].message != each[i].message) return fail("merged result differs", i);
  }
  if (log_each.size() != groups) return fail("per-group dispatches", log_each.size());
  for (const auto& d : log_each)
    if (d.pairs != 0 || d.rlc) return fail("per-group dispatch kind", d.pairs);
  if (log_merged.size() != 1 || log_merged[0].pairs != groups || log_merged[0].entries != n || log_merged[0].rlc)
    return fail("merged dispatches", log_merged.size());
  std::printf("ok groups=%zu entries=%zu calls=%zu->%zu\n", groups, n, log_each.size(), log_merged.size());
  return 0;
}
