"""The batches of the route trace (tests/test_gpu_route_trace.py, tools/route_trace.py): the
smallest of each kind that reaches one branch of the batch check's failure search.  The list only;
tools/route_trace.py runs a scenario and tests/golden/route_trace.json holds what each one gave.

api      "device": Gpu.verify_batch_device with statuses under the default pair;
         "pairs":  Gpu.verify_batch_pairs, entry i under pair i % npairs;
         "many":   Gpu.verify_batch_pairs_many, entry i under pair i % npairs.
forged   the entries whose s becomes s + 1; or density / seed: that share of the batch, drawn by
         numpy's default_rng(seed).
locate   verify_batch_pairs' argument.
env      environment of the call, which then runs in a child process.
"""
PART = 1 << 16  # an eighth of 2^19 entries: one top-level part of the bisection

SCENARIOS = [
    # default pair ------------------------------------------------------------------------------
    # one level of bisection above kLeaf = 2^16 (cuts aligned down to 256): the failing part is a leaf
    dict(name="default_one_level", api="device", n=65536 + 256, forged=[40000]),
    # five of the eight parts fail: the dense rule at the top level
    dict(name="default_dense_top", api="device", n=1 << 17, forged=[k * (1 << 14) + 100 for k in (0, 2, 3, 5, 7)]),
    # from kPartSparseMin = 2^19 a failing batch is partitioned; its one forgery is located
    dict(name="default_part_located", api="device", n=1 << 19, forged=[123456]),
    # two forgeries in one 128-proof block (verified whole) and one alone in another (located)
    dict(name="default_part_whole_and_located", api="device", n=1 << 19,
         forged=[1000 * 128 + 5, 1000 * 128 + 77, 3000 * 128 + 64]),
    # from kProbeMin = 2^20 the density probe runs: 0.3 % invalid, 10 of them among the 4096 sampled
    dict(name="default_probe_partitioned", api="device", n=1 << 20, density=0.003, seed=4),
    # 5 % invalid, 215 sampled: per proof, and the partial is 32 x 0xff
    dict(name="default_probe_per_proof", api="device", n=1 << 20, density=0.05, seed=4),
    # five pairs --------------------------------------------------------------------------------
    # one level of bisection above CPZ_PAIRS_MAX_PROOFS = 2048
    dict(name="pairs_one_level", api="pairs", npairs=5, n=2048 + 256, forged=[300]),
    # every part fails: the guard's sample is launched at the third, finds one failing block of
    # its 64, and the range goes to the partitioned search
    dict(name="pairs_guard_clean", api="pairs", npairs=5, n=1 << 19, forged=[k * PART + 1000 + 300 * k for k in range(8)]),
    # 1 % invalid: most sampled blocks fail and the range is verified per proof in bulk
    dict(name="pairs_guard_dense", api="pairs", npairs=5, n=1 << 19, density=0.01, seed=3),
    # CPZ_CALL_PARTITIONED: the partitioned search at once; two forgeries in one of three blocks
    dict(name="pairs_forced_partitioned", api="pairs", npairs=5, n=3 * 128, forged=[130, 140], locate="partitioned"),
    # more than CPZ_PAIRS_MAX pairs ---------------------------------------------------------------
    # one level of bisection, then a 256-entry leaf verified in runs of at most 64 pairs
    dict(name="many_leaf_in_runs", api="many", npairs=65, n=2048 + 256, forged=[300]),
    # 2048 entries hold 130 pairs: the deep policy cuts them down to single weight blocks
    dict(name="many_deep", api="many", npairs=130, n=2048, forged=[700]),
    # the same batch with the deep policy off: the whole batch in runs
    dict(name="many_deep_off", api="many", npairs=130, n=2048, forged=[700], env={"CPZ_PAIRS_MANY_DEEP": "0"}),
]
