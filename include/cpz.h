/*
 * cpz.h -- C ABI of the MI355X-native Chaum-Pedersen / ristretto255 batch verifier.
 *
 * Drop-in boundary for the reference's `verifier::batch::BatchVerifier`
 * (kobby-pentangeli/chaum-pedersen-zkp, src/verifier/batch.rs).  Plain C: caller-owned
 * buffers, structure-of-arrays inputs, no callbacks, no torch/HIP types in signatures.
 * Every entry point returns an int status (CPZ_OK = 0, < 0 on error) and never aborts;
 * cpz_last_error() describes the most recent failure on the calling thread.
 *
 * Input layout (per proof i, each field a 32-byte little-endian encoding):
 *   y1[i], y2[i]  Statement (gadgets.rs:177-239), compressed ristretto255 points
 *   r1[i], r2[i]  Commitment (gadgets.rs:245-265), compressed ristretto255 points
 *   s[i]          Response (gadgets.rs:272-286), canonical scalar bytes
 * i.e. the bytes [5..37), [41..73), [77..109) of `Proof::to_bytes` (gadgets.rs:343-361)
 * plus the statement encodings.  Optional per-proof transcript contexts
 * (`add_with_context`, batch.rs:144-168) are given as one byte blob plus n + 1 offsets;
 * ctx_present distinguishes Some(b"") from None (NULL = every entry Some).
 *
 * Per-proof status codes (uint8):
 *   CPZ_STATUS_OK               Ok(())
 *   CPZ_STATUS_EQ_FAIL          Err(InvalidParams("Proof verification failed"))  batch.rs:224-228
 *   CPZ_STATUS_BAD_POINT        a point fails to decode (InvalidGroupElement)    ristretto.rs:120-138
 *   CPZ_STATUS_BAD_SCALAR       s is not canonical (InvalidScalar)                ristretto.rs:94-112
 *   CPZ_STATUS_IDENTITY         r1 or r2 is the identity (InvalidParams            gadgets.rs:474-478
 *                               "Commitment contains identity element")
 *   CPZ_STATUS_ZERO_S           s is zero (InvalidParams "Response scalar is zero")  gadgets.rs:480-482
 * Codes 2-5 are rejected by the reference before an entry can reach the batch
 * (`Proof::from_bytes`, service.rs:501-507); the bulk path reports them per entry.
 */
#ifndef CPZ_H_
#define CPZ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPZ_OK 0
#define CPZ_EINVAL (-1)     /* bad argument (null pointer, n == 0 where forbidden, misalignment) */
#define CPZ_EHIP (-2)       /* HIP runtime / kernel failure */
#define CPZ_ENOMEM (-3)     /* device or host allocation failed */
#define CPZ_EGENERATOR (-4) /* g or h does not decode to a valid, non-identity, distinct pair */
#define CPZ_EEMPTY (-5)     /* "Cannot verify empty batch" (batch.rs:172-176) */

#define CPZ_STATUS_OK 0
#define CPZ_STATUS_EQ_FAIL 1
#define CPZ_STATUS_BAD_POINT 2
#define CPZ_STATUS_BAD_SCALAR 3
#define CPZ_STATUS_IDENTITY 4
#define CPZ_STATUS_ZERO_S 5
#define CPZ_STATUS_BAD_GENERATOR 6 /* cpz_verify_each_gh only: the entry's own (g, h) is no valid pair */

/* ABI revision of this header (cpz_abi_version): bumped whenever an entry point's signature or
 * an array size it writes changes, so that callers built against another header can refuse
 * to run instead of passing wrongly sized buffers.  3: CPZ_NUM_STAGES = 16,
 * cpz_ctx_stage_times_n, cpz_ctx_set_commitment_checks.  4: per-call flags (the _ex entry
 * points, CPZ_CALL_EQUATIONS_ONLY), stage 7 (generator tables), density probe with contexts.
 * 5: CPZ_FALLBACK_STATS = 8 (the partitioned check's locate pass). */
#define CPZ_ABI_VERSION 5

typedef struct cpz_ctx cpz_ctx;

/* The CPZ_ABI_VERSION the library was built with. */
int cpz_abi_version(void);

/* Number of visible GPUs (0 when none / no HIP runtime). */
int cpz_device_count(void);

/* Create a verifier context bound to one GPU (one HIP stream, cached generator tables,
 * reusable device buffers).  Contexts serialise concurrent calls internally. */
int cpz_ctx_create(int device_ordinal, cpz_ctx **out);
void cpz_ctx_destroy(cpz_ctx *ctx);

/* Commitment checks (default on): statuses 4 (identity r1 / r2) and 5 (zero s) are the
 * rejections Proof::from_bytes applies (gadgets.rs:474-482) before a proof can reach the
 * service's batch (service.rs:501-507).  A Proof built with Proof::new(Commitment::new(..),
 * Response::new(..)) (gadgets.rs:252, 278, 317) skips them, and the reference's verify_one
 * (batch.rs:185-231) / verify_with_transcript (verifier/mod.rs:120-171) judge it by the two
 * equations alone -- e.g. a nonce k = 0 gives r1 = r2 = identity and an accepted proof.
 * enable = 0 gives exactly that: identity commitments and zero s are not reported, the
 * equations decide (and such entries keep their RLC weight).  Applies to every later call
 * on the context, from any thread: callers that share a context and need the equations-only
 * mode for their own calls pass CPZ_CALL_EQUATIONS_ONLY to the _ex entry points instead. */
int cpz_ctx_set_commitment_checks(cpz_ctx *ctx, int enable);

/* Per-call flags of the _ex entry points (cpz_verify_each_ex, cpz_verify_batch_ex,
 * cpz_verify_response_ex): each behaves as its plain form with these options for that call
 * alone -- the context's own mode and other threads' calls are unaffected.
 *   CPZ_CALL_EQUATIONS_ONLY  commitment checks off for this call (as
 *                            cpz_ctx_set_commitment_checks(ctx, 0)): what verify_one does
 *                            with a Proof value (the mirrors of BatchVerifier / Verifier). */
#define CPZ_CALL_EQUATIONS_ONLY 1u
/*   CPZ_CALL_PARTITIONED     cpz_verify_batch_pairs_ex alone (every other entry point ignores it,
 *                            and so does that one with npairs == 1): a failing batch with
 *                            status_out is searched by the partitioned check at once, whatever
 *                            its size, instead of by bisection -- for callers who know that
 *                            their invalid entries are too many for bisection to prune. */
#define CPZ_CALL_PARTITIONED 2u
/*   CPZ_CALL_PARTITIONED_MANY  cpz_verify_batch_pairs_many alone (every other entry point ignores
 *                            it): above CPZ_PAIRS_MAX pairs a failing batch with status_out is
 *                            searched by the partitioned check over block-local pair lists, with
 *                            every per-proof pass from the call's small per-pair tables, instead
 *                            of by bisection and runs; up to CPZ_PAIRS_MAX pairs the forwarded
 *                            call sees CPZ_CALL_PARTITIONED in its place.  Opt-in, not automatic.
 *                            2^20 entries over 4096 pairs with 0.1 % forged: 29.1 ms against
 *                            13.4 s unflagged and 59.7 ms for cpz_verify_each_pairs_many; from
 *                            1 % forged it loses to the latter (79.3 against 59.0 ms), as it
 *                            does below ~2^17 entries: see cpz_verify_batch_pairs_many. */
#define CPZ_CALL_PARTITIONED_MANY 4u

/* Thread-local description of the last error returned on this thread. */
const char *cpz_last_error(void);

/* Encodings of the default generators: g = ristretto255 basepoint, h = hash-to-group of
 * SHA-512("chaum-pedersen-zkp-v1.0.0-generator-h")   (ristretto.rs:27, 79-91). */
void cpz_default_generators(uint8_t g[32], uint8_t h[32]);

/* Per-proof verification of n proofs under generators (g, h).
 * Replaces BatchVerifier::verify (batch.rs:171-183) / verify_one (batch.rs:185-231):
 * status_out[i] is the outcome the reference reports for entry i.  Host buffers.
 * n == 0 -> CPZ_EEMPTY. */
int cpz_verify_each(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                    const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                    const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                    const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_each_ex(cpz_ctx *ctx, uint32_t flags, const uint8_t g[32], const uint8_t h[32], size_t n,
                       const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                       const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                       const uint8_t *ctx_present, uint8_t *status_out);

/* Per-proof verification of n proofs whose entries carry their own generators, in one call
 * and one verify launch: a BatchVerifier batch over several Parameters (batch.rs:52).
 * `pairs` holds npairs rows of 64 bytes (g then h), pair_idx[i] < npairs names entry i's row,
 * and status_out[i] is what cpz_verify_each_ex reports for entry i under that pair (every
 * status, flag, commitment-check mode and context shape).  Rows may repeat and may be the
 * default pair.  Every pair is verified from its 128-entry tables (a pair without cached
 * tables gets a light set, stage 13; no combs are built), all resident at once -- hence
 * CPZ_PAIRS_MAX, the light-set cache; CPZ_PAIRS_MAX_PROOFS is the latency kernels' bound.
 * Checked before anything is launched, cpz_last_error naming the index or entry:
 * n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_PAIRS_MAX, n > CPZ_PAIRS_MAX_PROOFS, a null
 * pointer or a pair_idx[i] >= npairs -> CPZ_EINVAL; a pair that is the identity, has g == h
 * or does not decode -> CPZ_EGENERATOR.  Host buffers only: the indices are checked on the
 * host.  For more than CPZ_PAIRS_MAX_PROOFS entries, or for rows already on the device, use
 * cpz_verify_each_pairs_bulk / cpz_verify_each_pairs_device below. */
#define CPZ_PAIRS_MAX 64
#define CPZ_PAIRS_MAX_PROOFS 2048
int cpz_verify_each_pairs(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                          const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                          const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                          const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                          const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_each_pairs_ex(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                             const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                             const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                             const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                             const uint8_t *ctx_present, uint8_t *status_out);

/* The mixed-pair per-proof call without the latency kernels' bound: up to
 * CPZ_PAIRS_BULK_MAX_PROOFS entries, from host buffers or from device-resident rows.  Every
 * argument means what it means for cpz_verify_each_pairs, and status_out[i] is what
 * cpz_verify_each_ex reports for entry i under pairs[pair_idx[i]] -- every status, with
 * CPZ_CALL_EQUATIONS_ONLY, the context's commitment-check mode and every context shape; rows of
 * `pairs` may repeat and may be the default pair.
 *   npairs == 1 is cpz_verify_each_ex (the device form: cpz_verify_each_device) under that pair.
 *   The host form with n <= CPZ_PAIRS_MAX_PROOFS is cpz_verify_each_pairs_ex.
 *   Otherwise every pair is made resident at once (light sets, stage 13; no combs), and the
 *   entries are verified in chunks of at most 16384 proofs (14080 on a 110-CU part: the table
 *   slab's bound), eight lanes per proof, every proof from its own pair's 128-entry tables; the
 *   chunks alternate over the context's verify streams and are joined at the end.
 * Both forms return synchronised.  The device form takes 16-byte aligned device rows and n
 * device-resident indices (`pairs` stays a host array of 64-byte rows), on `stream` (a
 * hipStream_t, or NULL for the context's own stream).  It first scans the indices on the device
 * and synchronises `stream` to read the result: no kernel that follows an index is enqueued
 * before that, and an offending index is CPZ_EINVAL naming the lowest such entry with
 * d_status_out untouched.  It then enqueues the chunks and synchronises `stream` again before it
 * returns.  Any later call on the same context, on any stream, is ordered after this call's
 * kernels (they read the context's cached tables and work buffers).
 * Checked before anything is launched (the device form: before anything but the index scan) or
 * written, in cpz_verify_each_pairs' order and wording, cpz_last_error naming the pair or the
 * entry: n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_PAIRS_MAX,
 * n > CPZ_PAIRS_BULK_MAX_PROOFS, a null pointer or a pair_idx[i] >= npairs -> CPZ_EINVAL; a pair
 * that is the identity, has g == h or does not decode -> CPZ_EGENERATOR. */
#define CPZ_PAIRS_BULK_MAX_PROOFS 1048576 /* 1 << 20, as CPZ_BATCH_PAIRS_MAX_PROOFS */
int cpz_verify_each_pairs_bulk(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                               const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                               const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                               const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                               const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_each_pairs_bulk_ex(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                                  const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                                  const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                                  const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                                  const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_each_pairs_device(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                                 const uint32_t *d_pair_idx, const void *d_y1, const void *d_y2,
                                 const void *d_r1, const void *d_r2, const void *d_s,
                                 const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                                 const uint8_t *d_ctx_present, void *d_status_out, void *stream);

/* cpz_verify_each_pairs_bulk_ex over up to CPZ_EACH_PAIRS_MANY_MAX (g, h) pairs: the same
 * arguments and the same statuses -- status_out[i] is what cpz_verify_each_ex reports for entry i
 * under pairs[pair_idx[i]], every status, with CPZ_CALL_EQUATIONS_ONLY, the context's
 * commitment-check mode and every context shape -- for callers who need exact statuses over more
 * pairs than a context keeps resident (a tenant per entry).  Rows of `pairs` may repeat, may be
 * the default pair and may have no entry; n may be up to CPZ_PAIRS_BULK_MAX_PROOFS.
 *   npairs <= CPZ_PAIRS_MAX is cpz_verify_each_pairs_bulk_ex itself (the call is forwarded):
 * resident 128-entry tables are the faster form where they fit (measured on MI355X at 64 pairs,
 * warm: the small tables take 1.36x the time at 16,384 entries and 1.065x at 2^20; cold they are
 * the faster form at 16,384 entries, 0.64x, and 1.03x at 2^20; profiles/each_pairs_many_ab.json).
 * CPZ_EACH_MANY_FORWARD=0 in the environment, read at every call, sends such calls down the path
 * below too (for measurement).
 *   Above that the call builds no 128-entry set and no comb: the descriptors are built on the
 * device, and every pair gets small tables -- the cached multiples 0..8 of g, 2^128 g, h and
 * 2^128 h, 5,760 bytes per pair, all pairs in one launch, recorded as one stage-13 span whose
 * launch count is npairs.  The entries are then verified in chunks as the bulk call's are, eight
 * lanes per proof, [s'] g and [s'] h from the pair's small tables by radix-16 digits (four
 * additions per window of the Straus loop instead of three).  The call does not touch the
 * light-set cache or its least-recently-used order (cpz_ctx_pairs_resident answers the same before
 * and after), keeps nothing across calls (the tables are rebuilt per call) and leaves
 * cpz_ctx_fallback_stats alone.
 * Checked before anything is launched or written, in cpz_verify_batch_pairs_many's order and
 * wording for the pairs and the bulk call's for the rest, cpz_last_error naming the lowest
 * offending pair or entry: n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_EACH_PAIRS_MANY_MAX,
 * n > CPZ_PAIRS_BULK_MAX_PROOFS, a null pointer, bad context offsets or a pair_idx[i] >= npairs ->
 * CPZ_EINVAL; a pair that is the identity, has g == h or does not decode (found by the descriptor
 * launch, before any table is built) -> CPZ_EGENERATOR.  status_out is not written on an error.
 * Host buffers only; the call returns synchronised. */
#define CPZ_EACH_PAIRS_MANY_MAX 4096
int cpz_verify_each_pairs_many(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                               const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                               const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                               const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                               const uint8_t *ctx_present, uint8_t *status_out);

/* Per-proof verification in which every entry carries its own generators: two more rows, g[i] and
 * h[i] (n x 32 bytes each), instead of a pair list and an index -- the shape of decryption-share
 * and VRF / OPRF evaluation proofs, where g is a fixed base and h a fresh point per proof (a
 * ciphertext component, a hashed input: cpz_hash_to_group_device can leave 2^20 of them in device
 * memory).  n may be up to CPZ_PAIRS_BULK_MAX_PROOFS; the number of distinct pairs has no bound.
 * Rows may repeat, and a row may be the default pair.
 *   status_out[i] is CPZ_STATUS_BAD_GENERATOR if Parameters::with_generators(g_i, h_i) would fail
 * (gadgets.rs:77-103): g_i or h_i does not decode, is the identity (32 zero bytes), or g_i == h_i
 * (encodings are canonical, so the bytes decide).  Status 6 wins over every other status -- in
 * the reference no entry exists under such parameters -- and is never a call-level error: these
 * calls do not return CPZ_EGENERATOR.  Otherwise status_out[i] is exactly what cpz_verify_each_ex
 * reports for entry i under (g_i, h_i): every status 0-5, with CPZ_CALL_EQUATIONS_ONLY, the
 * context's commitment-check mode and every context shape.
 *   The pair is used once, so nothing is built per pair and nothing is kept: every entry takes
 * the byte-wise transcript from the one snapshot no pair enters (stage 0), and the eight-lane
 * kernel decodes the entry's generator beside its Y and R and builds the small tables of B and
 * 2^128 B (cpz_verify_each_pairs_many's, 128 doublings per generator) in the proof's own scratch
 * (stages 1 / 5).  A proof keeps four tables per equation, so a launch holds half the eight-lane
 * bound: the chunk bound is half of it, 8192 proofs on the 256-CU MI355X (7040 on a 110-CU part);
 * the chunks alternate over the verify streams.  No cache is touched: neither the generator
 * cache nor the light-set cache nor its least-recently-used order (cpz_ctx_pairs_resident answers
 * the same before and after); no comb is built, no stage 7 or stage 13 is recorded, and
 * cpz_ctx_fallback_stats is left alone.
 *   Measured on MI355X (profiles/each_gh_ab.json, host buffers, medians, against
 * cpz_verify_each_pairs_many over consecutive slices of 4096 entries, a distinct pair per entry):
 * n = 1000: 0.69 ms (0.68 - 0.70) against 0.82 (0.81 - 0.85), one call on each side; n = 4096: 0.75
 * (0.74 - 0.78) against 0.95 (0.94 - 1.01), one call on each side; n = 2^17: 10.4 ms (10.3 - 10.7)
 * against 30.4 (29.8 - 30.8) for the 32 calls; n = 2^20: 77.5 ms (77.3 - 77.7) against 243.5 (241.5 -
 * 244.8) for the 256 calls, the verify launches taking 72.0 ms of GPU time (14.6 M proofs/s); every
 * pair of ranges apart.  When not to use it: where many entries share few pairs
 * cpz_verify_each_pairs_many builds a pair's tables once per call instead of once per proof -- 2^17
 * entries over 16 pairs take 9.74 ms (9.73 - 9.77) here against 6.78 (6.77 - 6.84) in one such call,
 * 1.44x the time.
 * Checked before anything is launched or written, in the bulk call's wording: n == 0 ->
 * CPZ_EEMPTY; a null pointer, n > CPZ_PAIRS_BULK_MAX_PROOFS, bad context offsets (host form) or
 * a device row that is not 16-byte aligned (device form) -> CPZ_EINVAL.
 *   cpz_verify_each_gh         host buffers; returns synchronised.
 *   cpz_verify_each_gh_device  device-resident rows; enqueues on `stream` (NULL: the context's
 *                              own) and does not synchronise: like cpz_verify_each_device, later
 *                              calls on the context are ordered after it, and the statuses are
 *                              the caller's to read after the stream's own synchronisation.  No
 *                              part of the call reads anything back to the host.
 *   cpz_challenges_gh          the entries' Fiat-Shamir challenges alone (32 bytes each), host
 *                              buffers; returns synchronised. */
int cpz_verify_each_gh(cpz_ctx *ctx, uint32_t flags, size_t n,
                       const uint8_t *g, const uint8_t *h,
                       const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                       const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                       const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_each_gh_device(cpz_ctx *ctx, uint32_t flags, size_t n,
                              const void *d_g, const void *d_h,
                              const void *d_y1, const void *d_y2, const void *d_r1, const void *d_r2,
                              const void *d_s, const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                              const uint8_t *d_ctx_present, void *d_status_out, void *stream);
int cpz_challenges_gh(cpz_ctx *ctx, size_t n, const uint8_t *g, const uint8_t *h,
                      const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                      const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
                      uint8_t *c_out);

/* The light-set cache behind the mixed-pair calls (cpz_verify_each_pairs*, cpz_prove_pairs*, the
 * fallback of cpz_verify_batch_pairs): a context keeps the 128-entry tables and transcript
 * prefixes of its CPZ_PAIRS_MAX most recently used pairs, and a call finds which of its pairs
 * have none and builds them all in ONE pass (two launches, one copy back, one synchronisation
 * for any number of pairs: stage 13, counted per set), evicting the least recently used sets
 * that the call itself does not read.  CPZ_PAIRS_BUILD_BATCH=0 in the environment, read at every
 * call, restores one build per pair (for measurement).
 *   cpz_ctx_load_pairs makes the npairs rows of `pairs` (64 bytes each, g then h; rows may
 * repeat and may be the default pair) resident without verifying anything: a service warms a
 * context before its first request, or before a call under another set of tenants.  A pair
 * with cached tables, full or light, keeps them and is marked most recently used.  *built_out
 * (optional) receives the number of sets built.  npairs == 0, npairs > CPZ_PAIRS_MAX or a null
 * ctx / pairs -> CPZ_EINVAL; a pair without cached tables that is the identity, has g == h or
 * does not decode -> CPZ_EGENERATOR, cpz_last_error naming the lowest such pair ("pair P: ..."),
 * with nothing launched and no cached set touched.
 *   cpz_ctx_pairs_resident writes resident_out[p] = 1 if row p has cached tables (full or
 * light: a mixed-pair call would build nothing for it), else 0.  It builds nothing and changes
 * neither the cache nor its least-recently-used order.  Same CPZ_EINVAL cases. */
int cpz_ctx_load_pairs(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t *built_out);
int cpz_ctx_pairs_resident(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, uint8_t *resident_out);

/* cpz_verify_each with device-resident, 16-byte aligned inputs/outputs, enqueued on `stream`
 * (a hipStream_t, or NULL for the context's own stream, which is a blocking stream and so
 * is ordered with the legacy default stream).  Does not synchronise.  Any later call on the
 * same context, on any stream, is ordered after this call's kernels (they read the context's
 * cached tables and work buffers). */
int cpz_verify_each_device(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                           const void *d_y1, const void *d_y2, const void *d_r1, const void *d_r2,
                           const void *d_s, const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                           const uint8_t *d_ctx_present, void *d_status_out, void *stream);

/* Fiat-Shamir challenges c_i (32-byte canonical scalars), bit-exact with
 * Transcript::challenge_scalar (transcript.rs:67-71) as built by batch.rs:188-206. */
int cpz_challenges(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                   const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                   const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
                   uint8_t *c_out);

/* Per-proof verification with caller-supplied challenges c_i (32-byte little-endian scalars):
 * Verifier::verify_response (verifier/mod.rs:144-171) -- g^s == r1 y1^c and h^s == r2 y2^c,
 * no transcript.  status_out[i] as for cpz_verify_each: the entry's decode-level checks first
 * (2, 3 for s, 4, 5), then CPZ_STATUS_BAD_SCALAR if c_i is not canonical (c_i >= l: what
 * scalar_from_bytes would reject, ristretto.rs:94-112), then 0 / 1.  n == 0 -> CPZ_EEMPTY. */
int cpz_verify_response(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                        const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                        const uint8_t *s, const uint8_t *c, uint8_t *status_out);
int cpz_verify_response_ex(cpz_ctx *ctx, uint32_t flags, const uint8_t g[32], const uint8_t h[32], size_t n,
                           const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                           const uint8_t *s, const uint8_t *c, uint8_t *status_out);
int cpz_verify_response_device(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                               const void *d_y1, const void *d_y2, const void *d_r1, const void *d_r2,
                               const void *d_s, const void *d_c, void *d_status_out, void *stream);

/* Batch prover from caller witnesses x_i and nonces k_i (32-byte little-endian scalars, taken
 * mod l): Prover::prove_with_transcript (prover/mod.rs:86-110) with commit's nonce supplied
 * (commit :115-121, respond :126-131) and the statement from the witness (gadgets.rs:217-221):
 *   y1 = x g, y2 = x h, r1 = k g, r2 = k h, c = the transcript challenge (optional per-proof
 *   contexts as in cpz_verify_each, appended first as the service does), s = k + c x.
 * Outputs are n x 32-byte encodings.  n == 0 -> CPZ_EEMPTY. */
int cpz_prove(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n, const uint8_t *x,
              const uint8_t *k, const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
              uint8_t *y1, uint8_t *y2, uint8_t *r1, uint8_t *r2, uint8_t *s);
int cpz_prove_device(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n, const void *d_x,
                     const void *d_k, const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                     const uint8_t *d_ctx_present, void *d_y1, void *d_y2, void *d_r1, void *d_r2, void *d_s,
                     void *stream);

/* The prover with a (g, h) pair per proof, in one call: `pairs` holds npairs host rows of 64
 * bytes (g then h), pair_idx[i] < npairs names entry i's row, and row i of every output is byte
 * for byte what cpz_prove writes for (x_i, k_i, context i) under pairs[pair_idx[i]].  Rows of
 * `pairs` may repeat and may be the default pair.  Every pair is made resident at once from its
 * 128-entry tables (a pair without cached tables gets a light set, stage 13) and every proof's
 * four points come from its own pair's tables: 24 doublings and at most 32 additions per point
 * against the comb's 16 additions, but no comb is ever built by these calls, for any npairs
 * (1 included) and any n up to CPZ_PROVE_PAIRS_MAX_PROOFS, and there is no chunking.  Kernel
 * time is reported under stage 6.
 * Both forms return synchronised.  The device form takes 16-byte aligned device rows and n
 * device-resident indices (`pairs` stays a host array), on `stream` (a hipStream_t, or NULL for
 * the context's own stream).  As cpz_verify_each_pairs_device it first scans the indices on the
 * device and synchronises `stream` to read the result: an offending index is CPZ_EINVAL naming
 * the lowest such entry, with every output untouched.  It then enqueues the prover and
 * synchronises `stream` again before it returns.  Any later call on the same context, on any
 * stream, is ordered after this call's kernels.
 * Checked before anything is launched (the device form: before anything but the index scan) or
 * written, in cpz_verify_each_pairs' order, cpz_last_error naming the pair or the entry:
 * n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_PAIRS_MAX, n > CPZ_PROVE_PAIRS_MAX_PROOFS, a
 * null pointer, a misaligned device row or a pair_idx[i] >= npairs -> CPZ_EINVAL; a pair that is
 * the identity, has g == h or does not decode -> CPZ_EGENERATOR. */
#define CPZ_PROVE_PAIRS_MAX_PROOFS 1048576 /* 1 << 20 */
int cpz_prove_pairs(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                    const uint32_t *pair_idx, const uint8_t *x, const uint8_t *k,
                    const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
                    uint8_t *y1, uint8_t *y2, uint8_t *r1, uint8_t *r2, uint8_t *s);
int cpz_prove_pairs_device(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                           const uint32_t *d_pair_idx, const void *d_x, const void *d_k,
                           const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                           const uint8_t *d_ctx_present, void *d_y1, void *d_y2, void *d_r1,
                           void *d_r2, void *d_s, void *stream);

/* cpz_prove_pairs / cpz_prove_pairs_device over up to CPZ_PROVE_PAIRS_MANY_MAX (g, h) pairs: the
 * same arguments and the same outputs -- row i of every output is byte for byte what cpz_prove
 * writes for (x_i, k_i, context i) under pairs[pair_idx[i]], scalars taken mod l, every context
 * shape -- for callers who prove under more pairs than a context keeps resident (a tenant per
 * entry).  Rows of `pairs` may repeat, may be the default pair and may have no entry; n may be up
 * to CPZ_PROVE_PAIRS_MAX_PROOFS.
 *   npairs <= CPZ_PAIRS_MAX is cpz_prove_pairs[_device] itself (the call is forwarded): resident
 * 128-entry tables take 24 doublings and at most 32 additions per point, the small tables about
 * 124 doublings and 64 additions.  CPZ_PROVE_MANY_FORWARD=0 in the environment, read at every
 * call, sends such calls down the path below too (for measurement).
 *   Above that the call builds no 128-entry set and no comb: the descriptors are built on the
 * device, and every pair gets small tables -- the cached multiples 0..8 of g, 2^128 g, h and
 * 2^128 h, 5,760 bytes per pair, all pairs in one launch, recorded as one stage-13 span whose
 * launch count is npairs.  Every proof's four points then come from its own pair's small tables,
 * four lanes per proof, by 2 x 32 signed radix-16 digits of the scalar (k_prove_points_micro), in
 * one launch for any n; challenges and responses as in cpz_prove_pairs.  Kernel time is reported
 * under stage 6.  The call does not touch the light-set cache or its least-recently-used order
 * (cpz_ctx_pairs_resident answers the same before and after), keeps nothing across calls (the
 * tables are rebuilt per call) and leaves cpz_ctx_fallback_stats alone.
 *   Measured on MI355X against the route it replaces -- cpz_prove_pairs in runs of at most
 * CPZ_PAIRS_MAX pairs on gathered rows -- medians (min - max) in ms, profiles/prove_pairs_many_ab.json
 * (tools/prove_pairs_many_ab.py): 1000 entries over 1000 pairs, 1.44 (1.44 - 1.44) against 31.7
 * (31.7 - 31.8) warm and 1.71 (1.66 - 1.78) against 32.3 (32.1 - 32.5) cold, 16 calls on the other
 * side.  2^17 and 2^20 entries over 4096 pairs, uniform or skewed, are not measured yet (the tool
 * runs them; the file holds no figure for them).  Where the new path is NOT the faster one: at 64
 * pairs, hence the forwarding -- CPZ_PROVE_MANY_FORWARD=0 against the forwarded call takes 1.60
 * (1.58 - 1.62) against 1.11 (1.10 - 1.14) ms at 16,384 entries and 59.9 (59.6 - 60.0) against 25.2
 * (25.1 - 26.3) ms at 2^20 warm, and 60.1 against 26.8 ms at 2^20 cold; only cold at 16,384 entries
 * are the small tables ahead, 1.98 (1.95 - 2.05) against 2.81 (2.76 - 3.16) ms.  The doubling and
 * addition counts above are derived from the code, not measured.
 * Both forms return synchronised.  The device form is cpz_prove_pairs_device's: 16-byte aligned
 * device rows, n device-resident indices (`pairs` stays a host array), `stream` a hipStream_t or
 * NULL for the context's own; it scans the indices on the device first and synchronises `stream`
 * to read the result -- an offending index is CPZ_EINVAL naming the lowest such entry, with every
 * output untouched -- and any later call on the same context, on any stream, is ordered after this
 * call's kernels.
 * Checked before anything is launched (the device form: before anything but the index scan) or
 * written, in cpz_prove_pairs' order and wording up to the indices and
 * cpz_verify_each_pairs_many's for the pairs, cpz_last_error naming the lowest offending pair or
 * entry: n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_PROVE_PAIRS_MANY_MAX,
 * n > CPZ_PROVE_PAIRS_MAX_PROOFS, a null pointer, a misaligned device row, bad context offsets or
 * a pair_idx[i] >= npairs -> CPZ_EINVAL; a pair that is the identity, has g == h or does not
 * decode (found by the descriptor launch, before any table is built) -> CPZ_EGENERATOR.  No
 * output is written on an error. */
#define CPZ_PROVE_PAIRS_MANY_MAX 4096
int cpz_prove_pairs_many(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                         const uint32_t *pair_idx, const uint8_t *x, const uint8_t *k,
                         const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
                         uint8_t *y1, uint8_t *y2, uint8_t *r1, uint8_t *r2, uint8_t *s);
int cpz_prove_pairs_many_device(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                                const uint32_t *d_pair_idx, const void *d_x, const void *d_k,
                                const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                                const uint8_t *d_ctx_present, void *d_y1, void *d_y2, void *d_r1,
                                void *d_r2, void *d_s, void *stream);

/* Synthetic input generator (Prover::prove_with_transcript, prover/mod.rs:86-131):
 * witness x_i and nonce k_i = from_bytes_mod_order_wide(ChaCha20(seed_x / seed_k, block
 * first_index + i)); writes y1 = x g, y2 = x h, r1 = k g, r2 = k h, s = k + c x. */
int cpz_prove_synthetic(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                        uint64_t first_index, const uint8_t seed_x[32], const uint8_t seed_k[32],
                        const uint8_t *ctx_bytes, const uint64_t *ctx_off, const uint8_t *ctx_present,
                        uint8_t *y1, uint8_t *y2, uint8_t *r1, uint8_t *r2, uint8_t *s);
int cpz_prove_synthetic_device(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                               uint64_t first_index, const uint8_t seed_x[32], const uint8_t seed_k[32],
                               const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                               const uint8_t *d_ctx_present, void *d_y1, void *d_y2, void *d_r1,
                               void *d_r2, void *d_s, void *stream);

/* Random-linear-combination batch verification (configs C3-C5): one Pippenger MSM checks
 *   P = sum_i [a_i s_i] g - [a_i] r1_i - [a_i c_i] y1_i + [b_i s_i] h - [b_i] r2_i - [b_i c_i] y2_i == O
 * -- the reference's verify_batch_equations (batch.rs:271-312) with the equation corrected
 * (the reference omits alpha on y*c, batch.rs:297-300).  Weights replace random_scalar
 * (batch.rs:240): the (first_index + i)-th ChaCha20 keystream block of `seed` read as 32
 * little-endian int16 words w_k; a_i = sum_{k<8} w_k 2^(16k), b_i = sum_{k<8} w_(8+k) 2^(16k)
 * (mod l) -- 128-bit weights, uniform over 2^128 values each (error <= 2^-128 per forged
 * entry), whose MSM digits are the words themselves.
 *   partial_out  32-byte encoding of P for this batch / shard (identity = 32 zero bytes);
 *                shards with global first_index values sum to the single-GPU P.
 *   batch_ok     1 iff every entry decodes and P is the identity.
 *   status_out   optional (n): exact per-entry statuses.  When the batch fails, a fallback
 *                search (sub-range RLC partials, per-proof verification at the leaves)
 *                locates the invalid entries (verify_individually, batch.rs:314-318).
 *                With a fallback, a batch of >= 2^20 entries (with or without contexts) is
 *                first sampled (4096 entries verified per proof, beside the batch's challenges):
 *                if two or more sampled entries are invalid the batch cannot pass and
 *                bisection could not prune it.  2 to 20 sampled invalid entries (density
 *                up to ~0.5 %): the partitioned check -- every 128-proof block's own RLC
 *                partial, then for the failing blocks an index-weighted second partial that
 *                locates a block's single invalid entry, per-proof verification of the
 *                located entries and of the blocks holding more; partial_out is the batch's
 *                partial as usual.  More: nothing is prepared, every entry is verified per
 *                proof, batch_ok = 0 and partial_out is 32 bytes of 0xff (not an encoding:
 *                "no partial computed").
 *   seed         must be secret and unpredictable to whoever produced the proofs (a CSPRNG
 *                draw per call, as the reference's random_scalar(rng) is, batch.rs:240): the
 *                weights' 2^-128 bound per forged entry, and the locate pass's ~2^-121 per
 *                failing block (CPZ_FALLBACK_STATS out[7]), hold only for weights the prover
 *                could not predict.  A seed an adversary knows lets forgeries cancel.
 * The _device form takes device-resident inputs and always needs d_status_out (decode-level
 * statuses, or exact ones when fallback != 0); it synchronises `stream`. */
int cpz_verify_batch(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                     const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                     const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                     const uint8_t *ctx_present, const uint8_t seed[32], uint64_t first_index,
                     uint8_t partial_out[32], int *batch_ok, uint8_t *status_out);
int cpz_verify_batch_ex(cpz_ctx *ctx, uint32_t flags, const uint8_t g[32], const uint8_t h[32], size_t n,
                        const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                        const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                        const uint8_t *ctx_present, const uint8_t seed[32], uint64_t first_index,
                        uint8_t partial_out[32], int *batch_ok, uint8_t *status_out);
int cpz_verify_batch_device(cpz_ctx *ctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                            const void *d_y1, const void *d_y2, const void *d_r1, const void *d_r2,
                            const void *d_s, const void *d_ctx_bytes, const uint64_t *d_ctx_off,
                            const uint8_t *d_ctx_present, const uint8_t seed[32], uint64_t first_index,
                            uint8_t partial_out[32], int *batch_ok, void *d_status_out, int fallback,
                            void *stream);

/* The same batch check over entries that carry their own generators, in one MSM: `pairs` and
 * pair_idx mean what they mean for cpz_verify_each_pairs (npairs rows of g then h, at most
 * CPZ_PAIRS_MAX; rows may repeat and may be the default pair).  Entry i is weighted by the
 * (first_index + i)-th weights of `seed` and takes the challenge of its own pair's transcript:
 *   P = sum_i [a_i s_i] g_p(i) - [a_i] r1_i - [a_i c_i] y1_i + [b_i s_i] h_p(i) - [b_i] r2_i - [b_i c_i] y2_i
 * -- the sum over the pairs of cpz_verify_batch's partial over that pair's entries, weights keyed
 * by the entries' positions in this call.  The MSM sees g_p and h_p as 2 npairs more points with
 * the per-pair sums of a_i s_i and b_i s_i as scalars, so a batch that passes builds no table
 * and no comb, whatever its pairs: only a failing batch with status_out makes its pairs resident
 * (light sets, stage 13), when its bisection reaches the first range of at most
 * CPZ_PAIRS_MAX_PROOFS entries, which the mixed-pair latency kernels verify, or a range most of
 * whose eight parts fail, which goes through cpz_verify_each_pairs_bulk's chunked eight-lane
 * path.  With every pair's tables already resident and n <= CPZ_PAIRS_MAX_PROOFS,
 * cpz_verify_each_pairs is the faster call (one launch); a caller that wants exact statuses of a
 * larger set whatever its validity calls cpz_verify_each_pairs_bulk; this one is for sets
 * expected to pass, and for pairs the context has not seen or too many to keep.
 *   partial_out, batch_ok   as for cpz_verify_batch (both required); shards with global
 *                first_index values combine (cpz_combine_partials) to the unsharded P.
 *   status_out   optional (n).  Entries with a non-zero decode-level status carry zero weight and
 *                report it; when the batch fails, every status is what cpz_verify_each_pairs_ex
 *                reports for that entry.  The fallback is the bisection (no density probe, hence
 *                CPZ_BATCH_PAIRS_MAX_PROOFS); a range of at least CPZ_BATCH_PAIRS_PART_MIN entries
 *                most of whose eight parts fail -- and with CPZ_CALL_PARTITIONED the whole failing
 *                batch -- goes to the partitioned check instead of per-proof verification: every
 *                128-entry block's partial with the block's own per-pair sums on its pairs'
 *                points, the failing blocks' index-weighted partials, and per-proof verification
 *                under each entry's own pair of the located entries and of the blocks holding
 *                more than one invalid entry.  Where more than half of the blocks fail, the
 *                range is verified per proof after all; the automatic route first looks at the
 *                partials of 64 blocks from the range's middle, computed beside the bisection's
 *                MSMs, and goes straight to per-proof verification if most of those fail.  The
 *                sample and the flag choose the route only: every route reports exact statuses.
 *   seed         secret and unpredictable, as for cpz_verify_batch.
 * CPZ_CALL_EQUATIONS_ONLY and the context's commitment-check mode apply as for cpz_verify_batch;
 * cpz_ctx_fallback_stats reports CPZ_FALLBACK_NONE, _BISECTION with out[4] and out[5], or
 * _PARTITIONED with out[2] .. out[7] (out[5] the bisection's MSMs before it).
 * npairs == 1 is cpz_verify_batch_ex under that pair.  Checked before anything is staged,
 * cpz_last_error naming the pair or the entry, and no output buffer is written on an error:
 * n == 0 -> CPZ_EEMPTY; npairs == 0, npairs > CPZ_PAIRS_MAX, n > CPZ_BATCH_PAIRS_MAX_PROOFS, a
 * null pointer (status_out and the contexts excepted) or a pair_idx[i] >= npairs -> CPZ_EINVAL; a
 * pair that is the identity, has g == h or does not decode -> CPZ_EGENERATOR.  Host buffers
 * only: the indices are checked on the host and the kernels trust them. */
#define CPZ_BATCH_PAIRS_MAX_PROOFS 1048576 /* 1 << 20 */
#define CPZ_BATCH_PAIRS_PART_MIN 524288 /* 1 << 19 */
int cpz_verify_batch_pairs(cpz_ctx *ctx, size_t npairs, const uint8_t *pairs, size_t n,
                           const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                           const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                           const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                           const uint8_t *ctx_present, const uint8_t seed[32], uint64_t first_index,
                           uint8_t partial_out[32], int *batch_ok, uint8_t *status_out);
int cpz_verify_batch_pairs_ex(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                              const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                              const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                              const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                              const uint8_t *ctx_present, const uint8_t seed[32], uint64_t first_index,
                              uint8_t partial_out[32], int *batch_ok, uint8_t *status_out);

/* cpz_verify_batch_pairs_ex over up to CPZ_BATCH_PAIRS_MANY_MAX (g, h) pairs in one MSM: the
 * same arguments, partial, batch_ok and statuses -- the sum over the pairs of cpz_verify_batch's
 * partial over that pair's entries, weights keyed by first_index + position, statuses what
 * cpz_verify_each_pairs_ex reports under each entry's own pair -- for callers with more pairs
 * than a context keeps resident (a tenant per entry, a bulk batch over thousands of tenants).
 * Rows of `pairs` may repeat, may be the default pair and may have no entry; shards combine
 * through cpz_combine_partials; CPZ_CALL_EQUATIONS_ONLY and the context's commitment-check mode
 * apply.  npairs <= CPZ_PAIRS_MAX is cpz_verify_batch_pairs_ex itself (the call is forwarded).
 * Above that:
 *   - a passing batch builds no table: the descriptors are built on the device, the entries are
 *     bucketed by pair once, and every MSM's per-pair sums cost O(n + npairs);
 *   - a failing batch with status_out is bisected (sub-range MSMs, no table), and each range
 *     that is verified per proof is cut into consecutive runs of at most CPZ_PAIRS_MAX distinct
 *     pairs, whose tables are built in one pass per run (stage 13 counts the sets built) before
 *     the run is verified;
 *   - CPZ_CALL_PARTITIONED is ignored: the partitioned check's lists hold CPZ_PAIRS_MAX pairs,
 *     so the route is bisection, then runs;
 *   - cpz_ctx_fallback_stats reports CPZ_FALLBACK_NONE or _BISECTION with out[4] and out[5].
 *   - CPZ_CALL_PARTITIONED_MANY (opt-in) sends a failing batch with status_out to the partitioned
 *     search at once instead: every pair's small tables in one launch (one stage-13 span whose
 *     launch count is npairs, as in cpz_verify_each_pairs_many), every 128-entry block's partial
 *     with the block's pairs in block-local slots (a pair's slot is its rank by first occurrence
 *     in the block, at most 128 of them whatever npairs is), the failing blocks' index-weighted
 *     partials, and per-proof verification from the small tables of the located entries and of
 *     the blocks not located (more than half of the blocks failing: of the whole batch).  No
 *     128-entry set is built, no run is formed, the light-set cache and its LRU order are
 *     untouched and stage 7 stays zero; partial_out, batch_ok and every status are as without
 *     the flag, and shards still combine.  cpz_ctx_fallback_stats then reports
 *     CPZ_FALLBACK_PARTITIONED with out[2] .. out[7] as for cpz_verify_batch_pairs_ex, out[1] = 0
 *     (no sample) and out[5] = 0.  A passing batch, or one without status_out, is unaffected.
 *     The route is not automatic: neither a size or density threshold nor a sampled guard like
 *     cpz_verify_batch_pairs_ex's chooses it unasked; both wait for measurements
 *     (tools/batch_pairs_many_part_ab.py writes profiles/batch_pairs_many_part_ab.json).
 *     Measured on an MI355X over 4096 pairs, flagged / unflagged / cpz_verify_each_pairs_many on
 *     the same rows, medians in ms: 2^20 entries, 1 forged 27.5 / 38.0 / 59.6; 0.1 % forged
 *     29.1 / 13,357 / 59.7; 1 % and 10 % forged (most blocks fail, everything is verified per
 *     proof after the block pass) 79.3-79.7 / 13,235-13,258 / 59.0-59.1 -- the route loses to
 *     cpz_verify_each_pairs_many there.  With 90 % of the entries in one pair: 24.2 / 35.9 /
 *     59.0, 25.8 / 1,719 / 59.0, 76.0-76.6 / 1,720-1,794 / 59.2-59.7.  2^17 entries: 1 forged
 *     8.2 / 20.3 / 8.4, 0.1 % 9.1 / 1,662 / 8.7, 1 % and 10 % 12.6 / 1,660-1,666 / 8.7 (skewed:
 *     7.5 / 17.1 / 8.6, 8.3 / 221 / 8.6, 12.0-12.1 / 220 / 8.5) -- no gain over
 *     cpz_verify_each_pairs_many at that size, and a loss from 1 %.  1000 entries over 1000
 *     pairs, 3 forged: 5.9 / 13.2 / 0.90 -- cpz_verify_each_pairs_many is the call to make.
 * Checked before anything is staged, in cpz_verify_batch_pairs_ex's order and wording,
 * cpz_last_error naming the lowest offending pair or entry, and no output buffer is written on
 * an error; npairs > CPZ_BATCH_PAIRS_MANY_MAX -> CPZ_EINVAL.  Host buffers only. */
#define CPZ_BATCH_PAIRS_MANY_MAX 4096
int cpz_verify_batch_pairs_many(cpz_ctx *ctx, uint32_t flags, size_t npairs, const uint8_t *pairs, size_t n,
                                const uint32_t *pair_idx, const uint8_t *y1, const uint8_t *y2,
                                const uint8_t *r1, const uint8_t *r2, const uint8_t *s,
                                const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                                const uint8_t *ctx_present, const uint8_t seed[32], uint64_t first_index,
                                uint8_t partial_out[32], int *batch_ok, uint8_t *status_out);

/* What the last cpz_verify_batch[_device] or cpz_verify_batch_pairs call on the context did to
 * locate invalid entries (fallback != 0, or status_out given), for tests and benchmarks; a
 * mixed-pair batch that reaches the partitioned check in several ranges reports their totals:
 *   out[0]  path: CPZ_FALLBACK_NONE (the batch passed, or no fallback), _BISECTION (sub-range
 *           RLC partials, per-proof leaves: a failed batch below 2^19 proofs), _PARTITIONED
 *           (every 128-proof block's partial, the failing blocks' index-weighted partials,
 *           per-proof verification of the located entries and of the blocks not located: the
 *           density probe's moderate densities, and a failed batch of 2^19 proofs or more),
 *           _PER_PROOF (dense: everything)
 *   out[1]  invalid entries the density probe saw (0 without a probe); cpz_verify_batch_pairs:
 *           failing blocks among the 64 sampled ahead of the partitioned check
 *   out[2]  blocks whose partial the partitioned check computed
 *   out[3]  blocks whose partial was not the identity
 *   out[4]  entries the fallback verified per proof
 *   out[5]  sub-range MSMs the bisection ran
 *   out[6]  failing blocks whose index-weighted partial the locate pass computed
 *   out[7]  of those, blocks whose one invalid entry it located (verified alone; the rest of
 *           such a block is accepted on P'_b = [j] P_b, error <= ~2^-121 per block for a seed
 *           the proofs' author could not predict -- see `seed` above; with a known seed an
 *           adversary could place two related forgeries in one block that pass as one) */
#define CPZ_FALLBACK_STATS 8
#define CPZ_FALLBACK_NONE 0
#define CPZ_FALLBACK_BISECTION 1
#define CPZ_FALLBACK_PARTITIONED 2
#define CPZ_FALLBACK_PER_PROOF 3
int cpz_ctx_fallback_stats(cpz_ctx *ctx, uint64_t out[CPZ_FALLBACK_STATS]);

/* Bulk Ristretto255::element_from_bytes (ristretto.rs:120-138) on the device: ok_out[i] = 1 iff
 * the 32-byte encoding points[i] decodes (RFC 9496), and, when reencoded_out is not NULL, the
 * element_to_bytes (ristretto.rs:141-143) encoding of the decoded point (32 zero bytes where
 * it does not decode).  Statement registration (service.rs:82-86) and parity checks use it. */
int cpz_decode_points(cpz_ctx *ctx, size_t n, const uint8_t *points, uint8_t *ok_out, uint8_t *reencoded_out);

/* Multi-scalar multiplication through the same Pippenger kernels: out = enc(sum_j [k_j] P_j)
 * for n encoded points and n scalars (little-endian, < 2^253), n <= 2^24 - 3 (CPZ_EINVAL above).
 * Exposed for testing the MSM against the oracle with adversarial digit patterns. */
int cpz_msm(cpz_ctx *ctx, size_t n, const uint8_t *points, const uint8_t *scalars, uint8_t out[32]);

/* Sum k 32-byte partials (per-GPU shards) on the device: out = encoding of the sum,
 * *is_identity = 1 iff the combined batch equation holds.  A partial of 32 x 0xff (a shard
 * whose fallback skipped its MSM, cpz_verify_batch) makes out 32 x 0xff and *is_identity 0:
 * the batch cannot pass.  CPZ_EINVAL if a partial does not decode. */
int cpz_combine_partials(cpz_ctx *ctx, size_t k, const uint8_t *partials, uint8_t out[32], int *is_identity);

/* Bulk wire-format ingestion: Proof::from_bytes (gadgets.rs:364-489) for n
 * 109-byte-format blobs at blob[off[i] .. off[i+1]), on the device.  Writes the r1, r2, s rows
 * (n x 32 B SoA, zero where not parsed) and one CPZ_PARSE_* code per blob -- the first check
 * the reference would fail, in its order (each field's structure, then its decode
 * element_from_bytes / scalar_from_bytes, before the next field; trailing bytes; identity
 * commitment; zero s).  aux_out (optional) holds the value the reference's message prints
 * (length, version or trailing-byte count).  Entries with a non-zero code are rejected before
 * batching, as the service does (service.rs:501-507). */
#define CPZ_PARSE_OK 0
#define CPZ_PARSE_TOO_SMALL 1        /* InvalidParams "Proof too small: {aux} bytes" */
#define CPZ_PARSE_BAD_VERSION 2      /* InvalidParams "Unsupported proof version: {aux}" */
#define CPZ_PARSE_R1_LEN_MISSING 3   /* InvalidParams "Truncated proof: missing r1 length" */
#define CPZ_PARSE_R1_LEN_INVALID 4   /* InvalidParams "Invalid r1 length: {aux}" */
#define CPZ_PARSE_R1_TRUNCATED 5     /* InvalidParams "Truncated proof: incomplete r1 data" */
#define CPZ_PARSE_R1_SIZE 6          /* InvalidGroupElement "Expected 32 bytes, got {aux}" */
#define CPZ_PARSE_R1_POINT 7         /* InvalidGroupElement "Bytes do not represent a valid Ristretto point" */
#define CPZ_PARSE_R2_LEN_MISSING 8   /* as 3..7 for r2 */
#define CPZ_PARSE_R2_LEN_INVALID 9
#define CPZ_PARSE_R2_TRUNCATED 10
#define CPZ_PARSE_R2_SIZE 11
#define CPZ_PARSE_R2_POINT 12
#define CPZ_PARSE_S_LEN_MISSING 13   /* InvalidParams "Truncated proof: missing s length" */
#define CPZ_PARSE_S_LEN_INVALID 14   /* InvalidParams "Invalid s length: {aux}" */
#define CPZ_PARSE_S_TRUNCATED 15     /* InvalidParams "Truncated proof: incomplete s data" */
#define CPZ_PARSE_S_SIZE 16          /* InvalidScalar "Expected 32 bytes, got {aux}" */
#define CPZ_PARSE_S_SCALAR 17        /* InvalidScalar "Bytes do not represent a valid scalar" */
#define CPZ_PARSE_TRAILING 18        /* InvalidParams "Proof has {aux} trailing bytes" */
#define CPZ_PARSE_IDENTITY 19        /* InvalidParams "Commitment contains identity element" */
#define CPZ_PARSE_ZERO_S 20          /* InvalidParams "Response scalar is zero" */
int cpz_parse_proofs(cpz_ctx *ctx, size_t n, const uint8_t *blob, const uint64_t *off, uint8_t *r1_out,
                     uint8_t *r2_out, uint8_t *s_out, uint8_t *code_out, uint32_t *aux_out);
int cpz_parse_proofs_device(cpz_ctx *ctx, size_t n, const void *d_blob, const uint64_t *d_off, void *d_r1,
                            void *d_r2, void *d_s, void *d_code, void *d_aux, void *stream);

/* Hash-to-group on the device: sound (g, h) pairs from labels.  generator_h() of the reference is
 * RistrettoPoint::from_uniform_bytes(SHA-512(dst)) (ristretto.rs:27, 86-91); these calls run that
 * construction -- FIPS 180-4 SHA-512, then the ristretto255 one-way map of RFC 9496 4.3.4 -- for n
 * messages at once, so that nobody knows a discrete logarithm between any two of the points.
 *   cpz_from_uniform_bytes  n rows of 64 uniform bytes -> n 32-byte encodings.  Bit 255 of each
 *                           32-byte half is ignored and a half in [p, 2^255) stands for its
 *                           residue, as dalek's FieldElement::from_bytes takes it.
 *   cpz_hash_to_group       points_out[i] = from_uniform_bytes(SHA-512(blob[off[i] .. off[i+1]))).
 *                           The message "chaum-pedersen-zkp-v1.0.0-generator-h" gives the h of
 *                           cpz_default_generators.
 *   cpz_derive_pairs        pairs_out row p (64 bytes, g then h) =
 *                           ( hash_to_group(CPZ_PAIR_DST_G || label_p),
 *                             hash_to_group(CPZ_PAIR_DST_H || label_p) ),
 *                           label_p = labels[off[p] .. off[p+1]); the rows go as they are into
 *                           every `pairs` argument of this header.  At most
 *                           CPZ_EACH_PAIRS_MANY_MAX labels; the 2 npairs prefixed messages are
 *                           built on the host and take one hash launch and one map launch.  Both
 *                           prefixes have one length and end in '/', so distinct labels give
 *                           distinct messages and the empty label does not give the default h.
 *                           The rows are then checked as every call checks its pairs: a row with
 *                           the identity or with g == h is CPZ_EGENERATOR naming the pair (no
 *                           label is known to reach this) and nothing is written.
 * Host forms: offsets as for cpz_parse_proofs (n + 1 of them, relative to off[0], non-decreasing).
 * n == 0 is CPZ_EEMPTY; a null pointer, n > CPZ_HASH_MAX_N (CPZ_EACH_PAIRS_MANY_MAX labels),
 * decreasing offsets or a message longer than CPZ_HASH_MAX_MSG bytes -- for cpz_derive_pairs the
 * label plus the prefix -- is CPZ_EINVAL, cpz_last_error naming the lowest offending entry.  Every
 * check is made before anything is launched or written; the calls return synchronised.
 * Device forms: enqueued on `stream` (NULL: the context's own) after the context's last call, not
 * synchronised, like cpz_verify_each_device.  d_points_out must be 16-byte aligned; the blob and
 * the uniform rows may start at any byte.  The offsets are trusted, except that every length is
 * clamped to CPZ_HASH_MAX_MSG in the kernel.
 * The calls record no stage and leave cpz_ctx_fallback_stats alone.
 * Measured (profiles/hash_to_group_ab.json, tools/hash_to_group_ab.py; host clocks around the
 * synchronous calls, medians): cpz_derive_pairs of 64 / 1000 / 4096 labels 0.20 / 0.35 / 0.80 ms,
 * cpz_hash_to_group of 2^16 short messages through the Python wrapper 8.3 ms.  The other side there is
 * the Python oracle's map, timed in the same run on 64 points (0.21 ms a point) and scaled, not run:
 * 27 / 420 / 1722 ms and 13.8 s. */
#define CPZ_HASH_MAX_MSG 4096 /* bytes per message */
#define CPZ_HASH_MAX_N 1048576 /* 1 << 20 */
#define CPZ_PAIR_DST_G "chaum-pedersen-zkp-v1.0.0-generator-g/"
#define CPZ_PAIR_DST_H "chaum-pedersen-zkp-v1.0.0-generator-h/"
int cpz_from_uniform_bytes(cpz_ctx *ctx, size_t n, const uint8_t *uniform, uint8_t *points_out);
int cpz_from_uniform_bytes_device(cpz_ctx *ctx, size_t n, const void *d_uniform, void *d_points_out, void *stream);
int cpz_hash_to_group(cpz_ctx *ctx, size_t n, const uint8_t *blob, const uint64_t *off, uint8_t *points_out);
int cpz_hash_to_group_device(cpz_ctx *ctx, size_t n, const void *d_blob, const uint64_t *d_off,
                             void *d_points_out, void *stream);
int cpz_derive_pairs(cpz_ctx *ctx, size_t npairs, const uint8_t *labels, const uint64_t *off, uint8_t *pairs_out);

/* Single-process multi-GPU forms: one context per GPU (e.g. the 8 GPUs of a node, or
 * several contexts on one GPU), the n proofs cut into nctx contiguous shards whose
 * boundaries are multiples of 256 proofs (the RLC weight-block granule), each shard
 * verified by its own context on its own host thread -- what a single host process behind
 * BatchVerifier::verify (batch.rs:171-183) uses instead of one process per GPU.
 *   cpz_verify_each_multi   per-proof statuses for all n (no data exchange).
 *   cpz_verify_batch_multi  per-shard RLC partials (weights keyed by the GLOBAL index, so
 *                           they sum to the single-GPU partial) -> partials_out (nctx x 32,
 *                           identity for an empty shard), combined on ctxs[0] ->
 *                           total_out; batch_ok = 1 iff every entry decodes and the sum is
 *                           the identity; status_out (optional, n) exact per entry, failing
 *                           shards running their own fallback search.
 * Contexts are given in shard order; the first failing shard's error is returned (its
 * message via cpz_last_error on the calling thread). */
int cpz_verify_each_multi(cpz_ctx *const *ctxs, int nctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                          const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                          const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                          const uint8_t *ctx_present, uint8_t *status_out);
int cpz_verify_batch_multi(cpz_ctx *const *ctxs, int nctx, const uint8_t g[32], const uint8_t h[32], size_t n,
                           const uint8_t *y1, const uint8_t *y2, const uint8_t *r1, const uint8_t *r2,
                           const uint8_t *s, const uint8_t *ctx_bytes, const uint64_t *ctx_off,
                           const uint8_t *ctx_present, const uint8_t seed[32], uint8_t *partials_out,
                           uint8_t total_out[32], int *batch_ok, uint8_t *status_out);

/* Per-kernel timing (HIP events recorded on the launch stream around every kernel).
 * Stages: 0 = k_challenge, 1 = k_verify_each, 2 = RLC decode/weights, 3 = RLC MSM,
 * 4 = fallback, 5 = the whole per-proof verify of one call (first to last k_verify_each,
 * whose launches overlap on several streams), 6 = prover (commitments / statements, then
 * challenges + responses; cpz_prove_pairs_many's point kernel and its challenges + responses
 * too), 7 = generator tables (a (g, h) pair's combs and transcript prefix
 * built: a cache miss, one launch each; a context keeps the tables of its 4 most recently used
 * pairs, or of CPZ_GEN_CACHE = 1..4 set in the environment when it is created, and frees the
 * others when a new pair's combs do not fit); phases of the RLC MSM (inside stage 3): 8 = bucket
 * sort, 9 = bucket accumulation (k_rlc_bucket), 10 = bucket fix-up, 11 = bucket reduction
 * (segment + window), 12 = window combine + encode (k_rlc_final16); 13 = variable-base generator
 * tables (a per-proof call of at most the eight-lane bound -- 16384 proofs on MI355X, smaller on
 * parts with fewer CUs -- on a pair other than the default one and
 * without combs in the cache builds only the pair's Niels tables and transcript prefix, ~0.5 ms
 * instead of ~3 ms, and verifies [s'] g, [s'] h from them; a context keeps 64 such pairs; a
 * mixed-pair call or cpz_ctx_load_pairs builds all of its missing pairs' tables in one pass,
 * recorded as one span whose launch count is the number of sets built; cpz_verify_each_pairs_many
 * and cpz_prove_pairs_many above CPZ_PAIRS_MAX pairs build every pair's small tables in one launch,
 * recorded as one span whose launch count is npairs);
 * phases of the partitioned check (inside stage 3): 14 = every block's bucket walk
 * (k_part_acc), 15 = the locate pass's walk over the failing blocks.
 * cpz_ctx_stage_times synchronises, writes the summed milliseconds and launch counts per stage
 * since the last call, and resets them. */
#define CPZ_NUM_STAGES 16
int cpz_ctx_set_timing(cpz_ctx *ctx, int enable);
int cpz_ctx_stage_times(cpz_ctx *ctx, double ms_out[CPZ_NUM_STAGES], int launches_out[CPZ_NUM_STAGES]);
/* The same for the first nstages stages only (arrays of nstages entries; launches_out may be
 * NULL): callers built against a header with another CPZ_NUM_STAGES pass their own size. */
int cpz_ctx_stage_times_n(cpz_ctx *ctx, int nstages, double *ms_out, int *launches_out);

#ifdef __cplusplus
}
#endif

#endif /* CPZ_H_ */
