// cpz_batch.hpp -- header-only C++ mirror of the reference's `verifier::batch::BatchVerifier`
// (kobby-pentangeli/chaum-pedersen-zkp, src/verifier/batch.rs:45-330) on top of the C ABI
// in cpz.h.  Same names, cap, error conditions and result order:
//
//   BatchVerifier()                      batch.rs:97       (new)
//   BatchVerifier::with_capacity(n)      batch.rs:113
//   len / is_empty / remaining_capacity  batch.rs:122-136
//   add / add_with_context               batch.rs:139-168  (cap MAX_BATCH_SIZE = 1000)
//   verify()                             batch.rs:171-183  -> one Result per entry
//   clear                                batch.rs:321-323
//   Proof::to_bytes / Proof::from_bytes  gadgets.rs:343-489 (from_bytes on the device parser)
//   Verifier: verify / verify_with_transcript / verify_response     verifier/mod.rs:42-172
//   Prover: prove_with_transcript (caller nonce) / statement        prover/mod.rs:86-131,
//                                                                    gadgets.rs:217-221
//
// Errors are returned, never thrown across the ABI; `Result` carries the reference's
// error kind (src/error.rs:5-17).  Points and scalars stay as their 32-byte encodings:
// decoding and all checks run on the GPU.  Verifier and BatchVerifier hold Proof values,
// which may have been built directly (Proof::new, gadgets.rs:317: no identity / zero-s
// checks), so their calls pass CPZ_CALL_EQUATIONS_ONLY -- the equations alone decide, as
// verify_one (batch.rs:185-231) and verify_with_transcript (verifier/mod.rs:120-171) do --
// for those calls only (the context's own mode, Device::set_commitment_checks, is untouched);
// proof_from_bytes still applies from_bytes' checks.
//
// BatchVerifier::verify issues exactly the call sequence of the Rust drop-in
// (rust/reference-patch/gpu.rs): entries grouped by Parameters in order of first appearance;
// a one-entry batch -> cpz_verify_each_ex (batch.rs:178-180, the rng untouched); otherwise
// 64 bytes per entry are drawn from the caller's rng, as the reference's random_scalar draws
// them (batch.rs:239-240), the first 32 keying every group's RLC check; groups take
// consecutive weight indices (first_index), and a group of at least rlc_min_group entries runs
// cpz_verify_batch_ex (RLC + exact fallback), a smaller one cpz_verify_each_ex.
// set_merge_groups(true) (off by default, so the sequence above stays the drop-in's): two or
// more smaller groups go out together as one cpz_verify_each_pairs_ex call per CPZ_PAIRS_MAX
// groups -- one verify launch, every entry under its own pair -- with the same statuses.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <optional>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "cpz.h"

namespace chaum_pedersen {

constexpr std::size_t MAX_BATCH_SIZE = 1000;  // batch.rs:48

// Smallest Parameters group that takes the RLC batch check rather than per-proof
// verification (both return verify_one's outcome per entry).  The same threshold as
// rust/reference-patch/gpu.rs (RLC_MIN_GROUP), from the per-call latency table
// bench.py's small_batch (profiles/r05_bench_i.json): one synchronous host-buffer call takes
// 0.112-0.118 ms per proof at n = 1 .. 100 (k_verify_wide) and 0.265 ms at 1000 (k_verify_small),
// against 0.54-0.59 ms through the RLC check at n <= 100 and 0.73 ms at 1000, so no group of at most MAX_BATCH_SIZE entries takes
// the RLC check (set_rlc_min_group lowers it; a one-entry batch is then keyed by the OS's
// randomness, not the caller's).
constexpr std::size_t RLC_MIN_GROUP = 1001;

using Bytes32 = std::array<uint8_t, 32>;

enum class ErrorKind { None, InvalidParams, InvalidScalar, InvalidGroupElement, Device };

struct Result {
  ErrorKind kind = ErrorKind::None;
  std::string message;
  bool is_ok() const { return kind == ErrorKind::None; }
  bool is_err() const { return !is_ok(); }
  static Result ok() { return Result{}; }
  static Result err(ErrorKind k, std::string m) { return Result{k, std::move(m)}; }
};

inline Result status_result(uint8_t st) {
  switch (st) {
    case CPZ_STATUS_OK: return Result::ok();
    case CPZ_STATUS_EQ_FAIL: return Result::err(ErrorKind::InvalidParams, "Proof verification failed");
    case CPZ_STATUS_BAD_POINT:
      return Result::err(ErrorKind::InvalidGroupElement, "Bytes do not represent a valid Ristretto point");
    case CPZ_STATUS_BAD_SCALAR: return Result::err(ErrorKind::InvalidScalar, "Bytes do not represent a valid scalar");
    case CPZ_STATUS_IDENTITY: return Result::err(ErrorKind::InvalidParams, "Commitment contains identity element");
    default: return Result::err(ErrorKind::InvalidParams, "Response scalar is zero");  // CPZ_STATUS_ZERO_S
  }
}

class Device;

struct Parameters {  // gadgets.rs:25-118
  Bytes32 g, h;
  Parameters() { cpz_default_generators(g.data(), h.data()); }
  Parameters(const Bytes32& g_, const Bytes32& h_) : g(g_), h(h_) {}
  // The pair derived from a label by hashing to the group (cpz_derive_pairs): g and h are
  // from_uniform_bytes(SHA-512(CPZ_PAIR_DST_G / CPZ_PAIR_DST_H || label)), generator_h()'s
  // construction (ristretto.rs:86-91), so nobody knows a discrete logarithm between them.
  static Result from_label(Device& dev, const uint8_t* label, std::size_t len, Parameters* out);
};

struct Statement {  // gadgets.rs:177-239
  Bytes32 y1, y2;
};

struct Proof {  // gadgets.rs:245-311
  Bytes32 r1, r2, s;

  // gadgets.rs:343-361: [version 1][u32be 32][r1][u32be 32][r2][u32be 32][s] = 109 bytes.
  std::vector<uint8_t> to_bytes() const {
    std::vector<uint8_t> out{1};
    for (const Bytes32* f : {&r1, &r2, &s}) {
      const uint8_t len[4] = {0, 0, 0, 32};
      out.insert(out.end(), len, len + 4);
      out.insert(out.end(), f->begin(), f->end());
    }
    return out;
  }
};

// The reference's error for a CPZ_PARSE_* code (gadgets.rs:364-489).
inline Result parse_result(uint8_t code, uint32_t aux) {
  const std::string a = std::to_string(aux);
  switch (code) {
    case CPZ_PARSE_OK: return Result::ok();
    case CPZ_PARSE_TOO_SMALL: return Result::err(ErrorKind::InvalidParams, "Proof too small: " + a + " bytes");
    case CPZ_PARSE_BAD_VERSION: return Result::err(ErrorKind::InvalidParams, "Unsupported proof version: " + a);
    case CPZ_PARSE_R1_LEN_MISSING: return Result::err(ErrorKind::InvalidParams, "Truncated proof: missing r1 length");
    case CPZ_PARSE_R1_LEN_INVALID: return Result::err(ErrorKind::InvalidParams, "Invalid r1 length: " + a);
    case CPZ_PARSE_R1_TRUNCATED: return Result::err(ErrorKind::InvalidParams, "Truncated proof: incomplete r1 data");
    case CPZ_PARSE_R2_LEN_MISSING: return Result::err(ErrorKind::InvalidParams, "Truncated proof: missing r2 length");
    case CPZ_PARSE_R2_LEN_INVALID: return Result::err(ErrorKind::InvalidParams, "Invalid r2 length: " + a);
    case CPZ_PARSE_R2_TRUNCATED: return Result::err(ErrorKind::InvalidParams, "Truncated proof: incomplete r2 data");
    case CPZ_PARSE_R1_SIZE:
    case CPZ_PARSE_R2_SIZE: return Result::err(ErrorKind::InvalidGroupElement, "Expected 32 bytes, got " + a);
    case CPZ_PARSE_R1_POINT:
    case CPZ_PARSE_R2_POINT:
      return Result::err(ErrorKind::InvalidGroupElement, "Bytes do not represent a valid Ristretto point");
    case CPZ_PARSE_S_LEN_MISSING: return Result::err(ErrorKind::InvalidParams, "Truncated proof: missing s length");
    case CPZ_PARSE_S_LEN_INVALID: return Result::err(ErrorKind::InvalidParams, "Invalid s length: " + a);
    case CPZ_PARSE_S_TRUNCATED: return Result::err(ErrorKind::InvalidParams, "Truncated proof: incomplete s data");
    case CPZ_PARSE_S_SIZE: return Result::err(ErrorKind::InvalidScalar, "Expected 32 bytes, got " + a);
    case CPZ_PARSE_S_SCALAR: return Result::err(ErrorKind::InvalidScalar, "Bytes do not represent a valid scalar");
    case CPZ_PARSE_TRAILING: return Result::err(ErrorKind::InvalidParams, "Proof has " + a + " trailing bytes");
    case CPZ_PARSE_IDENTITY: return Result::err(ErrorKind::InvalidParams, "Commitment contains identity element");
    default: return Result::err(ErrorKind::InvalidParams, "Response scalar is zero");  // CPZ_PARSE_ZERO_S
  }
}

// One GPU context; shareable by many BatchVerifiers on one thread.
class Device {
 public:
  explicit Device(int ordinal = 0) { rc_ = cpz_ctx_create(ordinal, &ctx_); }
  ~Device() { cpz_ctx_destroy(ctx_); }
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;
  bool ok() const { return rc_ == CPZ_OK && ctx_ != nullptr; }
  cpz_ctx* get() const { return ctx_; }
  // cpz_ctx_set_commitment_checks: the context's mode for every later call on it (the mirrors
  // below do not use it: their calls pass CPZ_CALL_EQUATIONS_ONLY)
  int set_commitment_checks(bool on) { return cpz_ctx_set_commitment_checks(ctx_, on ? 1 : 0); }

 private:
  cpz_ctx* ctx_ = nullptr;
  int rc_ = CPZ_EINVAL;
};

inline Result Parameters::from_label(Device& dev, const uint8_t* label, std::size_t len, Parameters* out) {
  const uint64_t off[2] = {0, len};
  const uint8_t pad = 0;
  uint8_t row[64];
  const int rc = cpz_derive_pairs(dev.get(), 1, len ? label : &pad, off, row);
  if (rc == CPZ_EINVAL || rc == CPZ_EGENERATOR) return Result::err(ErrorKind::InvalidParams, cpz_last_error());
  if (rc != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
  if (out) {
    std::memcpy(out->g.data(), row, 32);
    std::memcpy(out->h.data(), row + 32, 32);
  }
  return Result::ok();
}

// Statement::validate (gadgets.rs:234-238 -> ristretto.rs:173-185): y1 and y2 must be group
// elements, i.e. their encodings must decode (on the device).
inline Result validate_statement(Device& dev, const Statement& st) {
  uint8_t pts[64], ok[2] = {0, 0};
  std::memcpy(pts, st.y1.data(), 32);
  std::memcpy(pts + 32, st.y2.data(), 32);
  if (cpz_decode_points(dev.get(), 2, pts, ok, nullptr) != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
  if (!ok[0] || !ok[1]) return Result::err(ErrorKind::InvalidGroupElement, "Element failed recompression validation");
  return Result::ok();
}

// Proof::from_bytes (gadgets.rs:364-489) through the device parser: the reference's checks
// in its order (point decodes and canonical-scalar checks included), first failure wins.
inline Result proof_from_bytes(Device& dev, const uint8_t* blob, std::size_t len, Proof* out) {
  const uint64_t off[2] = {0, len};
  Proof p;
  uint8_t code = 0;
  uint32_t aux = 0;
  const uint8_t pad = 0;
  const int rc = cpz_parse_proofs(dev.get(), 1, len ? blob : &pad, off, p.r1.data(), p.r2.data(), p.s.data(), &code,
                                  &aux);
  if (rc != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
  Result r = parse_result(code, aux);
  if (r.is_ok() && out) *out = p;
  return r;
}

// Verifier (verifier/mod.rs:42-172) for one statement; each call is a 1-entry device call.
class Verifier {
 public:
  Verifier(Device& dev, Parameters params, Statement st) : dev_(&dev), params_(params), st_(st) {}
  // verifier/mod.rs:85-88 (fresh transcript) and :120-139 (transcript with an optional context)
  Result verify(const Proof& pr) const { return verify_with_transcript(pr, std::nullopt); }
  Result verify_with_transcript(const Proof& pr, const std::optional<std::vector<uint8_t>>& context) const {
    Result v = validate_statement(*dev_, st_);  // verifier/mod.rs:121
    if (v.is_err()) return v;
    uint8_t st = 0, present = context ? 1 : 0, pad = 0;
    const uint64_t off[2] = {0, context ? context->size() : 0};
    const uint8_t* cb = (context && !context->empty()) ? context->data() : &pad;
    const int rc = cpz_verify_each_ex(dev_->get(), CPZ_CALL_EQUATIONS_ONLY, params_.g.data(), params_.h.data(), 1,
                                      st_.y1.data(), st_.y2.data(), pr.r1.data(), pr.r2.data(), pr.s.data(),
                                      context ? cb : nullptr, context ? off : nullptr, context ? &present : nullptr,
                                      &st);
    if (rc != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
    return status_result(st);
  }
  // verifier/mod.rs:144-171: the caller's challenge (32 canonical little-endian bytes)
  Result verify_response(const Bytes32& challenge, const Proof& pr) const {
    uint8_t st = 0;
    const int rc = cpz_verify_response_ex(dev_->get(), CPZ_CALL_EQUATIONS_ONLY, params_.g.data(), params_.h.data(), 1,
                                          st_.y1.data(), st_.y2.data(), pr.r1.data(), pr.r2.data(), pr.s.data(),
                                          challenge.data(), &st);
    if (rc != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
    return status_result(st);
  }

 private:
  Device* dev_;
  Parameters params_;
  Statement st_;
};

// Prover (prover/mod.rs:25-132) for one witness x; the nonce k is the caller's (commit draws it
// from an rng in the reference, :115-121).
class Prover {
 public:
  Prover(Device& dev, Parameters params, Bytes32 x) : dev_(&dev), params_(params), x_(x) {}
  // prover/mod.rs:86-110: proof (and the statement y = x g, x h) for nonce k.
  Result prove_with_transcript(const Bytes32& k, const std::optional<std::vector<uint8_t>>& context, Proof* proof,
                               Statement* statement = nullptr) const {
    Statement st;
    Proof pr;
    uint8_t present = context ? 1 : 0, pad = 0;
    const uint64_t off[2] = {0, context ? context->size() : 0};
    const uint8_t* cb = (context && !context->empty()) ? context->data() : &pad;
    const int rc = cpz_prove(dev_->get(), params_.g.data(), params_.h.data(), 1, x_.data(), k.data(),
                             context ? cb : nullptr, context ? off : nullptr, context ? &present : nullptr,
                             st.y1.data(), st.y2.data(), pr.r1.data(), pr.r2.data(), pr.s.data());
    if (rc != CPZ_OK) return Result::err(ErrorKind::Device, cpz_last_error());
    if (proof) *proof = pr;
    if (statement) *statement = st;
    return Result::ok();
  }

 private:
  Device* dev_;
  Parameters params_;
  Bytes32 x_;
};

class BatchVerifier {
 public:
  explicit BatchVerifier(Device& dev) : dev_(&dev) {}
  static BatchVerifier with_capacity(Device& dev, std::size_t cap) {
    BatchVerifier b(dev);
    b.entries_.reserve(cap < MAX_BATCH_SIZE ? cap : MAX_BATCH_SIZE);
    return b;
  }

  std::size_t len() const { return entries_.size(); }
  bool is_empty() const { return entries_.empty(); }
  std::size_t remaining_capacity() const { return entries_.size() >= MAX_BATCH_SIZE ? 0 : MAX_BATCH_SIZE - entries_.size(); }

  Result add(const Parameters& p, const Statement& st, const Proof& pr) { return add_with_context(p, st, pr, std::nullopt); }

  Result add_with_context(const Parameters& p, const Statement& st, const Proof& pr,
                          std::optional<std::vector<uint8_t>> context) {
    if (entries_.size() >= MAX_BATCH_SIZE)
      return Result::err(ErrorKind::InvalidParams, "Batch size limit exceeded (max 1000)");
    Result v = validate_statement(*dev_, st);  // batch.rs:158
    if (v.is_err()) return v;
    entries_.push_back(Entry{p, st, pr, std::move(context)});
    return Result::ok();
  }

  void clear() { entries_.clear(); }

  // The caller's randomness (the reference's rng: &mut impl CryptoRngCore, batch.rs:171):
  // fills `len` bytes.  os_rng reads the OS entropy source.
  using FillBytes = std::function<void(uint8_t*, std::size_t)>;
  static void os_rng(uint8_t* out, std::size_t len) {
    std::random_device rd;
    for (std::size_t i = 0; i < len; i += 4) {
      const uint32_t v = rd();
      for (std::size_t k = 0; k < 4 && i + k < len; k++) out[i + k] = (uint8_t)(v >> (8 * k));
    }
  }

  // What verify issued for one Parameters group (tests: the drop-in's call sequence).
  struct Dispatch {
    bool rlc = false;             // cpz_verify_batch_ex (else cpz_verify_each_ex)
    std::size_t entries = 0;
    uint64_t first_index = 0;     // the group's first weight index
    Bytes32 seed{};               // the batch's seed (every group's)
    Bytes32 partial{};            // the group's RLC partial (rlc only)
    int batch_ok = 0;
    std::size_t pairs = 0;        // merged call (set_merge_groups): the Parameters groups it carries,
                                  // cpz_verify_each_pairs_ex over `entries` entries; 0 otherwise
  };

  // Groups of at least this many entries take the RLC check (RLC_MIN_GROUP by default).
  void set_rlc_min_group(std::size_t m) { rlc_min_group_ = m; }
  // Two or more groups below that threshold in one cpz_verify_each_pairs_ex call per
  // CPZ_PAIRS_MAX groups instead of one cpz_verify_each_ex call each (off by default).
  void set_merge_groups(bool on) { merge_groups_ = on; }

  // batch.rs:171-183.  `overall` is Err for an empty batch (and device failures); otherwise
  // the vector holds one Result per entry, in entry order.  `log` (optional) receives one
  // Dispatch per group, in group order.
  std::vector<Result> verify(Result* overall = nullptr) const { return verify(os_rng, overall); }
  std::vector<Result> verify(const FillBytes& rng, Result* overall = nullptr,
                             std::vector<Dispatch>* log = nullptr) const {
    if (overall) *overall = Result::ok();
    if (entries_.empty()) {
      if (overall) *overall = Result::err(ErrorKind::InvalidParams, "Cannot verify empty batch");
      return {};
    }
    std::vector<Result> out(entries_.size());
    // Parameters groups in order of first appearance (gpu.rs: a Vec searched per entry)
    std::vector<std::pair<Parameters, std::vector<std::size_t>>> groups;
    for (std::size_t i = 0; i < entries_.size(); i++) {
      std::size_t k = 0;
      while (k < groups.size() && !(groups[k].first.g == entries_[i].params.g && groups[k].first.h == entries_[i].params.h))
        k++;
      if (k == groups.size()) groups.push_back({entries_[i].params, {}});
      groups[k].second.push_back(i);
    }
    // The caller's rng is drawn exactly as the reference draws it, so a caller that keeps using a
    // seeded rng after verify sees the reference's stream: a one-entry batch is verify_one and
    // draws nothing (batch.rs:178-180; its RLC check, when the threshold is lowered to 1, is keyed
    // by a seed from the OS entropy source); a batch of n >= 2 draws one random_scalar, 64 bytes,
    // per entry (batch.rs:239-240, ristretto.rs:146-150), whatever entry point each group takes.
    // The first 32 bytes of the first draw key every group's RLC weights.
    const bool single = entries_.size() == 1;
    Bytes32 seed{};
    if (single) {
      if (entries_.size() >= rlc_min_group_) os_rng(seed.data(), seed.size());
    } else {
      uint8_t draw[64];
      for (std::size_t i = 0; i < entries_.size(); i++) {
        rng(draw, sizeof(draw));
        if (i == 0) std::memcpy(seed.data(), draw, seed.size());
      }
    }
    std::size_t small_groups = 0;
    for (const auto& grp : groups) small_groups += grp.second.size() < rlc_min_group_ ? 1 : 0;
    const bool merge = merge_groups_ && small_groups >= 2;
    uint64_t first_index = 0;
    for (const auto& grp : groups) {
      const auto& idx = grp.second;
      const std::size_t n = idx.size();
      if (merge && n < rlc_min_group_) {  // issued below, with the other small groups
        first_index += n;
        continue;
      }
      const Packed pk = pack(idx);
      const std::vector<uint8_t>&y1 = pk.y1, &y2 = pk.y2, &r1 = pk.r1, &r2 = pk.r2, &s = pk.s;
      std::vector<uint8_t> st(n);
      const uint8_t* cb = pk.cb();
      const uint64_t* co = pk.co();
      const uint8_t* cp = pk.cp();
      const Parameters& p = grp.first;
      Dispatch d;
      d.entries = n;
      d.first_index = first_index;
      int rc;
      if (n >= rlc_min_group_) {
        d.rlc = true;
        d.seed = seed;
        rc = cpz_verify_batch_ex(dev_->get(), CPZ_CALL_EQUATIONS_ONLY, p.g.data(), p.h.data(), n, y1.data(), y2.data(),
                                 r1.data(), r2.data(), s.data(), cb, co, cp, seed.data(), first_index,
                                 d.partial.data(), &d.batch_ok, st.data());
      } else {
        rc = cpz_verify_each_ex(dev_->get(), CPZ_CALL_EQUATIONS_ONLY, p.g.data(), p.h.data(), n, y1.data(), y2.data(),
                                r1.data(), r2.data(), s.data(), cb, co, cp, st.data());
      }
      if (rc != CPZ_OK) {
        if (overall) *overall = Result::err(ErrorKind::Device, cpz_last_error());
        return {};
      }
      first_index += n;
      if (log) log->push_back(d);
      for (std::size_t k = 0; k < n; k++) out[idx[k]] = status_result(st[k]);
    }
    if (merge) {
      // the small groups, CPZ_PAIRS_MAX per call, each call's entries in batch order
      std::size_t g0 = 0;
      while (g0 < groups.size()) {
        std::vector<uint8_t> gh;
        std::vector<std::pair<std::size_t, uint32_t>> ent;  // (entry, pair of this call)
        std::size_t g1 = g0;
        for (; g1 < groups.size() && gh.size() < 64 * (std::size_t)CPZ_PAIRS_MAX; g1++) {
          if (groups[g1].second.size() >= rlc_min_group_) continue;
          const uint32_t pair = (uint32_t)(gh.size() / 64);
          gh.insert(gh.end(), groups[g1].first.g.begin(), groups[g1].first.g.end());
          gh.insert(gh.end(), groups[g1].first.h.begin(), groups[g1].first.h.end());
          for (std::size_t i : groups[g1].second) ent.push_back({i, pair});
        }
        g0 = g1;
        if (ent.empty()) continue;
        std::sort(ent.begin(), ent.end());
        std::vector<std::size_t> idx(ent.size());
        std::vector<uint32_t> pair_idx(ent.size());
        for (std::size_t k = 0; k < ent.size(); k++) {
          idx[k] = ent[k].first;
          pair_idx[k] = ent[k].second;
        }
        const Packed pk = pack(idx);
        std::vector<uint8_t> st(idx.size());
        Dispatch d;
        d.entries = idx.size();
        d.pairs = gh.size() / 64;
        const int rc = cpz_verify_each_pairs_ex(dev_->get(), CPZ_CALL_EQUATIONS_ONLY, d.pairs, gh.data(), idx.size(),
                                                pair_idx.data(), pk.y1.data(), pk.y2.data(), pk.r1.data(), pk.r2.data(),
                                                pk.s.data(), pk.cb(), pk.co(), pk.cp(), st.data());
        if (rc != CPZ_OK) {
          if (overall) *overall = Result::err(ErrorKind::Device, cpz_last_error());
          return {};
        }
        if (log) log->push_back(d);
        for (std::size_t k = 0; k < idx.size(); k++) out[idx[k]] = status_result(st[k]);
      }
    }
    return out;
  }

 private:
  struct Entry {
    Parameters params;
    Statement statement;
    Proof proof;
    std::optional<std::vector<uint8_t>> context;
  };
  // The rows and contexts of entries idx, as one call takes them.
  struct Packed {
    std::vector<uint8_t> y1, y2, r1, r2, s, ctx_bytes, present;
    std::vector<uint64_t> off;
    bool any_ctx = false;
    const uint8_t* cb() const { return any_ctx ? ctx_bytes.data() : nullptr; }
    const uint64_t* co() const { return any_ctx ? off.data() : nullptr; }
    const uint8_t* cp() const { return any_ctx ? present.data() : nullptr; }
  };
  Packed pack(const std::vector<std::size_t>& idx) const {
    const std::size_t n = idx.size();
    Packed p;
    for (std::vector<uint8_t>* v : {&p.y1, &p.y2, &p.r1, &p.r2, &p.s}) v->resize(32 * n);
    p.present.resize(n);
    p.off.assign(n + 1, 0);
    for (std::size_t k = 0; k < n; k++) {
      const Entry& e = entries_[idx[k]];
      std::memcpy(&p.y1[32 * k], e.statement.y1.data(), 32);
      std::memcpy(&p.y2[32 * k], e.statement.y2.data(), 32);
      std::memcpy(&p.r1[32 * k], e.proof.r1.data(), 32);
      std::memcpy(&p.r2[32 * k], e.proof.r2.data(), 32);
      std::memcpy(&p.s[32 * k], e.proof.s.data(), 32);
      p.present[k] = e.context.has_value() ? 1 : 0;
      if (e.context) {
        p.any_ctx = true;
        p.ctx_bytes.insert(p.ctx_bytes.end(), e.context->begin(), e.context->end());
      }
      p.off[k + 1] = p.ctx_bytes.size();
    }
    if (p.ctx_bytes.empty()) p.ctx_bytes.push_back(0);
    return p;
  }
  Device* dev_;
  std::vector<Entry> entries_;
  std::size_t rlc_min_group_ = RLC_MIN_GROUP;
  bool merge_groups_ = false;
};

}  // namespace chaum_pedersen
