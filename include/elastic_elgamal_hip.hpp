// elastic_elgamal_hip.hpp -- C++17 host-side mirror of the reference's interface for the ballot-verification
// path, header-only on top of the C ABI (eg_hip.h).  The reference is a compiled (Rust) library and no Rust
// toolchain exists in the build image, so this is the compiled-language face of the drop-in boundary; names,
// argument meaning and error variants follow the reference:
//   ChoiceParams::single / ::multi            src/app/choice.rs:160-196
//   EncryptedChoice::verify  (batched)        src/app/choice.rs:358-380      -> verify_batch
//   ChoiceVerificationError                   src/app/choice.rs:407-419
//   QuadraticVotingParams::new                src/app/quadratic_voting.rs:63-76
//   QuadraticVotingBallot::verify (batched)   src/app/quadratic_voting.rs:291-329
//   QuadraticVotingError                      src/app/quadratic_voting.rs:335-354
//   VerificationError                         src/proofs/mod.rs:63-80
//   CommitmentEquivalenceProof::verify / ::new (batched)   src/proofs/commitment.rs:186-238, 134-181
//   Ristretto (Group backend, batched)        src/group/ristretto.rs:23-146
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "eg_hip.h"

namespace elastic_elgamal_hip {

using Bytes = std::vector<uint8_t>;
using Scalar = std::array<uint8_t, 32>;    // canonical little-endian, < l
using Element = std::array<uint8_t, 32>;   // canonical ristretto255 encoding

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) { if (rc != EG_OK) throw Error(rc, eg_last_error()); }

class Context {
 public:
  explicit Context(int device = 0) { check(eg_init(device, &ctx_)); }
  ~Context() { eg_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  eg_ctx* raw() const { return ctx_; }
 private:
  eg_ctx* ctx_ = nullptr;
};

// VerificationError (proofs/mod.rs:63-80)
enum class VerificationError { ChallengeMismatch, LenMismatch };

// ChoiceVerificationError (choice.rs:407-419) + the deserialisation failures that serde reports earlier
struct ChoiceVerificationError {
  enum Kind { OptionsLenMismatch, Sum, Range, MalformedScalar, MalformedElement } kind;
  VerificationError inner = VerificationError::ChallengeMismatch;
  size_t item = 0;   // index of the malformed 32-byte item
  std::string to_string() const {
    switch (kind) {
      case OptionsLenMismatch: return "number of options in the ballot differs from expected";
      case Sum: return "cannot verify sum proof: restored challenge scalar does not match the one provided in the proof";
      case Range: return "cannot verify range proofs: restored challenge scalar does not match the one provided in the proof";
      case MalformedScalar: return "non-canonical scalar at item " + std::to_string(item);
      default: return "invalid group element at item " + std::to_string(item);
    }
  }
};
inline std::optional<ChoiceVerificationError> choice_error_from_status(uint32_t s) {
  switch (EG_STATUS_KIND(s)) {
    case EG_ST_OK: return std::nullopt;
    case EG_ST_BAD_SCALAR: return ChoiceVerificationError{ChoiceVerificationError::MalformedScalar, {}, EG_STATUS_DETAIL(s)};
    case EG_ST_BAD_POINT: return ChoiceVerificationError{ChoiceVerificationError::MalformedElement, {}, EG_STATUS_DETAIL(s)};
    case EG_ST_OPTIONS_LEN: return ChoiceVerificationError{ChoiceVerificationError::OptionsLenMismatch};
    case EG_ST_SUM_CHALLENGE: return ChoiceVerificationError{ChoiceVerificationError::Sum, VerificationError::ChallengeMismatch};
    case EG_ST_RANGE_LEN: return ChoiceVerificationError{ChoiceVerificationError::Range, VerificationError::LenMismatch};
    default: return ChoiceVerificationError{ChoiceVerificationError::Range, VerificationError::ChallengeMismatch};
  }
}

// QuadraticVotingError (quadratic_voting.rs:335-354)
struct QuadraticVotingError {
  enum Kind { Variant, CreditRange, CreditEquivalence, OptionsLenMismatch, MalformedScalar, MalformedElement } kind;
  size_t index = 0;   // Variant: zero-based option index; Malformed*: item index
  VerificationError inner = VerificationError::ChallengeMismatch;
};
inline std::optional<QuadraticVotingError> qv_error_from_status(uint32_t s) {
  const size_t d = EG_STATUS_DETAIL(s);
  switch (EG_STATUS_KIND(s)) {
    case EG_ST_OK: return std::nullopt;
    case EG_ST_BAD_SCALAR: return QuadraticVotingError{QuadraticVotingError::MalformedScalar, d};
    case EG_ST_BAD_POINT: return QuadraticVotingError{QuadraticVotingError::MalformedElement, d};
    case EG_ST_QV_VARIANT_LEN: return QuadraticVotingError{QuadraticVotingError::Variant, d, VerificationError::LenMismatch};
    case EG_ST_QV_VARIANT_CHALLENGE: return QuadraticVotingError{QuadraticVotingError::Variant, d};
    case EG_ST_QV_CREDIT_RANGE_LEN: return QuadraticVotingError{QuadraticVotingError::CreditRange, 0, VerificationError::LenMismatch};
    case EG_ST_QV_CREDIT_RANGE_CHALLENGE: return QuadraticVotingError{QuadraticVotingError::CreditRange};
    case EG_ST_QV_CREDIT_EQUIV_LEN: return QuadraticVotingError{QuadraticVotingError::CreditEquivalence, 0, VerificationError::LenMismatch};
    case EG_ST_QV_CREDIT_EQUIV_CHALLENGE: return QuadraticVotingError{QuadraticVotingError::CreditEquivalence};
    default: return QuadraticVotingError{QuadraticVotingError::OptionsLenMismatch};
  }
}

// Ciphertext (encryption.rs:96-101): random_element || blinded_element
struct Ciphertext { Element random_element{}, blinded_element{}; };

template <class E>
struct BatchVerdict {
  std::vector<std::optional<E>> results;   // per ballot: nullopt == Ok(..)
  std::vector<Ciphertext> totals;          // homomorphic sum of the ciphertexts of accepted ballots, per option
  size_t accepted() const { size_t n = 0; for (auto& r : results) n += !r.has_value(); return n; }
};

inline std::vector<Ciphertext> unpack_totals(const Bytes& t) {
  std::vector<Ciphertext> out(t.size() / 64);
  for (size_t k = 0; k < out.size(); ++k) {
    std::copy(t.begin() + 64 * k, t.begin() + 64 * k + 32, out[k].random_element.begin());
    std::copy(t.begin() + 64 * k + 32, t.begin() + 64 * k + 64, out[k].blinded_element.begin());
  }
  return out;
}

// Per-group tally of a verified batch (eg_*_tally_grouped): totals[g] = what the verify call's totals would be for the ballots of group
// g alone; accepted[g] = how many of them were accepted.
struct GroupedTally {
  std::vector<std::vector<Ciphertext>> totals;
  std::vector<uint32_t> accepted;
};
inline GroupedTally unpack_grouped(const Bytes& t, std::vector<uint32_t> counts, size_t options) {
  GroupedTally g;
  g.accepted = std::move(counts);
  for (size_t k = 0; k < g.accepted.size(); ++k) g.totals.push_back(unpack_totals(Bytes(t.begin() + 64 * options * k, t.begin() + 64 * options * (k + 1))));
  return g;
}

// Weighted per-group tally (eg_*_tally_weighted): totals[g] = the sum of weight x ciphertext over the accepted ballots of group g;
// weight_sums[g] = the exact sum of their weights, a 128-bit number (the bound for the discrete-log solver); accepted[g] as above.
struct WeightSum { uint64_t low, high; };
struct WeightedTally {
  std::vector<std::vector<Ciphertext>> totals;
  std::vector<WeightSum> weight_sums;
  std::vector<uint32_t> accepted;
};
inline WeightedTally unpack_weighted(const Bytes& t, const std::vector<uint64_t>& sums, std::vector<uint32_t> counts, size_t options) {
  GroupedTally g = unpack_grouped(t, std::move(counts), options);
  WeightedTally w;
  w.totals = std::move(g.totals);
  w.accepted = std::move(g.accepted);
  for (size_t k = 0; k < w.accepted.size(); ++k) w.weight_sums.push_back(WeightSum{sums[2 * k], sums[2 * k + 1]});
  return w;
}

// Ballot weeding (eg_*_weed): dup_of[b] = EG_DUP_NONE, EG_DUP_PRIOR (a ciphertext of b is on the board) or the smallest earlier ballot that
// shares a ciphertext with b; status = the caller's words with EG_ST_DUPLICATE for the flagged ballots (what a tally entry takes);
// appended = the ciphertexts of the participating, unflagged ballots in ballot and option order (64 bytes each): what joins the board.
struct Weeded {
  std::vector<uint32_t> dup_of, status;
  Bytes appended;
  size_t dropped() const { size_t d = 0; for (uint32_t v : dup_of) d += v != EG_DUP_NONE; return d; }
};

// Ballot audits (eg_*_open_check; eg_hip.h, "ballot audits" has the rule).  An Opening is what a challenged voting device reveals: per
// ballot and tally ciphertext the value and the 32 bytes of the encryption randomness.  Audited: status[b] = EG_ST_OK, the caller's word of
// a ballot that did not participate, or EG_ST_BAD_OPENING with EG_OPEN_DETAIL(slot, check).  An opened ballot must never be counted: weed
// the audited pile onto the board (weed(..., append = true)), so that a later copy of an opened ciphertext is EG_DUP_PRIOR.
struct Opening {
  std::vector<uint64_t> values;     // n x options_count()
  Bytes rand;                       // n x options_count() x 32
};
struct Audited {
  std::vector<uint32_t> status;
  uint32_t participated = 0, failed = 0;
};

// ChoiceParams<G, S> (choice.rs:132-196); S is SingleChoice (sum proof) or MultiChoice
class ChoiceParams {
 public:
  static ChoiceParams single(const Context& ctx, const Element& receiver, size_t options_count) { return ChoiceParams(ctx, receiver, options_count, true); }
  static ChoiceParams multi(const Context& ctx, const Element& receiver, size_t options_count) { return ChoiceParams(ctx, receiver, options_count, false); }
  ~ChoiceParams() { eg_choice_params_destroy(p_); }
  ChoiceParams(ChoiceParams&& o) noexcept : p_(o.p_), n_(o.n_), single_(o.single_) { o.p_ = nullptr; }
  ChoiceParams(const ChoiceParams&) = delete;
  ChoiceParams& operator=(const ChoiceParams&) = delete;
  ChoiceParams& operator=(ChoiceParams&&) = delete;
  size_t options_count() const { return n_; }
  size_t ballot_size() const { return eg_choice_ballot_size((int)n_, single_); }
  // EncryptedChoice::verify for every packed ballot + totals[k] += vote[k] (examples/voting.rs:199-203)
  BatchVerdict<ChoiceVerificationError> verify_batch(const Bytes& packed) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size())   // the analogue of check_options_count (choice.rs:149-158)
      throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots for these parameters");
    std::vector<uint32_t> st(n);
    Bytes tally(64 * n_);
    check(eg_verify_choice_batch(p_, n, packed.data(), st.data(), tally.data()));
    BatchVerdict<ChoiceVerificationError> v;
    for (uint32_t s : st) v.results.push_back(choice_error_from_status(s));
    v.totals = unpack_totals(tally);
    return v;
  }
  // the same for a handful of ballots (at most EG_SMALL_BATCH_MAX) with low latency: one workgroup per ballot in one launch
  BatchVerdict<ChoiceVerificationError> verify_small(const Bytes& packed) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size())
      throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots for these parameters");
    std::vector<uint32_t> st(n);
    Bytes tally(64 * n_);
    check(eg_verify_choice_small(p_, n, packed.data(), st.data(), tally.data()));
    BatchVerdict<ChoiceVerificationError> v;
    for (uint32_t s : st) v.results.push_back(choice_error_from_status(s));
    v.totals = unpack_totals(tally);
    return v;
  }
  // asynchronous device-pointer form of verify_small: verdicts into d_status, accepted ballots into the running tally
  void verify_small_device(size_t n, const void* d_ballots, void* d_status, void* stream = nullptr) const {
    check(eg_verify_choice_small_device(p_, n, d_ballots, d_status, stream));
  }
  // per-group tally of a verified batch: `status` = the words a verify entry wrote for `packed` (0 = accepted), groups[b] = group of ballot b
  // (EG_GROUP_NONE: in no group).  Stateless; throws EG_ERR_BAD_ARG for an accepted ballot with an id >= n_groups or an undecodable point.
  GroupedTally tally_grouped(const Bytes& packed, const std::vector<uint32_t>& status, const std::vector<uint32_t>& groups, uint32_t n_groups) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || status.size() != n || groups.size() != n)
      throw Error(EG_ERR_BAD_ARG, "packed, status and groups do not describe the same number of ballots");
    if (n_groups == 0 || n_groups > EG_TALLY_GROUPS_MAX) throw Error(EG_ERR_BAD_ARG, "n_groups out of range");
    Bytes tallies((size_t)n_groups * 64 * n_);
    std::vector<uint32_t> counts(n_groups);
    check(eg_choice_tally_grouped(p_, n, packed.data(), status.data(), groups.data(), n_groups, tallies.data(), counts.data()));
    return unpack_grouped(tallies, std::move(counts), n_);
  }
  // asynchronous device-pointer form: d_scratch of tally_grouped_scratch_bytes(n, n_groups) bytes, d_bad two uint32 the library writes
  size_t tally_grouped_scratch_bytes(size_t n, uint32_t n_groups) const { return eg_choice_tally_grouped_scratch_bytes(p_, n, n_groups); }
  void tally_grouped_device(size_t n, const void* d_ballots, const void* d_status, const void* d_groups, uint32_t n_groups, void* d_scratch,
                            void* d_tallies, void* d_counts, void* d_bad, void* stream = nullptr) const {
    check(eg_choice_tally_grouped_device(p_, n, d_ballots, d_status, d_groups, n_groups, d_scratch, d_tallies, d_counts, d_bad, stream));
  }
  // weighted form: weights[b] < 2^weight_bits times the ciphertexts of ballot b; an empty `groups` puts every ballot into one group
  WeightedTally tally_weighted(const Bytes& packed, const std::vector<uint32_t>& status, const std::vector<uint64_t>& weights, int weight_bits,
                               const std::vector<uint32_t>& groups = {}, uint32_t n_groups = 1) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || status.size() != n || weights.size() != n || (!groups.empty() && groups.size() != n))
      throw Error(EG_ERR_BAD_ARG, "packed, status, weights and groups do not describe the same number of ballots");
    if (n_groups == 0 || n_groups > EG_TALLY_GROUPS_MAX) throw Error(EG_ERR_BAD_ARG, "n_groups out of range");
    Bytes tallies((size_t)n_groups * 64 * n_);
    std::vector<uint64_t> sums(2 * (size_t)n_groups);
    std::vector<uint32_t> counts(n_groups);
    check(eg_choice_tally_weighted(p_, n, packed.data(), status.data(), weights.data(), weight_bits, groups.empty() ? nullptr : groups.data(),
          n_groups, tallies.data(), sums.data(), counts.data()));
    return unpack_weighted(tallies, sums, std::move(counts), n_);
  }
  // asynchronous device-pointer form: d_scratch of tally_weighted_scratch_bytes(n, n_groups) bytes, d_bad three uint32 the library writes
  size_t tally_weighted_scratch_bytes(size_t n, uint32_t n_groups) const { return eg_choice_tally_weighted_scratch_bytes(p_, n, n_groups); }
  void tally_weighted_device(size_t n, const void* d_ballots, const void* d_status, const void* d_weights, int weight_bits, const void* d_groups,
                             uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_weight_sums, void* d_counts, void* d_bad,
                             void* stream = nullptr) const {
    check(eg_choice_tally_weighted_device(p_, n, d_ballots, d_status, d_weights, weight_bits, d_groups, n_groups, d_scratch, d_tallies,
          d_weight_sums, d_counts, d_bad, stream));
  }
  // ballot weeding between verify and tally: `status` = the words a verify entry wrote for `packed` (empty: every ballot participates),
  // `board` = the ciphertexts cast in earlier batches, 64 bytes each.  Stateless.
  Weeded weed(const Bytes& packed, const std::vector<uint32_t>& status = {}, const Bytes& board = Bytes(), bool append = true) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || (!status.empty() && status.size() != n) || board.size() % 64)
      throw Error(EG_ERR_BAD_ARG, "packed, status and board do not describe whole ballots and ciphertexts");
    Weeded w;
    w.dup_of.resize(n);
    w.status.resize(n);
    w.appended.resize(append ? n * n_ * 64 : 0);
    size_t n_appended = 0;
    const int rc = eg_choice_weed(p_, n, packed.data(), status.empty() ? nullptr : status.data(), board.size() / 64, board.data(), w.dup_of.data(),
                   w.status.data(), append ? w.appended.data() : nullptr, &n_appended);
    w.appended.resize(n_appended * 64);
    check(rc);
    return w;
  }
  // asynchronous device-pointer form: d_scratch of weed_scratch_bytes(n, n_prior) bytes, d_found three uint32 the library writes
  size_t weed_scratch_bytes(size_t n, size_t n_prior) const { return eg_choice_weed_scratch_bytes(p_, n, n_prior); }
  void weed_device(size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap, uint64_t hash_seed,
                   void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count, void* d_found, void* stream = nullptr) const {
    check(eg_choice_weed_device(p_, n, d_ballots, d_status, n_prior, d_board, board_cap, hash_seed, d_scratch, d_dup_of, d_status_out, d_board_count,
          d_found, stream));
  }
  // the same pass against a persistent board index (BoardIndex below): byte for byte the same outputs at O(batch) per call; d_scratch of
  // weed_indexed_scratch_bytes(n) bytes, whatever the board's size; with d_board_count the appended ciphertexts are added to the index
  size_t weed_indexed_scratch_bytes(size_t n) const { return eg_choice_weed_indexed_scratch_bytes(p_, n); }
  void weed_indexed_device(size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap, void* d_index,
                           uint64_t index_seed, uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count,
                           void* d_found, void* stream = nullptr) const {
    check(eg_choice_weed_indexed_device(p_, n, d_ballots, d_status, n_prior, d_board, board_cap, d_index, index_seed, hash_seed, d_scratch, d_dup_of,
          d_status_out, d_board_count, d_found, stream));
  }
  // ballot audit: the openings of `packed` re-encrypted and compared; `status` empty = every ballot participates
  Audited open_check(const Bytes& packed, const Opening& opening, const std::vector<uint32_t>& status = {}) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || opening.values.size() != n * n_ || opening.rand.size() != 32 * n * n_ ||
        (!status.empty() && status.size() != n))
      throw Error(EG_ERR_BAD_ARG, "packed, opening and status disagree about the number of ballots");
    Audited a;
    a.status.resize(n);
    uint32_t found[2] = {0, 0};
    check(eg_choice_open_check(p_, n, packed.data(), status.empty() ? nullptr : status.data(), opening.values.data(), opening.rand.data(),
          a.status.data(), found));
    a.participated = found[0];
    a.failed = found[1];
    return a;
  }
  // asynchronous device-pointer form: d_scratch of open_check_scratch_bytes(n) bytes, d_found two uint32 the library writes
  size_t open_check_scratch_bytes(size_t n) const { return eg_choice_open_check_scratch_bytes(p_, n); }
  void open_check_device(size_t n, const void* d_ballots, const void* d_status_in, const void* d_values, const void* d_rand, void* d_status_out,
                         void* d_found, void* d_scratch, void* stream = nullptr) const {
    check(eg_choice_open_check_device(p_, n, d_ballots, d_status_in, d_values, d_rand, d_status_out, d_found, d_scratch, stream));
  }
  // the opener of the synthetic ballots of encrypt_batch (selection empty) or of eg_choice_encrypt_selected_batch: VARIABLE TIME, test and
  // benchmark openings only (see eg_hip.h)
  Opening open_batch(uint64_t base_seed, size_t first, size_t n, int n_selected = 0, uint64_t rng_skip = 0,
                     const std::vector<uint32_t>& selection = {}) const {
    Opening o;
    o.values.resize(n * n_);
    o.rand.resize(32 * n * n_);
    check(eg_choice_open_batch(p_, base_seed, first, n, n_selected, rng_skip, selection.empty() ? nullptr : selection.data(), o.values.data(),
          o.rand.data()));
    return o;
  }
  // EncryptedChoice::new for synthetic voters base_seed + first + i (choice.rs:313-349), packed
  Bytes encrypt_batch(uint64_t base_seed, size_t first, size_t n, int n_selected = 0) const {
    Bytes out(n * ballot_size());
    check(eg_choice_encrypt_batch(p_, base_seed, first, n, n_selected, out.data()));
    return out;
  }
  // EncryptedChoice::single(&params, choice, rng) with the caller's choices (choice.rs:296-311); voter i draws from
  // ChaChaRng::seed_from_u64(base_seed + first + i).  VARIABLE TIME in the choice (see eg_hip.h): test / synthetic data only.
  Bytes encrypt_single_choices(uint64_t base_seed, size_t first, const std::vector<size_t>& choices) const {
    const size_t words = (n_ + 31) / 32;
    std::vector<uint32_t> sel(choices.size() * words, 0u);
    for (size_t i = 0; i < choices.size(); ++i) {
      if (choices[i] >= n_) throw Error(EG_ERR_BAD_ARG, "choice out of range");
      sel[i * words + choices[i] / 32] |= 1u << (choices[i] % 32);
    }
    Bytes out(choices.size() * ballot_size());
    check(eg_choice_encrypt_selected_batch(p_, base_seed, first, choices.size(), 0, sel.data(), out.data()));
    return out;
  }
  eg_choice_params* raw() const { return p_; }
 private:
  ChoiceParams(const Context& ctx, const Element& pk, size_t n, bool single) : n_(n), single_(single) {
    check(eg_choice_params_create(ctx.raw(), pk.data(), (int)n, single, &p_));
  }
  eg_choice_params* p_ = nullptr;
  size_t n_;
  int single_;
};

class QuadraticVotingParams {
 public:
  QuadraticVotingParams(const Context& ctx, const Element& receiver, size_t options, uint64_t credits) : n_(options), credits_(credits) {
    check(eg_qv_params_create(ctx.raw(), receiver.data(), (int)options, credits, &p_));
  }
  ~QuadraticVotingParams() { eg_qv_params_destroy(p_); }
  QuadraticVotingParams(const QuadraticVotingParams&) = delete;
  QuadraticVotingParams& operator=(const QuadraticVotingParams&) = delete;
  size_t options_count() const { return n_; }
  size_t ballot_size() const { return eg_qv_ballot_size(p_); }
  uint64_t credit_amount() const { return credits_; }
  // QuadraticVotingParams::max_votes (quadratic_voting.rs:84-87): isqrt(credit_amount)
  uint64_t max_votes() const { uint64_t r = 0; while ((r + 1) * (r + 1) <= credits_) ++r; return r; }
  BatchVerdict<QuadraticVotingError> verify_batch(const Bytes& packed) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots");
    std::vector<uint32_t> st(n);
    Bytes tally(64 * n_);
    check(eg_verify_qv_batch(p_, n, packed.data(), st.data(), tally.data()));
    BatchVerdict<QuadraticVotingError> v;
    for (uint32_t s : st) v.results.push_back(qv_error_from_status(s));
    v.totals = unpack_totals(tally);
    return v;
  }
  // the same for a handful of ballots (at most EG_SMALL_BATCH_MAX) with low latency: one workgroup per ballot in one launch
  BatchVerdict<QuadraticVotingError> verify_small(const Bytes& packed) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots");
    std::vector<uint32_t> st(n);
    Bytes tally(64 * n_);
    check(eg_verify_qv_small(p_, n, packed.data(), st.data(), tally.data()));
    BatchVerdict<QuadraticVotingError> v;
    for (uint32_t s : st) v.results.push_back(qv_error_from_status(s));
    v.totals = unpack_totals(tally);
    return v;
  }
  void verify_small_device(size_t n, const void* d_ballots, void* d_status, void* stream = nullptr) const {
    check(eg_verify_qv_small_device(p_, n, d_ballots, d_status, stream));
  }
  // per-group tally of a verified batch: `status` = the words a verify entry wrote for `packed` (0 = accepted), groups[b] = group of ballot b
  // (EG_GROUP_NONE: in no group).  Stateless; throws EG_ERR_BAD_ARG for an accepted ballot with an id >= n_groups or an undecodable point.
  GroupedTally tally_grouped(const Bytes& packed, const std::vector<uint32_t>& status, const std::vector<uint32_t>& groups, uint32_t n_groups) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || status.size() != n || groups.size() != n)
      throw Error(EG_ERR_BAD_ARG, "packed, status and groups do not describe the same number of ballots");
    if (n_groups == 0 || n_groups > EG_TALLY_GROUPS_MAX) throw Error(EG_ERR_BAD_ARG, "n_groups out of range");
    Bytes tallies((size_t)n_groups * 64 * n_);
    std::vector<uint32_t> counts(n_groups);
    check(eg_qv_tally_grouped(p_, n, packed.data(), status.data(), groups.data(), n_groups, tallies.data(), counts.data()));
    return unpack_grouped(tallies, std::move(counts), n_);
  }
  // asynchronous device-pointer form: d_scratch of tally_grouped_scratch_bytes(n, n_groups) bytes, d_bad two uint32 the library writes
  size_t tally_grouped_scratch_bytes(size_t n, uint32_t n_groups) const { return eg_qv_tally_grouped_scratch_bytes(p_, n, n_groups); }
  void tally_grouped_device(size_t n, const void* d_ballots, const void* d_status, const void* d_groups, uint32_t n_groups, void* d_scratch,
                            void* d_tallies, void* d_counts, void* d_bad, void* stream = nullptr) const {
    check(eg_qv_tally_grouped_device(p_, n, d_ballots, d_status, d_groups, n_groups, d_scratch, d_tallies, d_counts, d_bad, stream));
  }
  // weighted form: weights[b] < 2^weight_bits times the ciphertexts of ballot b; an empty `groups` puts every ballot into one group
  WeightedTally tally_weighted(const Bytes& packed, const std::vector<uint32_t>& status, const std::vector<uint64_t>& weights, int weight_bits,
                               const std::vector<uint32_t>& groups = {}, uint32_t n_groups = 1) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || status.size() != n || weights.size() != n || (!groups.empty() && groups.size() != n))
      throw Error(EG_ERR_BAD_ARG, "packed, status, weights and groups do not describe the same number of ballots");
    if (n_groups == 0 || n_groups > EG_TALLY_GROUPS_MAX) throw Error(EG_ERR_BAD_ARG, "n_groups out of range");
    Bytes tallies((size_t)n_groups * 64 * n_);
    std::vector<uint64_t> sums(2 * (size_t)n_groups);
    std::vector<uint32_t> counts(n_groups);
    check(eg_qv_tally_weighted(p_, n, packed.data(), status.data(), weights.data(), weight_bits, groups.empty() ? nullptr : groups.data(),
          n_groups, tallies.data(), sums.data(), counts.data()));
    return unpack_weighted(tallies, sums, std::move(counts), n_);
  }
  // asynchronous device-pointer form: d_scratch of tally_weighted_scratch_bytes(n, n_groups) bytes, d_bad three uint32 the library writes
  size_t tally_weighted_scratch_bytes(size_t n, uint32_t n_groups) const { return eg_qv_tally_weighted_scratch_bytes(p_, n, n_groups); }
  void tally_weighted_device(size_t n, const void* d_ballots, const void* d_status, const void* d_weights, int weight_bits, const void* d_groups,
                             uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_weight_sums, void* d_counts, void* d_bad,
                             void* stream = nullptr) const {
    check(eg_qv_tally_weighted_device(p_, n, d_ballots, d_status, d_weights, weight_bits, d_groups, n_groups, d_scratch, d_tallies,
          d_weight_sums, d_counts, d_bad, stream));
  }
  // ballot weeding between verify and tally: `status` = the words a verify entry wrote for `packed` (empty: every ballot participates),
  // `board` = the ciphertexts cast in earlier batches, 64 bytes each.  Stateless.
  Weeded weed(const Bytes& packed, const std::vector<uint32_t>& status = {}, const Bytes& board = Bytes(), bool append = true) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || (!status.empty() && status.size() != n) || board.size() % 64)
      throw Error(EG_ERR_BAD_ARG, "packed, status and board do not describe whole ballots and ciphertexts");
    Weeded w;
    w.dup_of.resize(n);
    w.status.resize(n);
    w.appended.resize(append ? n * n_ * 64 : 0);
    size_t n_appended = 0;
    const int rc = eg_qv_weed(p_, n, packed.data(), status.empty() ? nullptr : status.data(), board.size() / 64, board.data(), w.dup_of.data(),
                   w.status.data(), append ? w.appended.data() : nullptr, &n_appended);
    w.appended.resize(n_appended * 64);
    check(rc);
    return w;
  }
  // asynchronous device-pointer form: d_scratch of weed_scratch_bytes(n, n_prior) bytes, d_found three uint32 the library writes
  size_t weed_scratch_bytes(size_t n, size_t n_prior) const { return eg_qv_weed_scratch_bytes(p_, n, n_prior); }
  void weed_device(size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap, uint64_t hash_seed,
                   void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count, void* d_found, void* stream = nullptr) const {
    check(eg_qv_weed_device(p_, n, d_ballots, d_status, n_prior, d_board, board_cap, hash_seed, d_scratch, d_dup_of, d_status_out, d_board_count,
          d_found, stream));
  }
  // the same pass against a persistent board index (BoardIndex below): byte for byte the same outputs at O(batch) per call; d_scratch of
  // weed_indexed_scratch_bytes(n) bytes, whatever the board's size; with d_board_count the appended ciphertexts are added to the index
  size_t weed_indexed_scratch_bytes(size_t n) const { return eg_qv_weed_indexed_scratch_bytes(p_, n); }
  void weed_indexed_device(size_t n, const void* d_ballots, const void* d_status, size_t n_prior, void* d_board, size_t board_cap, void* d_index,
                           uint64_t index_seed, uint64_t hash_seed, void* d_scratch, void* d_dup_of, void* d_status_out, void* d_board_count,
                           void* d_found, void* stream = nullptr) const {
    check(eg_qv_weed_indexed_device(p_, n, d_ballots, d_status, n_prior, d_board, board_cap, d_index, index_seed, hash_seed, d_scratch, d_dup_of,
          d_status_out, d_board_count, d_found, stream));
  }
  // ballot audit: the openings of `packed` re-encrypted and compared; `status` empty = every ballot participates
  Audited open_check(const Bytes& packed, const Opening& opening, const std::vector<uint32_t>& status = {}) const {
    const size_t n = packed.size() / ballot_size();
    if (n * ballot_size() != packed.size() || opening.values.size() != n * n_ || opening.rand.size() != 32 * n * n_ ||
        (!status.empty() && status.size() != n))
      throw Error(EG_ERR_BAD_ARG, "packed, opening and status disagree about the number of ballots");
    Audited a;
    a.status.resize(n);
    uint32_t found[2] = {0, 0};
    check(eg_qv_open_check(p_, n, packed.data(), status.empty() ? nullptr : status.data(), opening.values.data(), opening.rand.data(),
          a.status.data(), found));
    a.participated = found[0];
    a.failed = found[1];
    return a;
  }
  // asynchronous device-pointer form: d_scratch of open_check_scratch_bytes(n) bytes, d_found two uint32 the library writes
  size_t open_check_scratch_bytes(size_t n) const { return eg_qv_open_check_scratch_bytes(p_, n); }
  void open_check_device(size_t n, const void* d_ballots, const void* d_status_in, const void* d_values, const void* d_rand, void* d_status_out,
                         void* d_found, void* d_scratch, void* stream = nullptr) const {
    check(eg_qv_open_check_device(p_, n, d_ballots, d_status_in, d_values, d_rand, d_status_out, d_found, d_scratch, stream));
  }
  // the opener of the synthetic ballots of eg_qv_encrypt_batch_device (votes empty) or of encrypt_votes_batch: VARIABLE TIME, test and
  // benchmark openings only (see eg_hip.h)
  Opening open_batch(uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip = 0, const std::vector<uint32_t>& votes = {}) const {
    Opening o;
    o.values.resize(n * n_);
    o.rand.resize(32 * n * n_);
    check(eg_qv_open_batch(p_, base_seed, first, n, rng_skip, votes.empty() ? nullptr : votes.data(), o.values.data(), o.rand.data()));
    return o;
  }
  // QuadraticVotingBallot::new(&params, votes, rng) for voters base_seed + first + i (quadratic_voting.rs:234-284); votes:
  // options_count() numbers per voter with sum(v^2) <= credits.  VARIABLE TIME in the votes (see eg_hip.h): test / synthetic data only.
  Bytes encrypt_votes_batch(uint64_t base_seed, size_t first, const std::vector<uint32_t>& votes) const {
    if (votes.size() % n_) throw Error(EG_ERR_BAD_ARG, "votes is not a whole number of ballots");
    const size_t n = votes.size() / n_;
    Bytes out(n * ballot_size());
    check(eg_qv_encrypt_votes_batch(p_, base_seed, first, n, 0, votes.data(), out.data()));
    return out;
  }
  eg_qv_params* raw() const { return p_; }
 private:
  eg_qv_params* p_ = nullptr;
  size_t n_;
  uint64_t credits_ = 0;
};

// CommitmentEquivalenceProof::verify (batched; src/proofs/commitment.rs:186-238) with transcript = Transcript::new(label): the
// ciphertext (R, B) for `receiver` and the Pedersen commitment C = [v]G + [r_c]H over `commitment_blinding_base` hide the same value.
// Packed item (224 bytes): R || B || C || challenge || randomness_response || value_response || commitment_response.
class CommitmentEquivalence {
 public:
  static constexpr size_t ITEM_SIZE = 224;
  // an item the reference could not even deserialise: a non-canonical scalar or an invalid element at 32-byte item `item` of proof `index`
  struct Malformed { size_t index; size_t item; bool scalar; };
  // commitment_blinding_base must decode and must not be the identity (Error with EG_ERR_BAD_ARG; see eg_hip.h)
  CommitmentEquivalence(const Context& ctx, const Element& receiver, const Element& commitment_blinding_base, const std::string& label) {
    check(eg_commit_equiv_params_create(ctx.raw(), receiver.data(), commitment_blinding_base.data(), label.data(), label.size(), &p_));
  }
  ~CommitmentEquivalence() { eg_proof_params_destroy(p_); }
  CommitmentEquivalence(const CommitmentEquivalence&) = delete;
  CommitmentEquivalence& operator=(const CommitmentEquivalence&) = delete;
  // per item: nullopt == Ok(()), else VerificationError::ChallengeMismatch.  Items that do not deserialise never reach verify() in the
  // reference: they are listed in *malformed (and count as ChallengeMismatch in the result); without `malformed` they throw.
  std::vector<std::optional<VerificationError>> verify(const Bytes& packed, std::vector<Malformed>* malformed = nullptr) const {
    const size_t n = packed.size() / ITEM_SIZE;
    if (n * ITEM_SIZE != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of commitment-equivalence items");
    std::vector<uint32_t> st(n);
    check(eg_verify_proof_batch(p_, n, packed.data(), st.data()));
    std::vector<std::optional<VerificationError>> out(n);
    for (size_t i = 0; i < n; ++i) {
      const uint32_t kind = EG_STATUS_KIND(st[i]);
      if (kind == EG_ST_OK) continue;
      out[i] = VerificationError::ChallengeMismatch;
      if (kind != EG_ST_BAD_SCALAR && kind != EG_ST_BAD_POINT) continue;
      if (!malformed) throw Error(EG_ERR_BAD_ARG, "item " + std::to_string(i) + " does not deserialise");
      malformed->push_back({i, EG_STATUS_DETAIL(st[i]), kind == EG_ST_BAD_SCALAR});
    }
    return out;
  }
  // CommitmentEquivalenceProof::new for values[i] from ChaChaRng::seed_from_u64(base_seed + first + i) (commitment.rs:134-181); the
  // blinding scalars r_c go to *blindings when given.  VARIABLE TIME (see eg_hip.h): test / synthetic data only.
  Bytes prove_batch(uint64_t base_seed, size_t first, const std::vector<uint64_t>& values, std::vector<Scalar>* blindings = nullptr) const {
    Bytes out(values.size() * ITEM_SIZE);
    if (blindings) blindings->resize(values.size());
    check(eg_commit_equiv_prove_batch(p_, base_seed, first, values.size(), 0, values.data(), out.data(),
                                      blindings ? reinterpret_cast<uint8_t*>(blindings->data()) : nullptr));
    return out;
  }
  eg_proof_params* raw() const { return p_; }
 private:
  eg_proof_params* p_ = nullptr;
};

// The other single-item proofs (eg_hip.h, "batch tier: single-ciphertext proofs"): one params object per proof kind, verified with
// eg_verify_proof_batch and PRODUCED on the GPU by the provers below.  Every prover is VARIABLE TIME (see eg_hip.h): test / synthetic
// data only.  Item i draws from ChaChaRng::seed_from_u64(base_seed + first + i) after rng_skip 64-byte draws.
class ProofParams {
 public:
  ~ProofParams() { eg_proof_params_destroy(p_); }
  ProofParams(const ProofParams&) = delete;
  ProofParams& operator=(const ProofParams&) = delete;
  size_t item_size() const { return eg_proof_item_size(p_); }
  std::vector<uint32_t> verify_batch(const Bytes& packed) const {       // status words of eg_hip.h, one per item
    const size_t n = packed.size() / item_size();
    if (n * item_size() != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of items");
    std::vector<uint32_t> st(n);
    check(eg_verify_proof_batch(p_, n, packed.data(), st.data()));
    return st;
  }
  eg_proof_params* raw() const { return p_; }
 protected:
  ProofParams() = default;
  // n items from the flat uint64 inputs (eg_proof_prove_input_size / 8 per item; none for the zero proof)
  Bytes prove_values(uint64_t base_seed, size_t first, size_t n, const std::vector<uint64_t>& inputs, uint64_t rng_skip) const {
    if (inputs.size() * 8 != n * eg_proof_prove_input_size(p_)) throw Error(EG_ERR_BAD_ARG, "wrong number of input values");
    Bytes out(n * item_size());
    check(eg_proof_prove_batch(p_, base_seed, first, n, rng_skip, inputs.data(), out.data()));
    return out;
  }
  eg_proof_params* p_ = nullptr;
};
// PublicKey::encrypt_zero / verify_zero (src/keys/impls.rs:31-69): item = ciphertext || challenge || response
class ZeroEncryption : public ProofParams {
 public:
  ZeroEncryption(const Context& ctx, const Element& receiver) { check(eg_proof_params_create(ctx.raw(), receiver.data(), EG_PROOF_ZERO, 0, &p_)); }
  Bytes encrypt_zero(uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip = 0) const { return prove_values(base_seed, first, n, {}, rng_skip); }
};
// PublicKey::encrypt_bool / verify_bool (:77-112): item = ciphertext || e0 || s0 || s1
class BoolEncryption : public ProofParams {
 public:
  BoolEncryption(const Context& ctx, const Element& receiver) { check(eg_proof_params_create(ctx.raw(), receiver.data(), EG_PROOF_BOOL, 0, &p_)); }
  Bytes encrypt_bool(uint64_t base_seed, size_t first, const std::vector<bool>& values, uint64_t rng_skip = 0) const {
    return prove_values(base_seed, first, values.size(), std::vector<uint64_t>(values.begin(), values.end()), rng_skip);
  }
};
// PublicKey::encrypt_range / verify_range (:124-151) with RangeDecomposition::optimal(upper_bound); values below upper_bound
class RangeEncryption : public ProofParams {
 public:
  RangeEncryption(const Context& ctx, const Element& receiver, uint64_t upper_bound) {
    check(eg_proof_params_create(ctx.raw(), receiver.data(), EG_PROOF_RANGE, upper_bound, &p_));
  }
  Bytes encrypt_range(uint64_t base_seed, size_t first, const std::vector<uint64_t>& values, uint64_t rng_skip = 0) const {
    return prove_values(base_seed, first, values.size(), values, rng_skip);
  }
};
// SumOfSquaresProof::new / verify (src/proofs/mul.rs:107-260) with Transcript::new(label) over n_values fresh ciphertexts per item:
// item = value ciphertexts || sum-of-squares ciphertext || challenge || ciphertext responses || sum response
class SumOfSquares : public ProofParams {
 public:
  SumOfSquares(const Context& ctx, const Element& receiver, size_t n_values, const std::string& label) : n_values_(n_values) {
    check(eg_sumsq_params_create(ctx.raw(), receiver.data(), (int)n_values, label.data(), label.size(), &p_));
  }
  // values: n_values per item, back to back; the sum of an item's squares must fit 64 bits
  Bytes prove(uint64_t base_seed, size_t first, const std::vector<uint64_t>& values, uint64_t rng_skip = 0) const {
    return prove_values(base_seed, first, values.size() / n_values_, values, rng_skip);
  }
 private:
  size_t n_values_;
};
// PublicKeySet::verify_share / ActiveParticipant::decrypt_share (src/sharing/key_set.rs:209-228, participant.rs:163-186) for ONE
// participant of a key set: item = ciphertext.random_element || dh_element || challenge || response
class DecryptionShares : public ProofParams {
 public:
  DecryptionShares(const Context& ctx, const Element& shared_key, uint64_t shares, uint64_t threshold, uint64_t index, const Element& participant_key) {
    check(eg_share_params_create(ctx.raw(), shared_key.data(), shares, threshold, index, participant_key.data(), &p_));
  }
  // one item per random element; (*ok)[i] = 0 and a zeroed item where it does not decode (without `ok` that throws).  Variable time in
  // the secret share.
  Bytes decrypt_share(const Scalar& secret_share, uint64_t base_seed, size_t first, const std::vector<Element>& random_elements,
                      std::vector<uint8_t>* ok = nullptr, uint64_t rng_skip = 0) const {
    const size_t n = random_elements.size();
    Bytes out(n * 128);
    std::vector<uint8_t> good(n);
    check(eg_share_prove_batch(p_, secret_share.data(), base_seed, first, n, rng_skip, reinterpret_cast<const uint8_t*>(random_elements.data()),
                               out.data(), good.data()));
    if (ok) *ok = good;
    else for (uint8_t g : good) if (!g) throw Error(EG_ERR_BAD_ARG, "a ciphertext's random element is not a valid ristretto255 encoding");
    return out;
  }
};

// One batch over several GPUs of this process (eg_verify_*_batch_multi): per_device[d] = the election's params created on the context
// of GPU d; contiguous slabs, one host thread per GPU inside the library, the slabs' tallies merged in the library.  What a
// single-process host like examples/voting.rs:179-213 calls when the node has more than one GPU.
inline BatchVerdict<ChoiceVerificationError> verify_batch_multi(const std::vector<const ChoiceParams*>& per_device, const Bytes& packed) {
  if (per_device.empty()) throw Error(EG_ERR_BAD_ARG, "no params objects");
  const size_t bs = per_device[0]->ballot_size(), n = packed.size() / bs;
  if (n * bs != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots for these parameters");
  std::vector<eg_choice_params*> raw;
  for (auto* p : per_device) raw.push_back(p->raw());
  std::vector<uint32_t> st(n);
  Bytes tally(64 * per_device[0]->options_count());
  check(eg_verify_choice_batch_multi(raw.data(), (int)raw.size(), n, packed.data(), st.data(), tally.data()));
  BatchVerdict<ChoiceVerificationError> v;
  for (uint32_t x : st) v.results.push_back(choice_error_from_status(x));
  v.totals = unpack_totals(tally);
  return v;
}
inline BatchVerdict<QuadraticVotingError> verify_batch_multi(const std::vector<const QuadraticVotingParams*>& per_device, const Bytes& packed) {
  if (per_device.empty()) throw Error(EG_ERR_BAD_ARG, "no params objects");
  const size_t bs = per_device[0]->ballot_size(), n = packed.size() / bs;
  if (n * bs != packed.size()) throw Error(EG_ERR_BAD_ARG, "packed length is not a whole number of ballots");
  std::vector<eg_qv_params*> raw;
  for (auto* p : per_device) raw.push_back(p->raw());
  std::vector<uint32_t> st(n);
  Bytes tally(64 * per_device[0]->options_count());
  check(eg_verify_qv_batch_multi(raw.data(), (int)raw.size(), n, packed.data(), st.data(), tally.data()));
  BatchVerdict<QuadraticVotingError> v;
  for (uint32_t x : st) v.results.push_back(qv_error_from_status(x));
  v.totals = unpack_totals(tally);
  return v;
}

// The same with every slab already resident on its GPU (eg_verify_*_batch_multi_device): slab d = counts[d] packed ballots at the device
// pointer d_ballots[d] on the device of per_device[d], verdicts (uint32 words) to d_status[d], streams[d] a hipStream_t of that device
// (empty vector: the null streams).  Returns the tally of this batch; every params object's running tally advances by its slab.  A
// failure in any slab throws and leaves every running tally as it was (eg_hip.h: "AFTER A FAILURE").
inline std::vector<Ciphertext> verify_batch_multi_device(const std::vector<const ChoiceParams*>& per_device, const std::vector<size_t>& counts,
                                                         const std::vector<const void*>& d_ballots, const std::vector<void*>& d_status,
                                                         const std::vector<void*>& streams = {}) {
  const size_t k = per_device.size();
  if (!k || counts.size() != k || d_ballots.size() != k || d_status.size() != k || (!streams.empty() && streams.size() != k))
    throw Error(EG_ERR_BAD_ARG, "one count, ballot pointer, status pointer (and stream) per params object");
  std::vector<eg_choice_params*> raw;
  for (auto* p : per_device) raw.push_back(p->raw());
  Bytes tally(64 * per_device[0]->options_count());
  check(eg_verify_choice_batch_multi_device(raw.data(), (int)k, counts.data(), d_ballots.data(), d_status.data(),
                                            streams.empty() ? nullptr : streams.data(), tally.data()));
  return unpack_totals(tally);
}
inline std::vector<Ciphertext> verify_batch_multi_device(const std::vector<const QuadraticVotingParams*>& per_device, const std::vector<size_t>& counts,
                                                         const std::vector<const void*>& d_ballots, const std::vector<void*>& d_status,
                                                         const std::vector<void*>& streams = {}) {
  const size_t k = per_device.size();
  if (!k || counts.size() != k || d_ballots.size() != k || d_status.size() != k || (!streams.empty() && streams.size() != k))
    throw Error(EG_ERR_BAD_ARG, "one count, ballot pointer, status pointer (and stream) per params object");
  std::vector<eg_qv_params*> raw;
  for (auto* p : per_device) raw.push_back(p->raw());
  Bytes tally(64 * per_device[0]->options_count());
  check(eg_verify_qv_batch_multi_device(raw.data(), (int)k, counts.data(), d_ballots.data(), d_status.data(),
                                        streams.empty() ? nullptr : streams.data(), tally.data()));
  return unpack_totals(tally);
}

// Wire ingest (src/serde.rs:19-80,179-355): ballots as JSON text in the reference's serde layout -> packed ballots, on the host.
// status[k]: EG_ST_OK (packed[k] valid), EG_ST_MALFORMED (does not deserialise) or EG_PACK_RESHAPE (wrong number of choices /
// responses / partial ciphertexts for this election: OptionsLenMismatch / LenMismatch territory).
struct PackedJson {
  Bytes packed;                  // n objects x ballot size; rejected slots are zero
  std::vector<uint32_t> status;
  size_t ballot_size = 0;
  Bytes accepted() const {       // the packed ballots with status OK, back to back (what verify_batch takes)
    Bytes out;
    for (size_t k = 0; k < status.size(); ++k)
      if (status[k] == EG_ST_OK) out.insert(out.end(), packed.begin() + k * ballot_size, packed.begin() + (k + 1) * ballot_size);
    return out;
  }
};
inline PackedJson pack_choice_json(size_t options, bool single, const std::string& text, int threads = 1) {
  PackedJson r;
  r.ballot_size = eg_choice_ballot_size((int)options, single);
  size_t n = 0;
  // first call sizes the output: with max_objects = 0 the library only counts (EG_ERR_BAD_ARG says "more objects than max_objects")
  const int rc = eg_choice_pack_json((int)options, single, text.data(), text.size(), threads, 0, nullptr, nullptr, &n);
  if (rc != EG_OK && n == 0) throw Error(rc, eg_last_error());
  r.packed.resize(n * r.ballot_size);
  r.status.resize(n);
  if (n) check(eg_choice_pack_json((int)options, single, text.data(), text.size(), threads, n, r.packed.data(), r.status.data(), &n));
  return r;
}
inline PackedJson pack_qv_json(size_t options, uint64_t credits, const std::string& text, int threads = 1) {
  PackedJson r;
  r.ballot_size = eg_qv_ballot_size_for((int)options, credits);
  size_t n = 0;
  const int rc = eg_qv_pack_json((int)options, credits, text.data(), text.size(), threads, 0, nullptr, nullptr, &n);
  if (rc != EG_OK && n == 0) throw Error(rc, eg_last_error());
  r.packed.resize(n * r.ballot_size);
  r.status.resize(n);
  if (n) check(eg_qv_pack_json((int)options, credits, text.data(), text.size(), threads, n, r.packed.data(), r.status.data(), &n));
  return r;
}

// The JSON text of a batch of ballots in PIECES (eg_verify_*_json_begin / eg_verify_json_feed / _take / _end): what a host does with
// ballots that arrive one at a time or in network-sized chunks (examples/voting.rs:195-198).  Pieces of any size, a ballot may straddle
// them.  RAII: a stream that is not finished is aborted (the params object's running tally is then what it was before).
class JsonStream {
 public:
  JsonStream(const ChoiceParams& p, int threads = 1) : options_(p.options_count()) { check(eg_verify_choice_json_begin(p.raw(), threads, &s_)); }
  JsonStream(const QuadraticVotingParams& p, int threads = 1) : options_(p.options_count()) { check(eg_verify_qv_json_begin(p.raw(), threads, &s_)); }
  // several params objects of ONE election, one per GPU (eg_verify_*_json_begin_multi): one parser, its packed windows dealt to the GPUs by
  // load, verdicts in text order; every params object tallies the windows it verified, finish() reports the text's tally
  JsonStream(const std::vector<const ChoiceParams*>& per_device, int threads = 1) : options_(per_device.at(0)->options_count()) {
    std::vector<eg_choice_params*> raw;
    for (auto* p : per_device) raw.push_back(p->raw());
    check(eg_verify_choice_json_begin_multi(raw.data(), (int)raw.size(), threads, &s_));
  }
  JsonStream(const std::vector<const QuadraticVotingParams*>& per_device, int threads = 1) : options_(per_device.at(0)->options_count()) {
    std::vector<eg_qv_params*> raw;
    for (auto* p : per_device) raw.push_back(p->raw());
    check(eg_verify_qv_json_begin_multi(raw.data(), (int)raw.size(), threads, &s_));
  }
  JsonStream(const JsonStream&) = delete;
  JsonStream& operator=(const JsonStream&) = delete;
  ~JsonStream() { if (s_) eg_verify_json_abort(s_); }
  // the next piece; returns the number of complete objects seen so far
  size_t feed(const char* text, size_t len) { size_t n = 0; check(eg_verify_json_feed(s_, text, len, &n)); objects_ = n; return n; }
  size_t feed(const std::string& piece) { return feed(piece.data(), piece.size()); }
  // a block handed over WITHOUT a copy (eg_verify_json_feed_owned): the stream keeps the shared buffer alive until the library gives it back
  size_t feed_owned(std::shared_ptr<const std::string> block) {
    auto* keep = new std::shared_ptr<const std::string>(std::move(block));
    size_t n = 0;
    const int rc = eg_verify_json_feed_owned(s_, (*keep)->data(), (*keep)->size(),
                                             [](void* user, const char*, size_t) { delete static_cast<std::shared_ptr<const std::string>*>(user); }, keep, &n);
    if (rc != EG_OK) { delete keep; check(rc); }          // a failed call leaves the block with the caller
    objects_ = n;
    return n;
  }
  // status words that are final so far, in order (never blocks)
  std::vector<uint32_t> take(size_t cap = 1 << 20) {
    std::vector<uint32_t> st(cap);
    size_t n = 0;
    check(eg_verify_json_take(s_, st.data(), cap, &n));
    st.resize(n);
    return st;
  }
  // flushes: the status words not yet taken; totals = the tally of the stream's ballots (the running tally of the params has them added)
  std::vector<uint32_t> finish(std::vector<Ciphertext>* totals = nullptr) {
    std::vector<uint32_t> st(objects_ + 1024);
    Bytes tally(64 * options_);
    size_t n = 0, total = 0;
    for (;;) {
      const int rc = eg_verify_json_end(s_, st.data(), st.size(), &n, &total, tally.data());
      if (rc == EG_OK) break;
      if (rc == EG_ERR_BAD_ARG && n > st.size()) { st.resize(n); continue; }     // more verdicts than feed() had reported yet: the stream is still open
      const std::string why = eg_last_error();
      s_ = nullptr;                // every other error: the library has destroyed the stream
      throw Error(rc, why);
    }
    s_ = nullptr;
    st.resize(n);
    objects_ = total;
    if (totals) *totals = unpack_totals(tally);
    return st;
  }
  size_t objects() const { return objects_; }
 private:
  eg_json_stream* s_ = nullptr;
  size_t options_, objects_ = 0;
};

// Ristretto: the Group backend (ristretto.rs), one problem per call shown here; *_batch in eg_hip.h for many.
// The reference's typed Elements cannot be invalid; here elements are byte strings, so the operations that take
// elements throw Error(EG_ERR_BAD_ARG) when an operand is not a valid ristretto255 encoding instead of silently
// treating it as the identity.
struct Ristretto {
  const Context& ctx;
  static void valid(uint8_t ok) { if (!ok) throw Error(EG_ERR_BAD_ARG, "operand is not a valid ristretto255 encoding"); }
  Scalar scalar_from_random_bytes(const std::array<uint8_t, 64>& wide) const { Scalar s; check(eg_scalar_from_wide_batch(ctx.raw(), 1, wide.data(), s.data())); return s; }
  std::optional<Scalar> deserialize_scalar(const Scalar& b) const { uint8_t ok = 0; check(eg_scalar_is_canonical_batch(ctx.raw(), 1, b.data(), &ok)); return ok ? std::optional<Scalar>(b) : std::nullopt; }
  std::optional<Element> deserialize_element(const Element& b) const { Element o; uint8_t ok = 0; check(eg_point_roundtrip_batch(ctx.raw(), 1, b.data(), o.data(), &ok)); return ok ? std::optional<Element>(o) : std::nullopt; }
  Element mul_generator(const Scalar& k) const { Element o; check(eg_mul_generator_batch(ctx.raw(), 1, k.data(), o.data())); return o; }
  Element vartime_double_mul_generator(const Scalar& k, const Element& p, const Scalar& r) const { Element o; uint8_t ok = 0; check(eg_vartime_double_mul_generator_batch(ctx.raw(), 1, k.data(), p.data(), r.data(), o.data(), &ok)); valid(ok); return o; }
  Element vartime_multi_mul(const std::vector<Scalar>& s, const std::vector<Element>& e) const {
    if (s.size() != e.size()) throw Error(EG_ERR_BAD_ARG, "scalars and elements differ in number");
    Bytes sb, eb; for (auto& x : s) sb.insert(sb.end(), x.begin(), x.end()); for (auto& x : e) eb.insert(eb.end(), x.begin(), x.end());
    Element o; uint8_t ok; check(eg_vartime_multi_mul_batch(ctx.raw(), 1, s.size(), sb.data(), eb.data(), o.data(), &ok)); valid(ok); return o;
  }
  // Element * &Scalar (ElementOps::Element: Mul<&Scalar>, group/mod.rs:136-143): one-term vartime_multi_mul.  VARIABLE TIME.
  Element mul(const Element& p, const Scalar& k) const { return vartime_multi_mul({k}, {p}); }
  // Scalar::from(u64) (ScalarOps::Scalar: From<u64>, group/mod.rs:70-80): the little-endian integer, canonical by construction
  static Scalar scalar_from_u64(uint64_t x) { Scalar s{}; for (int i = 0; i < 8; ++i) s[i] = (uint8_t)(x >> (8 * i)); return s; }
  Element add(const Element& a, const Element& b) const { Element o; uint8_t ok = 0; check(eg_point_add_batch(ctx.raw(), 1, a.data(), b.data(), 0, o.data(), &ok)); valid(ok); return o; }
  Element sub(const Element& a, const Element& b) const { Element o; uint8_t ok = 0; check(eg_point_add_batch(ctx.raw(), 1, a.data(), b.data(), 1, o.data(), &ok)); valid(ok); return o; }
  Element neg(const Element& a) const { return sub(identity(), a); }
  static Element identity() { return Element{}; }   // 32 zero bytes
  bool is_identity(const Element& a) const { uint8_t f = 0, ok = 0; check(eg_point_is_identity_batch(ctx.raw(), 1, a.data(), &f, &ok)); return f != 0; }
  Scalar invert_scalar(const Scalar& a) const { Scalar o; check(eg_scalar_invert_batch(ctx.raw(), 1, a.data(), o.data())); return o; }
  Scalar scalar_muladd(const Scalar& a, const Scalar& b, const Scalar& c) const { Scalar o; check(eg_scalar_muladd_batch(ctx.raw(), 1, a.data(), b.data(), c.data(), o.data())); return o; }
  Scalar scalar_neg(const Scalar& a) const { Scalar o; check(eg_scalar_neg_batch(ctx.raw(), 1, a.data(), o.data())); return o; }
};

// Voter signatures: Ed25519 (RFC 8032, pure EdDSA) of a batch in one pass (eg_hip.h, "voter signatures" has the rule).  Item b signs
// prefix || msgs[b * stride, b * stride + msg_len) under keys[b], or under keys[key_index[b]] out of a roster; status = 0 or
// EG_ST_BAD_SIGNATURE with the failed check (EG_ED25519_*) in EG_STATUS_DETAIL; a non-zero word of status_in is handed on.
// The signer (keypairs, sign) is VARIABLE TIME: a maker of test and benchmark items, not for a voter client.
struct Ed25519 {
  const Context& ctx;
  Bytes keypairs(const Bytes& seeds) const {
    Bytes keys(seeds.size() / 32 * 32);
    check(eg_ed25519_keypair_batch(ctx.raw(), seeds.size() / 32, seeds.data(), keys.data()));
    return keys;
  }
  Bytes sign(const Bytes& seeds, const Bytes& msgs, size_t msg_len, const Bytes& prefix = Bytes(), size_t msg_stride = 0) const {
    const size_t n = seeds.size() / 32;
    Bytes sigs(n * 64);
    check(eg_ed25519_sign_batch(ctx.raw(), n, seeds.data(), msgs.data(), msg_stride ? msg_stride : msg_len, msg_len, prefix.empty() ? nullptr : prefix.data(),
                                prefix.size(), sigs.data()));
    return sigs;
  }
  std::vector<uint32_t> verify(const Bytes& msgs, size_t msg_len, const Bytes& keys, const Bytes& sigs, const Bytes& prefix = Bytes(),
                               const std::vector<uint32_t>& key_index = {}, const std::vector<uint32_t>& status_in = {}, size_t msg_stride = 0) const {
    const size_t n = sigs.size() / 64;
    if ((!key_index.empty() && key_index.size() != n) || (!status_in.empty() && status_in.size() != n)) throw Error(EG_ERR_BAD_ARG, "one key index / status word per item");
    std::vector<uint32_t> status(n);
    check(eg_ed25519_verify_batch(ctx.raw(), n, msgs.data(), msg_stride ? msg_stride : msg_len, msg_len, prefix.empty() ? nullptr : prefix.data(), prefix.size(),
                                  keys.data(), keys.size() / 32, key_index.empty() ? nullptr : key_index.data(), sigs.data(),
                                  status_in.empty() ? nullptr : status_in.data(), status.data()));
    return status;
  }
  // asynchronous device-pointer form: d_scratch of verify_scratch_bytes(n) bytes; `prefix` is host memory; d_status_out may be d_status_in
  size_t verify_scratch_bytes(size_t n) const { return eg_ed25519_verify_scratch_bytes(ctx.raw(), n); }
  void verify_device(size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const Bytes& prefix, const void* d_keys, size_t n_keys,
                     const void* d_key_index, const void* d_sigs, const void* d_status_in, void* d_status_out, void* d_scratch, size_t scratch_bytes,
                     void* stream = nullptr) const {
    check(eg_ed25519_verify_device(ctx.raw(), n, d_msgs, msg_stride, msg_len, prefix.empty() ? nullptr : prefix.data(), prefix.size(), d_keys, n_keys,
                                   d_key_index, d_sigs, d_status_in, d_status_out, d_scratch, scratch_bytes, stream));
  }
  void keypairs_device(size_t n, const void* d_seeds, void* d_keys, void* stream = nullptr) const {
    check(eg_ed25519_keypair_batch_device(ctx.raw(), n, d_seeds, d_keys, stream));
  }
  void sign_device(size_t n, const void* d_seeds, const void* d_msgs, size_t msg_stride, size_t msg_len, const void* d_prefix, size_t prefix_len,
                   void* d_sigs, void* stream = nullptr) const {
    check(eg_ed25519_sign_batch_device(ctx.raw(), n, d_seeds, d_msgs, msg_stride, msg_len, d_prefix, prefix_len, d_sigs, stream));
  }
  // SHA-512(prefix || msg_b) of n messages of one length: 64 bytes each
  Bytes sha512(size_t n, const Bytes& msgs, size_t msg_len, const Bytes& prefix = Bytes(), size_t msg_stride = 0) const {
    Bytes out(n * 64);
    check(eg_sha512_batch(ctx.raw(), n, msgs.data(), msg_stride ? msg_stride : msg_len, msg_len, prefix.empty() ? nullptr : prefix.data(), prefix.size(), out.data()));
    return out;
  }
  void sha512_device(size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const void* d_prefix, size_t prefix_len, void* d_digests,
                     void* stream = nullptr) const {
    check(eg_sha512_batch_device(ctx.raw(), n, d_msgs, msg_stride, msg_len, d_prefix, prefix_len, d_digests, stream));
  }
};

// Voter roll: one counted ballot per voter, by a policy, across batches and GPUs (eg_hip.h, "voter roll" has the rule); between weeding
// and the tally.  The roll is the caller's vector of one 64-bit word per roster key (0 = no counted ballot yet), kept between calls and
// merged with the rolls of other slabs, ranks or GPUs by the element-wise maximum.  status_out / groups_out / weights_out are the arrays
// ChoiceParams::tally_grouped / tally_weighted take (groups and weights only with the roster arrays).
struct RollVerdicts {
  std::vector<uint64_t> superseded_by;                        // EG_SEQ_NONE: kept, not participating, or without a winner
  std::vector<uint32_t> status_out, groups_out;
  std::vector<uint64_t> weights_out;
  std::vector<std::pair<uint64_t, uint64_t>> displaced;       // cast only: (old sequence number, new sequence number)
  uint32_t found[3] = {0, 0, 0};                              // superseded, displaced (check: not cast), off the roll
};
struct VoterRoll {
  const Context& ctx;
  int policy = EG_ROLL_LAST;
  uint64_t word(uint64_t seq) const { return EG_ROLL_WORD(seq, policy); }
  uint64_t seq(uint64_t word) const { return EG_ROLL_SEQ(word, policy); }
  // ballot b has the sequence number seq_base + b and participates iff status_in[b] == 0 (empty: every ballot); `roll` is updated
  RollVerdicts cast(const std::vector<uint32_t>& key_index, std::vector<uint64_t>& roll, uint64_t seq_base = 0, const std::vector<uint32_t>& status_in = {},
                    const std::vector<uint32_t>& roster_groups = {}, const std::vector<uint64_t>& roster_weights = {}) const {
    RollVerdicts v = room(key_index, roll, status_in, roster_groups, roster_weights);
    const size_t n = key_index.size();
    std::vector<uint64_t> pairs(2 * n);
    uint64_t count = 0;
    ok(eg_roll_cast(ctx.raw(), n, key_index.data(), status_in.empty() ? nullptr : status_in.data(), seq_base, policy, roll.data(), roll.size(),
                       roster_groups.empty() ? nullptr : roster_groups.data(), roster_weights.empty() ? nullptr : roster_weights.data(),
                       v.superseded_by.data(), v.status_out.data(), roster_groups.empty() ? nullptr : v.groups_out.data(),
                       roster_weights.empty() ? nullptr : v.weights_out.data(), pairs.data(), &count, v.found));
    for (uint64_t k = 0; k < count; ++k) v.displaced.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
    return v;
  }
  // the same verdicts against a read-only roll: the final one at the close of the election, or a merged one
  RollVerdicts check(const std::vector<uint32_t>& key_index, const std::vector<uint64_t>& roll, uint64_t seq_base = 0,
                     const std::vector<uint32_t>& status_in = {}, const std::vector<uint32_t>& roster_groups = {},
                     const std::vector<uint64_t>& roster_weights = {}) const {
    RollVerdicts v = room(key_index, roll, status_in, roster_groups, roster_weights);
    ok(eg_roll_check(ctx.raw(), key_index.size(), key_index.data(), status_in.empty() ? nullptr : status_in.data(), seq_base, policy,
                                            roll.data(), roll.size(), roster_groups.empty() ? nullptr : roster_groups.data(),
                                            roster_weights.empty() ? nullptr : roster_weights.data(), v.superseded_by.data(), v.status_out.data(),
                                            roster_groups.empty() ? nullptr : v.groups_out.data(), roster_weights.empty() ? nullptr : v.weights_out.data(),
                                            v.found));
    return v;
  }
  // asynchronous device-pointer forms: no allocation, no synchronisation, no lock; d_scratch of cast_scratch_bytes(n, n_keys) bytes;
  // d_status_out may be d_status_in; d_displaced (n x 2 x uint64) comes with d_displaced_count (uint64), or both are null
  size_t cast_scratch_bytes(size_t n, size_t n_keys) const { return eg_roll_cast_scratch_bytes(ctx.raw(), n, n_keys); }
  void cast_device(size_t n, const void* d_key_index, const void* d_status_in, uint64_t seq_base, void* d_roll, size_t n_keys,
                   const void* d_roster_groups, const void* d_roster_weights, void* d_superseded_by, void* d_status_out, void* d_groups_out,
                   void* d_weights_out, void* d_displaced, void* d_displaced_count, void* d_found, void* d_scratch, size_t scratch_bytes,
                   void* stream = nullptr) const {
    ok(eg_roll_cast_device(ctx.raw(), n, d_key_index, d_status_in, seq_base, policy, d_roll, n_keys, d_roster_groups,
                                                  d_roster_weights, d_superseded_by, d_status_out, d_groups_out, d_weights_out, d_displaced,
                                                  d_displaced_count, d_found, d_scratch, scratch_bytes, stream));
  }
  void check_device(size_t n, const void* d_key_index, const void* d_status_in, uint64_t seq_base, const void* d_roll, size_t n_keys,
                    const void* d_roster_groups, const void* d_roster_weights, void* d_superseded_by, void* d_status_out, void* d_groups_out,
                    void* d_weights_out, void* d_found, void* stream = nullptr) const {
    ok(eg_roll_check_device(ctx.raw(), n, d_key_index, d_status_in, seq_base, policy, d_roll, n_keys, d_roster_groups,
                                                   d_roster_weights, d_superseded_by, d_status_out, d_groups_out, d_weights_out, d_found, stream));
  }

 private:
  // the member `check` hides the free function of the namespace
  static void ok(int rc) { if (rc != EG_OK) throw Error(rc, eg_last_error()); }
  static RollVerdicts room(const std::vector<uint32_t>& key_index, const std::vector<uint64_t>& roll, const std::vector<uint32_t>& status_in,
                           const std::vector<uint32_t>& roster_groups, const std::vector<uint64_t>& roster_weights) {
    const size_t n = key_index.size();
    if ((!status_in.empty() && status_in.size() != n) || (!roster_groups.empty() && roster_groups.size() != roll.size()) ||
        (!roster_weights.empty() && roster_weights.size() != roll.size()))
      throw Error(EG_ERR_BAD_ARG, "one status word per ballot, one group and one weight per roster key");
    RollVerdicts v;
    v.superseded_by.resize(n); v.status_out.resize(n);
    if (!roster_groups.empty()) v.groups_out.resize(n);
    if (!roster_weights.empty()) v.weights_out.resize(n);
    return v;
  }
};

// Board index: the open-addressing table over the weeding board's ciphertexts, kept by the caller in device memory between batches
// (eg_hip.h, "persistent board index" has the contract).  The struct holds what must stay the same for the life of an index - the board's
// room and the seed, which stays unpublished - and the caller holds the device memory: bytes() of it.
struct BoardIndex {
  const Context& ctx;
  size_t board_cap = 0;
  uint64_t index_seed = 0;
  size_t bytes() const { return eg_weed_index_bytes(board_cap); }
  // clears the index and inserts board entries [0, n_prior); d_found: one uint32 the library writes, non-zero after an overflow
  void build_device(size_t n_prior, const void* d_board, void* d_index, void* d_found, void* stream = nullptr) const {
    ok(eg_weed_index_build_device(ctx.raw(), n_prior, d_board, board_cap, index_seed, d_index, d_found, stream));
  }
  // d_pos[q] (uint32) = the smallest board position that holds the 64 bytes of key q, or EG_DUP_NONE; the index is only read
  void find_device(size_t n_q, const void* d_keys, size_t n_prior, const void* d_board, const void* d_index, void* d_pos,
                   void* stream = nullptr) const {
    ok(eg_weed_index_find_device(ctx.raw(), n_q, d_keys, n_prior, d_board, board_cap, d_index, index_seed, d_pos, stream));
  }

 private:
  static void ok(int rc) { if (rc != EG_OK) throw Error(rc, eg_last_error()); }
};

// Receipt log: a Merkle tree (RFC 6962, H = the first 32 bytes of SHA-512) over the posted ballots (eg_hip.h, "receipt log" has the rule);
// fed weeding's status_out.  The log is the caller's vector of 32-byte leaves; every tree() is a full rebuild, there is no frontier state;
// grow() builds the tree of the grown log out of the last one and hashes only what the append changed.
struct LeafPass {
  std::vector<uint64_t> leaf_index;                           // EG_LEAF_NONE: the ballot does not participate
  Bytes leaves;                                               // n x 32, zeroed rows for ballots that do not participate
  uint32_t found[2] = {0, 0};                                 // the number of leaves, non-zero: the append did not fit
};
struct MerkleTree {
  Bytes root;                                                 // 32 bytes
  Bytes nodes;                                                // levels 1 .. depth back to back (ReceiptLog::level)
};
struct Receipts {
  Bytes paths;                                                // m x depth(N) x 32
  std::vector<uint32_t> path_len;                             // EG_MERKLE_NO_PATH: no such leaf
};
struct ReceiptVerdicts {
  std::vector<uint32_t> verdict;                              // 0 or EG_MERKLE_BAD_INDEX / _BAD_LENGTH / _MISMATCH
  uint32_t found[3] = {0, 0, 0};
};
struct PastHeads {
  Bytes heads;                                                // m x 32; H("") for size 0, a zeroed row for a size above N
  uint32_t found[1] = {0};                                    // the number of sizes above N
};
struct ConsistencyProofs {
  Bytes proofs;                                               // m x (depth(N) + 1) x 32
  std::vector<uint32_t> proof_len;                            // EG_MERKLE_NO_PATH: old size 0 or above N
};
struct ConsistencyVerdicts {
  std::vector<uint32_t> verdict;                              // 0 or EG_MERKLE_BAD_INDEX / _BAD_LENGTH / _MISMATCH_OLD / _MISMATCH
  uint32_t found[4] = {0, 0, 0, 0};                           // BAD_INDEX, BAD_LENGTH, MISMATCH, MISMATCH_OLD
};
struct ReceiptLog {
  const Context& ctx;
  Bytes prefix = {};                                          // the election id, 0 .. 255 bytes
  static int depth(uint64_t n_leaves) { return eg_merkle_depth(n_leaves); }
  static size_t nodes_bytes(uint64_t n_leaves) { return eg_merkle_nodes_bytes(n_leaves); }
  // (byte offset into the node store, node count) of a level; level 0 is the log itself
  static std::pair<uint64_t, uint64_t> level(uint64_t n_leaves, int lvl) {
    uint64_t off = 0, count = 0;
    ok(eg_merkle_level(n_leaves, lvl, &off, &count));
    return {off, count};
  }
  // the leaves of n ballots of msg_len bytes (extra: n x extra_len bytes or empty, e.g. the signatures); with `log` the participating
  // leaves are appended to it (it grows) and leaf_index counts from its old size
  LeafPass leaves(const Bytes& msgs, size_t msg_len, size_t n, const Bytes& extra = {}, const std::vector<uint32_t>& status_in = {},
                  Bytes* log = nullptr, uint64_t n_prior = 0) const {
    const size_t extra_len = n && !extra.empty() ? extra.size() / n : 0;
    if (msgs.size() != n * msg_len || extra.size() != n * extra_len || (!status_in.empty() && status_in.size() != n))
      throw Error(EG_ERR_BAD_ARG, "n messages of msg_len bytes, n extras of one length, one status word per ballot");
    LeafPass v;
    v.leaf_index.resize(n); v.leaves.resize(n * EG_MERKLE_HASH_BYTES);
    uint64_t count = 0;
    if (log) { n_prior = log->size() / EG_MERKLE_HASH_BYTES; log->resize((n_prior + n) * EG_MERKLE_HASH_BYTES); }
    ok(eg_merkle_leaves(ctx.raw(), n, msgs.data(), msg_len, msg_len, prefix.empty() ? nullptr : prefix.data(), prefix.size(),
                        extra_len ? extra.data() : nullptr, extra_len, extra_len, status_in.empty() ? nullptr : status_in.data(), n_prior,
                        v.leaf_index.data(), v.leaves.data(), log ? log->data() : nullptr, n_prior + n, log ? &count : nullptr, v.found));
    if (log) log->resize(count * EG_MERKLE_HASH_BYTES);
    return v;
  }
  MerkleTree tree(const Bytes& log, bool with_nodes = true) const {
    const uint64_t n = log.size() / EG_MERKLE_HASH_BYTES;
    MerkleTree t;
    t.root.resize(EG_MERKLE_HASH_BYTES);
    if (with_nodes) t.nodes.resize(nodes_bytes(n) ? nodes_bytes(n) : 1);
    ok(eg_merkle_tree(ctx.raw(), n, log.data(), t.root.data(), with_nodes ? t.nodes.data() : nullptr));
    if (with_nodes) t.nodes.resize(nodes_bytes(n));
    return t;
  }
  Receipts paths(const std::vector<uint64_t>& index, const Bytes& log, const Bytes& nodes) const {
    const uint64_t n = log.size() / EG_MERKLE_HASH_BYTES;
    Receipts r;
    r.paths.resize(index.size() * (size_t)depth(n) * EG_MERKLE_HASH_BYTES); r.path_len.resize(index.size());
    ok(eg_merkle_paths(ctx.raw(), index.size(), index.data(), n, log.data(), nodes.data(), r.paths.data(), r.path_len.data()));
    return r;
  }
  // m receipts (index, leaf, path_len, path at paths + j * path_stride) against (n_leaves, root)
  ReceiptVerdicts check(const std::vector<uint64_t>& index, const Bytes& leaves, const Bytes& paths, size_t path_stride,
                        const std::vector<uint32_t>& path_len, uint64_t n_leaves, const Bytes& root) const {
    const size_t m = index.size();
    if (leaves.size() != m * EG_MERKLE_HASH_BYTES || path_len.size() != m || paths.size() < m * path_stride || root.size() != EG_MERKLE_HASH_BYTES)
      throw Error(EG_ERR_BAD_ARG, "one leaf, one path and one path_len per receipt, a root of 32 bytes");
    ReceiptVerdicts v;
    v.verdict.resize(m);
    ok(eg_merkle_check(ctx.raw(), m, index.data(), leaves.data(), paths.data(), path_stride, path_len.data(), n_leaves, root.data(),
                       v.verdict.data(), v.found));
    return v;
  }
  // asynchronous device-pointer forms: no allocation, no synchronisation, no lock
  static size_t leaves_scratch_bytes(size_t n) { return eg_merkle_leaves_scratch_bytes(n); }
  static size_t tree_scratch_bytes(uint64_t n_leaves) { return eg_merkle_tree_scratch_bytes(n_leaves); }
  void leaves_device(size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const void* d_extra, size_t extra_stride, size_t extra_len,
                     const void* d_status_in, uint64_t n_prior, void* d_leaf_index, void* d_leaves_out, void* d_log, uint64_t log_cap,
                     void* d_log_count, void* d_found, void* d_scratch, size_t scratch_bytes, void* stream = nullptr) const {
    ok(eg_merkle_leaves_device(ctx.raw(), n, d_msgs, msg_stride, msg_len, prefix.empty() ? nullptr : prefix.data(), prefix.size(), d_extra,
                               extra_stride, extra_len, d_status_in, n_prior, d_leaf_index, d_leaves_out, d_log, log_cap, d_log_count, d_found,
                               d_scratch, scratch_bytes, stream));
  }
  void tree_device(uint64_t n_leaves, const void* d_log, void* d_root, void* d_nodes, void* d_scratch = nullptr, size_t scratch_bytes = 0,
                   void* stream = nullptr) const {
    ok(eg_merkle_tree_device(ctx.raw(), n_leaves, d_log, d_root, d_nodes, d_scratch, scratch_bytes, stream));
  }
  void paths_device(size_t m, const void* d_index, uint64_t n_leaves, const void* d_log, const void* d_nodes, void* d_paths, void* d_path_len,
                    void* stream = nullptr) const {
    ok(eg_merkle_paths_device(ctx.raw(), m, d_index, n_leaves, d_log, d_nodes, d_paths, d_path_len, stream));
  }
  void check_device(size_t m, const void* d_index, const void* d_leaves, const void* d_paths, size_t path_stride, const void* d_path_len,
                    uint64_t n_leaves, const void* d_root, void* d_verdict, void* d_found, void* stream = nullptr) const {
    ok(eg_merkle_check_device(ctx.raw(), m, d_index, d_leaves, d_paths, path_stride, d_path_len, n_leaves, d_root, d_verdict, d_found, stream));
  }
  // past heads and consistency proofs (eg_hip.h, "PAST HEADS and CONSISTENCY PROOFS"), out of the log and its node store
  static uint32_t consistency_len(uint64_t old_size, uint64_t n_leaves) { return eg_merkle_consistency_len(old_size, n_leaves); }
  PastHeads heads(const std::vector<uint64_t>& size, const Bytes& log, const Bytes& nodes) const {
    PastHeads h;
    h.heads.resize(size.size() * EG_MERKLE_HASH_BYTES);
    ok(eg_merkle_heads(ctx.raw(), size.size(), size.data(), log.size() / EG_MERKLE_HASH_BYTES, log.data(), nodes.data(), h.heads.data(), h.found));
    return h;
  }
  ConsistencyProofs consistency(const std::vector<uint64_t>& old_size, const Bytes& log, const Bytes& nodes) const {
    const uint64_t n = log.size() / EG_MERKLE_HASH_BYTES;
    ConsistencyProofs p;
    p.proofs.resize(old_size.size() * ((size_t)depth(n) + 1) * EG_MERKLE_HASH_BYTES); p.proof_len.resize(old_size.size());
    ok(eg_merkle_consistency(ctx.raw(), old_size.size(), old_size.data(), n, log.data(), nodes.data(), p.proofs.data(), p.proof_len.data()));
    return p;
  }
  // m proofs (old_size, old_root, proof_len, proof at proofs + j * proof_stride) against (n_leaves, root)
  ConsistencyVerdicts consistency_check(const std::vector<uint64_t>& old_size, const Bytes& old_root, const Bytes& proofs, size_t proof_stride,
                                        const std::vector<uint32_t>& proof_len, uint64_t n_leaves, const Bytes& root) const {
    const size_t m = old_size.size();
    if (old_root.size() != m * EG_MERKLE_HASH_BYTES || proof_len.size() != m || proofs.size() < m * proof_stride || root.size() != EG_MERKLE_HASH_BYTES)
      throw Error(EG_ERR_BAD_ARG, "one old root, one proof and one proof_len per old size, a root of 32 bytes");
    ConsistencyVerdicts v;
    v.verdict.resize(m);
    ok(eg_merkle_consistency_check(ctx.raw(), m, old_size.data(), old_root.data(), proofs.data(), proof_stride, proof_len.data(), n_leaves,
                                   root.data(), v.verdict.data(), v.found));
    return v;
  }
  void heads_device(size_t m, const void* d_size, uint64_t n_leaves, const void* d_log, const void* d_nodes, void* d_heads, void* d_found,
                    void* stream = nullptr) const {
    ok(eg_merkle_heads_device(ctx.raw(), m, d_size, n_leaves, d_log, d_nodes, d_heads, d_found, stream));
  }
  void consistency_device(size_t m, const void* d_old_size, uint64_t n_leaves, const void* d_log, const void* d_nodes, void* d_proofs,
                          void* d_proof_len, void* stream = nullptr) const {
    ok(eg_merkle_consistency_device(ctx.raw(), m, d_old_size, n_leaves, d_log, d_nodes, d_proofs, d_proof_len, stream));
  }
  void consistency_check_device(size_t m, const void* d_old_size, const void* d_old_root, const void* d_proofs, size_t proof_stride,
                                const void* d_proof_len, uint64_t n_leaves, const void* d_root, void* d_verdict, void* d_found,
                                void* stream = nullptr) const {
    ok(eg_merkle_consistency_check_device(ctx.raw(), m, d_old_size, d_old_root, d_proofs, proof_stride, d_proof_len, n_leaves, d_root, d_verdict,
                                          d_found, stream));
  }
  // the tree of `log` out of `old`, the tree of its first old_size leaves (eg_hip.h, "GROW"): byte for byte what tree(log) returns, and
  // only the tiles that the append changed are hashed again; `old` is left as it is
  MerkleTree grow(uint64_t old_size, const MerkleTree& old, const Bytes& log) const {
    const uint64_t n = log.size() / EG_MERKLE_HASH_BYTES;
    if (old.nodes.size() < nodes_bytes(old_size)) throw Error(EG_ERR_BAD_ARG, "the old node store is smaller than a store of old_size leaves");
    MerkleTree t;
    t.root.resize(EG_MERKLE_HASH_BYTES);
    t.nodes.resize(nodes_bytes(n) ? nodes_bytes(n) : 1);
    ok(eg_merkle_grow(ctx.raw(), old_size, old_size > 1 ? old.nodes.data() : nullptr, n, log.data(), t.nodes.data(), t.root.data()));
    t.nodes.resize(nodes_bytes(n));
    return t;
  }
  void grow_device(uint64_t old_size, const void* d_nodes_old, uint64_t n_leaves, const void* d_log, void* d_nodes, void* d_root,
                   void* stream = nullptr) const {
    ok(eg_merkle_grow_device(ctx.raw(), old_size, d_nodes_old, n_leaves, d_log, d_nodes, d_root, stream));
  }

 private:
  static void ok(int rc) { if (rc != EG_OK) throw Error(rc, eg_last_error()); }
};

// ---- re-encryption shuffles (eg_hip.h, "re-encryption shuffles" has the rule) -------------------------------------------------------
// Checks a mixer's proof.  The commitment key H_0 .. H_cap is derived once from a seed and serves every shuffle of at most cap rows.
struct ShuffleVerdict {
  uint32_t mask = 0;               // EG_SHUFFLE_* bits, 0 = accepted
  std::vector<uint32_t> rows;      // EG_SHUFFLE_ROW_* bits per row
  uint32_t found[4] = {0, 0, 0xffffffffu, 0xffffffffu};
  bool accepted() const { return mask == 0; }
};
struct ShuffleVerifier {
  const Context& ctx;
  Element K;
  Bytes key;
  uint64_t cap;
  ShuffleVerifier(const Context& c, const Element& election_key, const Bytes& seed, uint64_t cap_) : ctx(c), K(election_key), cap(cap_) {
    key.resize(eg_shuffle_key_bytes(cap) ? eg_shuffle_key_bytes(cap) : 1);
    ok(eg_shuffle_key_derive(ctx.raw(), seed.empty() ? nullptr : seed.data(), seed.size(), cap, key.data()));
  }
  static size_t key_bytes(uint64_t cap) { return eg_shuffle_key_bytes(cap); }
  static size_t proof_bytes(uint64_t n) { return eg_shuffle_proof_bytes(n); }
  size_t verify_scratch_bytes(uint64_t n) const { return eg_shuffle_verify_scratch_bytes(ctx.raw(), n); }
  // in, out: n rows of 64 bytes (R || B); proof: proof_bytes(n) bytes
  ShuffleVerdict verify(const Bytes& in, const Bytes& out, const Bytes& proof, const Bytes& prefix = {}) const {
    const uint64_t n = in.size() / 64;
    if (out.size() != in.size() || proof.size() != proof_bytes(n)) throw Error(EG_ERR_BAD_ARG, "shuffle: out or proof has the wrong size for these rows");
    ShuffleVerdict v;
    v.rows.resize(n ? n : 1);
    ok(eg_shuffle_verify(ctx.raw(), n, in.data(), out.data(), K.data(), prefix.empty() ? nullptr : prefix.data(), prefix.size(), key.data(), cap,
                         proof.data(), &v.mask, v.rows.data(), v.found));
    v.rows.resize(n);
    return v;
  }
  void verify_device(uint64_t n, const void* d_in, const void* d_out, const Bytes& prefix, const void* d_key, uint64_t key_cap, const void* d_proof,
                     void* d_verdict, void* d_rows, void* d_found, void* d_scratch, size_t scratch_bytes, void* stream = nullptr) const {
    ok(eg_shuffle_verify_device(ctx.raw(), n, d_in, d_out, K.data(), prefix.empty() ? nullptr : prefix.data(), prefix.size(), d_key, key_cap, d_proof,
                                d_verdict, d_rows, d_found, d_scratch, scratch_bytes, stream));
  }
  void derive_key_device(const Bytes& seed, uint64_t cap_, void* d_key, void* d_exhausted, void* stream = nullptr) const {
    ok(eg_shuffle_key_derive_device(ctx.raw(), seed.empty() ? nullptr : seed.data(), seed.size(), cap_, d_key, d_exhausted, stream));
  }

 private:
  static void ok(int rc) { if (rc != EG_OK) throw Error(rc, eg_last_error()); }
};

// ---- tally stage (examples/voting.rs:122-177) ------------------------------------------------------------------------------------
// Params::combine_shares (sharing/mod.rs:302-325): the first `threshold` of the given (participant index, dh element) pairs ->
// the combined decryption [x]R, or nullopt when there are too few shares.  Verify the shares first (eg_share_params_create).
inline std::optional<Element> combine_shares(const Context& ctx, uint64_t shares, uint64_t threshold,
                                             const std::vector<std::pair<uint64_t, Element>>& given) {
  std::vector<uint64_t> idx; Bytes dh;
  for (auto& g : given) { idx.push_back(g.first); dh.insert(dh.end(), g.second.begin(), g.second.end()); }
  Element out; int combined = 0;
  check(eg_combine_shares(ctx.raw(), shares, threshold, idx.size(), idx.data(), dh.data(), out.data(), &combined));
  return combined ? std::optional<Element>(out) : std::nullopt;
}
// The same for a whole vector of ciphertexts in one pass (eg_combine_shares_batch): column j holds participant indexes[j]'s m items
// (128 bytes each: R || dh || challenge || response) and, in `status`, the verdicts of its DecryptionShares::verify_batch (empty: every
// share accepted).  Per ciphertext the first `threshold` usable columns are combined: dh = [x]R, plain = B - [x]R (what the discrete-log
// solver takes), combined = 0 where there were too few (zero bytes then), used = bit i for every participant i whose share was used.
struct CombinedShares {
  std::vector<Element> dh, plain;
  std::vector<uint8_t> combined;
  std::vector<uint64_t> used;
};
inline CombinedShares combine_shares_batch(const Context& ctx, uint64_t shares, uint64_t threshold, const Bytes& ciphertexts,
                                           const std::vector<uint64_t>& indexes, const Bytes& items, const std::vector<uint32_t>& status = {}) {
  const size_t m = ciphertexts.size() / 64, k = indexes.size();
  if (m * 64 != ciphertexts.size() || items.size() != k * m * 128 || (!status.empty() && status.size() != k * m))
    throw Error(EG_ERR_BAD_ARG, "ciphertexts, indexes, items and status do not describe the same columns");
  CombinedShares r;
  r.dh.resize(m); r.plain.resize(m); r.combined.resize(m); r.used.resize(m);
  check(eg_combine_shares_batch(ctx.raw(), shares, threshold, m, ciphertexts.data(), (int)k, indexes.data(), items.data(),
        status.empty() ? nullptr : status.data(), reinterpret_cast<uint8_t*>(r.dh.data()), reinterpret_cast<uint8_t*>(r.plain.data()),
        r.combined.data(), r.used.data()));
  return r;
}
// asynchronous device-pointer form: d_scratch of combine_shares_batch_scratch_bytes(threshold, m) bytes, d_bad three uint32 the library writes
inline size_t combine_shares_batch_scratch_bytes(uint64_t threshold, size_t m) { return eg_combine_shares_batch_scratch_bytes(threshold, m); }
inline void combine_shares_batch_device(const Context& ctx, uint64_t shares, uint64_t threshold, size_t m, const void* d_ciphertexts,
                                        const std::vector<uint64_t>& indexes, const void* d_items, const void* d_status, void* d_dh,
                                        void* d_plain, void* d_combined, void* d_used, void* d_bad, void* d_scratch, void* stream = nullptr) {
  check(eg_combine_shares_batch_device(ctx.raw(), shares, threshold, m, d_ciphertexts, (int)indexes.size(), indexes.data(), d_items, d_status,
        d_dh, d_plain, d_combined, d_used, d_bad, d_scratch, stream));
}
// DiscreteLogTable (encryption.rs:260-298)
class DiscreteLogTable {
 public:
  DiscreteLogTable(const Context& ctx, const std::vector<uint64_t>& values) { check(eg_dlog_table_create(ctx.raw(), values.size(), values.data(), &t_)); }
  ~DiscreteLogTable() { eg_dlog_table_destroy(t_); }
  DiscreteLogTable(const DiscreteLogTable&) = delete;
  DiscreteLogTable& operator=(const DiscreteLogTable&) = delete;
  std::optional<uint64_t> get(const Element& decrypted_element) const {
    uint64_t v = 0; uint8_t found = 0;
    check(eg_dlog_table_get(t_, 1, decrypted_element.data(), &v, &found));
    return found ? std::optional<uint64_t>(v) : std::nullopt;
  }
 private:
  eg_dlog_table* t_ = nullptr;
};
// DiscreteLogTable::new(lo..hi) for ranges no table can hold: baby-step/giant-step on the GPU (eg_dlog_solver_*).  One solver serves
// any range; solve() answers every option of a tally in one call.
class DiscreteLogSolver {
 public:
  explicit DiscreteLogSolver(const Context& ctx, int baby_bits = 0) { check(eg_dlog_solver_create(ctx.raw(), baby_bits, &s_)); }
  ~DiscreteLogSolver() { eg_dlog_solver_destroy(s_); }
  DiscreteLogSolver(const DiscreteLogSolver&) = delete;
  DiscreteLogSolver& operator=(const DiscreteLogSolver&) = delete;
  std::vector<std::optional<uint64_t>> solve(const std::vector<Element>& decrypted_elements, uint64_t lo, uint64_t hi) const {
    Bytes in;
    for (auto& e : decrypted_elements) in.insert(in.end(), e.begin(), e.end());
    std::vector<uint64_t> v(decrypted_elements.size());
    std::vector<uint8_t> found(decrypted_elements.size());
    check(eg_dlog_solver_solve(s_, v.size(), in.data(), lo, hi, v.data(), found.data()));
    std::vector<std::optional<uint64_t>> out;
    for (size_t i = 0; i < v.size(); ++i) out.push_back(found[i] ? std::optional<uint64_t>(v[i]) : std::nullopt);
    return out;
  }
  uint64_t max_span(size_t n) const { return eg_dlog_solver_max_span(s_, n); }
  size_t table_bytes() const { return eg_dlog_solver_table_bytes(s_); }
 private:
  eg_dlog_solver* s_ = nullptr;
};

// The tally stage for a whole vector of ciphertexts (per-precinct tallies): every participant's DecryptionShares verifier checks its
// column, one combine_shares_batch over the verdicts, one DiscreteLogSolver::solve over [lo, hi) for all decrypted elements.
// verifiers[j] = (participant index, its verifier), in the order in which shares are preferred; items[j] = its m packed items.
// values[c] = nullopt where fewer than `threshold` shares verified or the plaintext is outside the range.
struct DecryptedTallies {
  std::vector<std::optional<uint64_t>> values;
  std::vector<uint8_t> combined;
  std::vector<uint64_t> used;
};
inline DecryptedTallies decrypt_tallies(const Context& ctx, uint64_t shares, uint64_t threshold, const Bytes& ciphertexts,
                                        const std::vector<std::pair<uint64_t, const ProofParams*>>& verifiers, const std::vector<Bytes>& items,
                                        const DiscreteLogSolver& solver, uint64_t lo, uint64_t hi) {
  if (verifiers.size() != items.size()) throw Error(EG_ERR_BAD_ARG, "one column of items per verifier");
  std::vector<uint64_t> indexes;
  std::vector<uint32_t> status;
  Bytes all;
  for (size_t j = 0; j < verifiers.size(); ++j) {
    const std::vector<uint32_t> st = verifiers[j].second->verify_batch(items[j]);
    indexes.push_back(verifiers[j].first);
    status.insert(status.end(), st.begin(), st.end());
    all.insert(all.end(), items[j].begin(), items[j].end());
  }
  CombinedShares cs = combine_shares_batch(ctx, shares, threshold, ciphertexts, indexes, all, status);
  DecryptedTallies r;
  r.values = solver.solve(cs.plain, lo, hi);
  for (size_t c = 0; c < r.values.size(); ++c) if (!cs.combined[c]) r.values[c] = std::nullopt;
  r.combined = std::move(cs.combined);
  r.used = std::move(cs.used);
  return r;
}

}  // namespace elastic_elgamal_hip
