// voting.cpp -- the reference's examples/voting.rs on the GPU backend, in C++ on top of the C ABI:
//   `Args::vote`            (examples/voting.rs:179-213)  ./voting [votes] [options] [seed]
//   `Args::quadratic_vote`  (examples/voting.rs:219-269)  ./voting --qv [votes] [options] [credits] [seed]
//   options: --devices N, --json, --precincts P, --weighted, --replays K, --signed K, --revotes K, --receipts K, --heads K, --grow, --audits K,
//            --board-index
// talliers' key -> voters create ballots from their own choices -> verify every ballot -> homomorphic totals -> decrypt and
// compare with the EXPECTED totals the voters' choices add up to.  Threshold sharing of the key (examples/voting.rs:105-120) is out
// of scope; a single key pair stands in for the shared key (tests/test_gpu_parity.py::test_threshold_tally_end_to_end
// runs the 7-of-10 tally stage).  With --devices N the batch goes through the in-process multi-GPU entry
// (eg_verify_*_batch_multi) over N contexts on the visible GPUs (all on GPU 0 when fewer are visible).  With --json the ballots travel
// the way examples/voting.rs:195-198 prints them - serde_json text, ONE BALLOT AT A TIME - into the streaming entry
// (JsonStream = eg_verify_choice_json_begin / eg_verify_json_feed / _end), which cuts, packs and verifies them as they arrive.
// With --precincts P voter v belongs to precinct v mod P: after the overall totals, the per-precinct totals of the same verified batch
// (tally_grouped = eg_*_tally_grouped, one pass over the accepted ballots) are decrypted the same way and must add up to the overall result.
// With --weighted voter v also holds a weight (shares, stake): 1 + 7919 v mod 65535.  The weighted totals of the same verified batch
// (tally_weighted = eg_*_tally_weighted: total += ciphertext * weight, the reference's impl Mul<u64> for Ciphertext) are decrypted and read
// with the discrete-log solver over [0, sum of the counted weights x most votes per option] - the table above would not reach that far.
// With --replays K, K extra voters resubmit byte-for-byte copies of earlier ballots.  The reference's proofs bind nothing of the voter, so
// every copy of an accepted ballot verifies; the flow weeds between verify and tally (weed = eg_*_weed: ballots that repeat a ciphertext
// are flagged), prints the number dropped, tallies what is left (tally_grouped over the weeded status words) and reaches the same totals.
// With --board-index (only with --replays) the weeding runs as a board of a long election would run it: the board and its index
// (BoardIndex = eg_weed_index_*) stay in device memory, the honest voters and the replays are two batches through weed_indexed_device, and
// the same two lines are printed.
// With --signed K every voter signs their packed ballot (Ed25519 under the election's prefix) with a key of the voters' roster, and K
// envelopes are forged: a right signature under another voter's roster index, or a flipped bit.  The signature pass (Ed25519::verify =
// eg_ed25519_verify_batch) runs before the ballots are verified; its status words are chained with the verifier's, and the K forgeries,
// and only they, are left out of the tally (tally_grouped over the chained words) - their ballots themselves are perfectly valid.
// With --revotes K (choice ballots), K voters cast a second ballot with another choice.  Both ballots are fresh and valid, so neither
// verification nor weeding objects; the voter-roll pass (VoterRoll::cast = eg_roll_cast, policy EG_ROLL_LAST: the last ballot of a
// voter counts) runs between weeding and the tally, reports the K first ballots as superseded and hands the voters' precincts and
// weights to the tally from the roster (groups_out / weights_out: --precincts and --weighted combine with it); the decrypted totals
// must equal those of the last ballots.
// With --receipts K, after the tally, the accepted ballots are posted to the receipt log (ReceiptLog = eg_merkle_*: a Merkle tree over the
// ballots' leaf hashes under the election's prefix); the root and the size are printed, the receipts of K accepted ballots are issued
// and checked against the root together with one forged receipt (a flipped bit in its leaf), and the verdicts are printed.
// With --heads K (only with --receipts), K earlier sizes of the log spread over 1 .. N stand for the heads that voters and monitors were
// given before: their heads are re-derived from the node store (heads = eg_merkle_heads), their consistency proofs against the present
// head are issued and checked (consistency / consistency_check: the board only grew), and one old head with a flipped bit must be
// refused as the old root's mismatch; one summary line is printed.
// With --grow (only with --receipts), the log is taken as two batches: the tree of the first half of its leaves is built, the tree of the
// whole log is GROWN out of it (grow = eg_merkle_grow: only what the second batch changed is hashed), and its root and node store must
// equal those of the rebuild; one summary line is printed.
// With --audits K (choice ballots), K extra ballots are CHALLENGED instead of cast (the Benaloh challenge of Helios and ElectionGuard): the
// voting device opens them - the value and the encryption randomness of every ciphertext -, the audit pass (open_check = eg_*_open_check)
// re-encrypts and compares, and the one device that encrypted another option than the voter pressed is caught.  Every audited ballot,
// whatever its verdict, is spoiled: its ciphertexts go onto weeding's board, and a device that casts an opened ballot after all is
// flagged EG_DUP_PRIOR by the weeding of the cast batch.
//
//   g++ -std=c++17 -Iinclude examples/voting.cpp -Lelastic_elgamal_amd -leg_hip -Wl,-rpath,$PWD/elastic_elgamal_amd -o voting
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>

#include <dlfcn.h>

#include "elastic_elgamal_hip.hpp"

using namespace elastic_elgamal_hip;

// the voters' randomness (rand::rng() in the reference): splitmix64, so that a run is reproducible from its seed
struct Rng {
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  uint64_t below(uint64_t n) { return next() % n; }
  bool chance(double p) { return (double)(next() >> 11) / 9007199254740992.0 < p; }
};

// Self::tally (examples/voting.rs:122-177) with one key: decrypt each total = blinded - [sk]random, look it up in
// DiscreteLogTable::new(0..=max), compare with the expected totals
static bool tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const std::vector<Ciphertext>& totals,
                  const std::vector<uint64_t>& expected, uint64_t max_value, std::vector<uint64_t>* decrypted = nullptr) {
  std::vector<uint64_t> range(max_value + 1);
  for (uint64_t m = 0; m <= max_value; ++m) range[m] = m;
  const DiscreteLogTable lookup(ctx, range);
  bool ok = true;
  for (size_t k = 0; k < totals.size(); ++k) {
    const Element dh = group.mul(totals[k].random_element, sk);                 // Element * &Scalar
    const Element m_g = group.sub(totals[k].blinded_element, dh);
    const std::optional<uint64_t> found = lookup.get(m_g);
    if (!found) { printf("  variant #%zu: decryption failed\n", k + 1); return false; }
    printf("  variant #%zu decrypted tally: %llu (expected %llu)\n", k + 1, (unsigned long long)*found, (unsigned long long)expected[k]);
    ok = ok && *found == expected[k];
    if (decrypted) decrypted->push_back(*found);
  }
  return ok;
}

// --precincts: the totals of every precinct from the batch that was just verified, decrypted like the overall totals; they must equal
// what the precinct's voters chose and add up to the overall result
template <class Params, class Verdict>
static bool precinct_tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const Params& params, const Bytes& ballots,
                           const Verdict& verdict, uint32_t precincts, const std::vector<std::vector<uint64_t>>& expected_by_precinct,
                           const std::vector<uint64_t>& expected, uint64_t max_value) {
  const size_t votes = verdict.results.size();
  std::vector<uint32_t> status(votes), groups(votes);
  for (size_t v = 0; v < votes; ++v) { status[v] = verdict.results[v] ? 1u : 0u; groups[v] = (uint32_t)(v % precincts); }
  const GroupedTally by = params.tally_grouped(ballots, status, groups, precincts);
  std::vector<uint64_t> sum(expected.size(), 0);
  size_t accepted = 0;
  bool ok = true;
  for (uint32_t p = 0; p < precincts; ++p) {
    printf("precinct #%u: %u accepted ballots\n", p + 1, by.accepted[p]);
    std::vector<uint64_t> got;
    ok = tally(ctx, group, sk, by.totals[p], expected_by_precinct[p], max_value, &got) && ok;
    for (size_t k = 0; k < got.size() && k < sum.size(); ++k) sum[k] += got[k];
    accepted += by.accepted[p];
  }
  ok = ok && sum == expected && accepted == verdict.accepted();
  printf("precinct totals %s the overall totals\n", ok ? "add up to" : "DO NOT add up to");
  return ok;
}

// --weighted: every accepted ballot counts weight(v) times; votes_of[v * options + k] = what voter v gave option k
static uint64_t weight_of(size_t v) { return 1 + (7919 * (uint64_t)v) % 65535; }
template <class Params, class Verdict>
static bool weighted_tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const Params& params, const Bytes& ballots,
                           const Verdict& verdict, const std::vector<uint32_t>& votes_of, size_t options, uint64_t max_per_option) {
  const size_t votes = verdict.results.size();
  std::vector<uint32_t> status(votes);
  std::vector<uint64_t> weights(votes), expected(options, 0);
  for (size_t v = 0; v < votes; ++v) {
    status[v] = verdict.results[v] ? 1u : 0u;
    weights[v] = weight_of(v);
    printf("weighted voter #%zu: weight %llu, votes", v + 1, (unsigned long long)weights[v]);
    for (size_t k = 0; k < options; ++k) {
      printf(" %u", votes_of[v * options + k]);
      if (!status[v]) expected[k] += weights[v] * votes_of[v * options + k];
    }
    printf(", %s\n", status[v] ? "rejected" : "accepted");
  }
  const WeightedTally w = params.tally_weighted(ballots, status, weights, 16);          // one group: every ballot
  if (w.weight_sums[0].high) { printf("the weights add up to more than 64 bits\n"); return false; }
  const uint64_t weight_sum = w.weight_sums[0].low;
  printf("sum of the counted weights: %llu\n", (unsigned long long)weight_sum);
  std::vector<Element> decrypted;
  for (const Ciphertext& c : w.totals[0]) decrypted.push_back(group.sub(c.blinded_element, group.mul(c.random_element, sk)));
  const DiscreteLogSolver solver(ctx);
  const std::vector<std::optional<uint64_t>> found = solver.solve(decrypted, 0, weight_sum * max_per_option);
  bool ok = w.accepted[0] == verdict.accepted();
  for (size_t k = 0; k < options; ++k) {
    if (!found[k]) { printf("weighted total of option #%zu: not found\n", k + 1); ok = false; continue; }
    printf("weighted total of option #%zu: %llu\n", k + 1, (unsigned long long)*found[k]);
    ok = ok && *found[k] == expected[k];
  }
  printf("%s: the decrypted weighted totals %s the expected ones\n", ok ? "OK" : "MISMATCH", ok ? "equal" : "differ from");
  return ok;
}

// --board-index: the board and its index live in device memory between batches.  The C++ interface takes device pointers and leaves the
// allocation to the host, so the example asks the HIP runtime that libeg_hip.so has already loaded, by name
struct DeviceMemory {
  int (*alloc)(void**, size_t) = (int (*)(void**, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
  int (*release)(void*) = (int (*)(void*))dlsym(RTLD_DEFAULT, "hipFree");
  int (*copy)(void*, const void*, size_t, int) = (int (*)(void*, const void*, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
  std::vector<void*> held;
  ~DeviceMemory() { for (void* p : held) release(p); }
  void* take(size_t bytes, const void* from = nullptr) {
    void* p = nullptr;
    if (!alloc || !release || !copy || alloc(&p, bytes ? bytes : 16) != 0) throw Error(EG_ERR_HIP, "no device memory for the board index");
    held.push_back(p);
    if (from && bytes) up(p, from, bytes);
    return p;
  }
  void up(void* to, const void* from, size_t bytes) { if (copy(to, from, bytes, 1) != 0) throw Error(EG_ERR_HIP, "host to device copy"); }
  void down(void* to, const void* from, size_t bytes) { if (copy(to, from, bytes, 2) != 0) throw Error(EG_ERR_HIP, "device to host copy"); }
};
// The batches of a day against one board: each through weed_indexed_device, which reads the index, appends the kept ciphertexts to the
// board and adds exactly those to the index - O(batch) per call, where weed() re-inserts the whole board.  Here the honest voters are the
// first batch and the replays the second; every replay is then EG_DUP_PRIOR, a ciphertext that is already on the board
template <class Params>
static Weeded weed_with_board_index(const Context& ctx, const Params& params, const Bytes& all, const std::vector<uint32_t>& status, size_t first_batch,
                                    size_t options) {
  const size_t size = params.ballot_size(), total = status.size(), board_cap = total * options;
  std::random_device rd;
  auto draw = [&] { return ((uint64_t)rd() << 32) ^ (uint64_t)rd(); };
  const BoardIndex index{ctx, board_cap, draw()};                               // the seed stays unpublished for the life of the index
  DeviceMemory dev;
  void* d_ballots = dev.take(all.size(), all.data());
  void* d_status = dev.take(total * 4, status.data());
  void* d_board = dev.take(board_cap * 64);
  void* d_index = dev.take(index.bytes());
  void* d_dup = dev.take(total * 4);
  void* d_words = dev.take(32);                                                  // the board count (uint64), then found[3]
  index.build_device(0, d_board, d_index, static_cast<char*>(d_words) + 8);      // an empty board
  Weeded w;
  w.dup_of.resize(total);
  w.status.resize(total);
  uint64_t n_prior = 0;
  for (size_t at = 0; at < total;) {
    const size_t n = at < first_batch ? first_batch - at : total - at;
    void* d_scratch = dev.take(params.weed_indexed_scratch_bytes(n));
    char* status_at = static_cast<char*>(d_status) + 4 * at;
    params.weed_indexed_device(n, static_cast<char*>(d_ballots) + at * size, status_at, n_prior, d_board, board_cap, d_index, index.index_seed,
                               draw(), d_scratch, static_cast<char*>(d_dup) + 4 * at, status_at, d_words,
                               static_cast<char*>(d_words) + 8);
    struct { uint64_t count; uint32_t found[3], pad[3]; } words;
    dev.down(&words, d_words, 32);                                               // (hipMemcpy waits for the pass)
    if (words.found[2]) throw Error(EG_ERR_BAD_ARG, "the board has no room");
    printf("board index: batch of %zu ballots against a board of %llu ciphertexts, %llu after it\n", n, (unsigned long long)n_prior,
           (unsigned long long)words.count);
    n_prior = words.count;
    at += n;
  }
  dev.down(w.dup_of.data(), d_dup, total * 4);
  dev.down(w.status.data(), d_status, total * 4);
  return w;
}

// --replays: K extra voters resubmit copies of earlier ballots; verify, weed, tally what is left - the totals of the honest voters
template <class Params>
static bool replayed_tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const Params& params, const Bytes& ballots, size_t votes,
                           size_t replays, const std::vector<uint64_t>& expected, uint64_t max_value, bool board_index = false) {
  const size_t size = params.ballot_size();
  Bytes all = ballots;
  for (size_t i = 0; i < replays; ++i) {
    const size_t from = (7 * i + 1) % votes;
    all.insert(all.end(), ballots.begin() + from * size, ballots.begin() + (from + 1) * size);
  }
  const auto verdict = params.verify_batch(all);
  printf("with %zu replayed ballots: %zu of %zu ballots verified\n", replays, verdict.accepted(), votes + replays);
  std::vector<uint32_t> status(votes + replays);
  size_t copies_accepted = 0;
  for (size_t v = 0; v < votes + replays; ++v) { status[v] = verdict.results[v] ? 1u : 0u; copies_accepted += v >= votes && !status[v]; }
  const Weeded w = board_index ? weed_with_board_index(ctx, params, all, status, votes, expected.size()) : params.weed(all, status);
  for (size_t v = 0; v < w.dup_of.size(); ++v) {
    if (w.dup_of[v] == EG_DUP_PRIOR) printf("  voter #%zu dropped: repeats a ciphertext that is on the board\n", v + 1);
    else if (w.dup_of[v] != EG_DUP_NONE) printf("  voter #%zu dropped: repeats a ciphertext of voter #%u\n", v + 1, w.dup_of[v] + 1);
  }
  printf("weeding dropped %zu ballots\n", w.dropped());
  const GroupedTally kept = params.tally_grouped(all, w.status, std::vector<uint32_t>(votes + replays, 0u), 1);
  bool ok = w.dropped() == copies_accepted && kept.accepted[0] == verdict.accepted() - copies_accepted;
  for (size_t v = 0; v < votes; ++v) ok = ok && w.dup_of[v] == EG_DUP_NONE;
  ok = tally(ctx, group, sk, kept.totals[0], expected, max_value) && ok;
  printf("the weeded totals %s those without the replays\n", ok ? "equal" : "DIFFER from");
  return ok;
}

// --audits: K extra ballots are opened, checked and spoiled instead of cast; the first comes from a device that cheats
static bool audited_ballots(const ChoiceParams& params, const Bytes& ballots, size_t votes, size_t audits, size_t options, uint64_t seed, Rng& rng) {
  const size_t size = params.ballot_size(), words = (options + 31) / 32;
  std::vector<size_t> pressed(audits), encrypted(audits);
  for (size_t i = 0; i < audits; ++i) encrypted[i] = pressed[i] = (size_t)rng.below(options);
  encrypted[0] = (pressed[0] + 1) % options;                                     // this device encrypts another option than was pressed
  const Bytes pile = params.encrypt_single_choices(seed, votes, encrypted);      // the devices commit to their ballots ...
  std::vector<uint32_t> sel(audits * words, 0u);
  for (size_t i = 0; i < audits; ++i) sel[i * words + encrypted[i] / 32] |= 1u << (encrypted[i] % 32);
  Opening opening = params.open_batch(seed, votes, audits, 0, 0, sel);           // ... and open them when challenged (test openings: eg_hip.h)
  for (size_t k = 0; k < options; ++k) opening.values[k] = k == pressed[0] ? 1u : 0u;   // the cheat claims what the voter pressed
  const Audited a = params.open_check(pile, opening);
  printf("%u ballots audited, %u failed\n", a.participated, a.failed);
  bool ok = a.participated == audits && a.failed == 1 && EG_STATUS_KIND(a.status[0]) == EG_ST_BAD_OPENING;
  for (size_t i = 0; i < audits; ++i)
    if (a.status[i])
      printf("  audited ballot #%zu: ciphertext #%u does not open to the claimed value (check %u)\n", i + 1,
             EG_OPEN_DETAIL_SLOT(EG_STATUS_DETAIL(a.status[i])) + 1, EG_OPEN_DETAIL_CHECK(EG_STATUS_DETAIL(a.status[i])));
  const Weeded spoiled = params.weed(pile);                                      // every audited ballot is spoiled, whatever its verdict
  ok = ok && spoiled.appended.size() == audits * options * 64;
  Bytes all = ballots;                                                           // a device casts the last opened ballot after all
  all.insert(all.end(), pile.end() - size, pile.end());
  const auto verdict = params.verify_batch(all);
  std::vector<uint32_t> status(votes + 1);
  for (size_t v = 0; v <= votes; ++v) status[v] = verdict.results[v] ? 1u : 0u;
  const Weeded w = params.weed(all, status, spoiled.appended, false);
  ok = ok && status[votes] == 0u && w.dup_of[votes] == EG_DUP_PRIOR && w.dropped() == 1;
  printf("%s: the opened ballot that was cast again %s\n", ok ? "OK" : "MISMATCH", w.dup_of[votes] == EG_DUP_PRIOR ? "is on the board and dropped" : "WAS NOT FLAGGED");
  return ok;
}

// --revotes: K voters cast a second ballot with another choice; verify, weed, roll (the last ballot counts), tally with the roster's
// precincts and weights - the totals of the last ballots
static bool revoted_tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const ChoiceParams& params, const Bytes& ballots,
                          const std::vector<size_t>& choices, size_t revotes, size_t options, uint32_t precincts, bool weighted, uint64_t seed) {
  const size_t votes = choices.size(), n = votes + revotes;
  std::vector<uint32_t> voter(n);
  std::vector<size_t> cast_choice = choices, again(revotes);
  for (size_t v = 0; v < votes; ++v) voter[v] = (uint32_t)v;
  for (size_t i = 0; i < revotes; ++i) {
    voter[votes + i] = (uint32_t)((7 * i) % votes);
    again[i] = (choices[voter[votes + i]] + 1) % options;
    cast_choice.push_back(again[i]);
  }
  Bytes all = ballots;
  const Bytes second = params.encrypt_single_choices(seed ^ 0x5ec0ull, votes, again);
  all.insert(all.end(), second.begin(), second.end());
  const auto verdict = params.verify_batch(all);
  printf("with %zu re-votes: %zu of %zu ballots verified\n", revotes, verdict.accepted(), n);
  std::vector<uint32_t> status(n);
  for (size_t b = 0; b < n; ++b) status[b] = verdict.results[b] ? 1u : 0u;
  const Weeded w = params.weed(all, status);                       // a superseded ballot's ciphertexts still belong on the board
  // the roster: voter v's precinct and weight, whatever the ballots say
  const uint32_t n_groups = precincts ? precincts : 1u;
  std::vector<uint32_t> roster_groups(votes);
  std::vector<uint64_t> roster_weights(votes), words(votes, 0);
  for (size_t v = 0; v < votes; ++v) { roster_groups[v] = (uint32_t)(v % n_groups); roster_weights[v] = weighted ? weight_of(v) : 1; }
  const VoterRoll roll{ctx, EG_ROLL_LAST};
  const RollVerdicts r = roll.cast(voter, words, 0, w.status, roster_groups, roster_weights);
  for (size_t b = 0; b < n; ++b)
    if (r.superseded_by[b] != EG_SEQ_NONE) printf("  ballot #%zu superseded by ballot #%llu\n", b + 1, (unsigned long long)r.superseded_by[b] + 1);
  printf("the roll superseded %u ballots\n", r.found[0]);
  // what the last accepted ballot of every voter adds up to, per precinct
  std::vector<std::vector<uint64_t>> expected(n_groups, std::vector<uint64_t>(options, 0));
  std::vector<uint64_t> weight_sum(n_groups, 0);
  std::vector<long> last(votes, -1);
  size_t superseded = 0;
  for (size_t b = 0; b < n; ++b) if (!w.status[b]) { superseded += last[voter[b]] >= 0; last[voter[b]] = (long)b; }
  for (size_t v = 0; v < votes; ++v) {
    if (last[v] < 0) continue;
    expected[roster_groups[v]][cast_choice[(size_t)last[v]]] += roster_weights[v];
    weight_sum[roster_groups[v]] += roster_weights[v];
  }
  const WeightedTally t = params.tally_weighted(all, r.status_out, r.weights_out, 16, r.groups_out, n_groups);
  bool ok = r.found[0] == superseded && r.found[2] == 0 && r.displaced.empty();
  const DiscreteLogSolver solver(ctx);
  for (uint32_t g = 0; g < n_groups; ++g) {
    std::vector<Element> decrypted;
    for (const Ciphertext& c : t.totals[g]) decrypted.push_back(group.sub(c.blinded_element, group.mul(c.random_element, sk)));
    const std::vector<std::optional<uint64_t>> found = solver.solve(decrypted, 0, weight_sum[g]);
    ok = ok && t.weight_sums[g].low == weight_sum[g] && !t.weight_sums[g].high;
    for (size_t k = 0; k < options; ++k) {
      if (precincts) printf("  precinct #%u", g + 1);
      printf("  variant #%zu total after the roll: %llu (expected %llu)\n", k + 1, found[k] ? (unsigned long long)*found[k] : 0ull,
             (unsigned long long)expected[g][k]);
      ok = ok && found[k] && *found[k] == expected[g][k];
    }
  }
  printf("the totals %s those of the last ballots\n", ok ? "equal" : "DIFFER from");
  return ok;
}

// --signed: every voter signs the packed ballot under a roster key; K envelopes are forged; signature pass -> verify -> tally of the rest
template <class Params>
static bool signed_tally(const Context& ctx, const Ristretto& group, const Scalar& sk, const Params& params, const Bytes& ballots, size_t votes,
                         size_t forgeries, const std::vector<uint32_t>& votes_of, size_t options, uint64_t max_value, uint64_t seed) {
  const size_t size = params.ballot_size();
  const Ed25519 ed{ctx};
  const char* election = "voting.cpp election #1";
  const Bytes prefix(election, election + strlen(election));
  Rng rng{seed ^ 0x5167ull};
  Bytes seeds(32 * votes);
  for (auto& b : seeds) b = (uint8_t)rng.next();
  const Bytes roster = ed.keypairs(seeds);                       // the registered voters' keys; voter v holds seed v
  Bytes sigs = ed.sign(seeds, ballots, size, prefix);
  std::vector<uint32_t> index(votes);
  for (size_t v = 0; v < votes; ++v) index[v] = (uint32_t)v;
  std::vector<bool> forged(votes, false);
  for (size_t i = 0; i < forgeries; ++i) {
    const size_t v = votes - 1 - i;
    forged[v] = true;
    if (i % 2) index[v] = (uint32_t)((v + 1) % votes);           // somebody else's place in the roster
    else sigs[64 * v + (i % 64)] ^= 1;                           // a flipped bit
  }
  const std::vector<uint32_t> sig_status = ed.verify(ballots, size, roster, sigs, prefix, index);     // BEFORE the ballots are looked at
  size_t refused = 0;
  bool ok = true;
  for (size_t v = 0; v < votes; ++v) {
    if (sig_status[v]) { ++refused; printf("  voter #%zu refused: bad signature (check %u)\n", v + 1, EG_STATUS_DETAIL(sig_status[v])); }
    ok = ok && (sig_status[v] != 0) == forged[v] && (!sig_status[v] || EG_STATUS_KIND(sig_status[v]) == EG_ST_BAD_SIGNATURE);
  }
  printf("%zu forged envelopes: the signature pass refused %zu of %zu\n", forgeries, refused, votes);
  const auto verdict = params.verify_batch(ballots);
  std::vector<uint32_t> chained(votes);
  std::vector<uint64_t> expected(options, 0);
  size_t counted = 0;
  for (size_t v = 0; v < votes; ++v) {
    chained[v] = sig_status[v] ? sig_status[v] : verdict.results[v] ? 1u : 0u;
    if (chained[v]) continue;
    ++counted;
    for (size_t k = 0; k < options; ++k) expected[k] += votes_of[v * options + k];
  }
  const GroupedTally kept = params.tally_grouped(ballots, chained, std::vector<uint32_t>(votes, 0u), 1);
  ok = ok && refused == forgeries && kept.accepted[0] == counted;
  ok = tally(ctx, group, sk, kept.totals[0], expected, max_value) && ok;
  printf("the forgeries%s are left out of the tally\n", ok ? ", and only they," : " and the tally DISAGREE: not only they");
  return ok;
}

// serde's human-readable form of an EncryptedChoice (src/serde.rs:19-80: every element and scalar as unpadded base64url; field names of
// choice.rs:276-280, ring.rs:282-287, log_equality.rs:96-101), from the packed ballot
static std::string b64url(const uint8_t* p, size_t n) {
  static const char* A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
  std::string out;
  for (size_t i = 0; i < n; i += 3) {
    const uint32_t v = (uint32_t)p[i] << 16 | (i + 1 < n ? (uint32_t)p[i + 1] << 8 : 0u) | (i + 2 < n ? (uint32_t)p[i + 2] : 0u);
    out += A[v >> 18]; out += A[(v >> 12) & 63];
    if (i + 1 < n) out += A[(v >> 6) & 63];
    if (i + 2 < n) out += A[v & 63];
  }
  return out;
}
static std::string choice_to_json(const uint8_t* b, size_t options) {
  auto item = [&](size_t k) { return "\"" + b64url(b + 32 * k, 32) + "\""; };
  std::string s = "{\"choices\":[";
  for (size_t k = 0; k < options; ++k)
    s += std::string(k ? "," : "") + "{\"random_element\":" + item(2 * k) + ",\"blinded_element\":" + item(2 * k + 1) + "}";
  s += "],\"range_proof\":{\"common_challenge\":" + item(2 * options) + ",\"ring_responses\":[";
  for (size_t k = 0; k < 2 * options; ++k) s += std::string(k ? "," : "") + item(2 * options + 1 + k);
  s += "]},\"sum_proof\":{\"challenge\":" + item(4 * options + 1) + ",\"response\":" + item(4 * options + 2) + "}}";
  return s;
}

// --heads: K earlier sizes of the log spread over 1 .. N: their heads out of the node store, their consistency proofs against the present
// head, all proven; then one old head with a flipped bit, refused as the old root's mismatch
static bool heads_check(const ReceiptLog& receipts, const Bytes& log, const MerkleTree& tree, size_t k) {
  const uint64_t size = log.size() / EG_MERKLE_HASH_BYTES;
  if (size == 0 || k == 0) { printf("past heads: none to check\n"); return true; }
  std::vector<uint64_t> old;
  for (size_t j = 0; j < k; ++j) old.push_back(k == 1 ? size : 1 + (uint64_t)j * (size - 1) / (k - 1));
  uint64_t bent = 0;                                               // an old size with a seed: not a power of two, below N
  for (uint64_t m : old) if (!bent && m < size && (m & (m - 1))) bent = m;
  if (!bent && size >= 4) bent = 3;
  if (bent) old.push_back(bent);
  const PastHeads past = receipts.heads(old, log, tree.nodes);
  Bytes roots = past.heads;
  if (bent) roots[roots.size() - 1] ^= 1;
  const ConsistencyProofs issued = receipts.consistency(old, log, tree.nodes);
  const size_t stride = ((size_t)ReceiptLog::depth(size) + 1) * EG_MERKLE_HASH_BYTES;
  const ConsistencyVerdicts v = receipts.consistency_check(old, roots, issued.proofs, stride, issued.proof_len, size, tree.root);
  size_t proven = 0, entries = 0;
  for (size_t j = 0; j < k; ++j) { proven += v.verdict[j] == 0; entries += issued.proof_len[j]; }
  const bool forged_ok = !bent || v.verdict[k] == EG_MERKLE_MISMATCH_OLD;
  printf("past heads: %zu of %zu consistency proofs proven against the head of %llu leaves (%zu proof entries); forged old head: %s\n", proven, k,
         (unsigned long long)size, entries, !bent ? "none to forge" : forged_ok ? "refused (old root mismatch)" : "NOT refused");
  return proven == k && forged_ok && past.found[0] == 0 && v.found[0] == 0 && v.found[1] == 0 && v.found[2] == 0 && v.found[3] == (bent ? 1u : 0u);
}

// --grow: the log as two batches: the tree of the whole log grown out of the tree of its first half must be the rebuilt tree
static bool grow_check(const ReceiptLog& receipts, const Bytes& log, const MerkleTree& tree) {
  const uint64_t size = log.size() / EG_MERKLE_HASH_BYTES, first = size / 2;
  const MerkleTree old = receipts.tree(Bytes(log.begin(), log.begin() + first * EG_MERKLE_HASH_BYTES));
  const MerkleTree grown = receipts.grow(first, old, log);
  const bool same = grown.root == tree.root && grown.nodes == tree.nodes;
  printf("grown log: the tree of %llu leaves out of the tree of its first %llu: root and node store %s\n", (unsigned long long)size,
         (unsigned long long)first, same ? "equal the rebuild" : "DIFFER from the rebuild");
  return same;
}

// --receipts: the accepted ballots are posted to the receipt log; K receipts and one forged one are checked against the root
static bool receipt_check(const Context& ctx, const Bytes& ballots, size_t ballot_size, const std::vector<uint32_t>& status, size_t k, uint64_t seed,
                          long heads = -1, bool grow = false) {
  const size_t n = status.size();
  const std::string id = "election #" + std::to_string(seed);
  const ReceiptLog receipts{ctx, Bytes(id.begin(), id.end())};
  Bytes log;
  const LeafPass pass = receipts.leaves(ballots, ballot_size, n, {}, status, &log);
  const uint64_t size = log.size() / EG_MERKLE_HASH_BYTES;
  const MerkleTree tree = receipts.tree(log);
  printf("receipt log: %llu leaves, root ", (unsigned long long)size);
  for (uint8_t b : tree.root) printf("%02x", b);
  printf("\n");
  const bool grown_ok = !grow || grow_check(receipts, log, tree);
  std::vector<uint64_t> index;
  Bytes leaves;
  std::vector<size_t> voter;
  for (size_t b = 0; b < n && index.size() < k; ++b) {
    if (pass.leaf_index[b] == EG_LEAF_NONE) continue;
    index.push_back(pass.leaf_index[b]);
    leaves.insert(leaves.end(), pass.leaves.begin() + b * EG_MERKLE_HASH_BYTES, pass.leaves.begin() + (b + 1) * EG_MERKLE_HASH_BYTES);
    voter.push_back(b);
  }
  if (index.empty()) {
    printf("no accepted ballot to issue a receipt for\n");
    return pass.found[0] == 0 && grown_ok && (heads < 0 || heads_check(receipts, log, tree, (size_t)heads));
  }
  index.push_back(index[0]);                                       // the forged receipt: the first one with a flipped bit in its leaf
  leaves.insert(leaves.end(), leaves.begin(), leaves.begin() + EG_MERKLE_HASH_BYTES);
  leaves[leaves.size() - 1] ^= 1;
  const Receipts issued = receipts.paths(index, log, tree.nodes);
  const size_t stride = (size_t)ReceiptLog::depth(size) * EG_MERKLE_HASH_BYTES;
  const ReceiptVerdicts v = receipts.check(index, leaves, issued.paths, stride, issued.path_len, size, tree.root);
  bool ok = pass.found[0] == size && pass.found[1] == 0 && grown_ok;
  for (size_t j = 0; j + 1 < index.size(); ++j) {
    printf("  receipt of voter #%zu: leaf %llu, %u path entries, %s\n", voter[j] + 1, (unsigned long long)index[j], issued.path_len[j],
           v.verdict[j] == 0 ? "proven" : "NOT proven");
    ok = ok && v.verdict[j] == 0;
  }
  const uint32_t forged = v.verdict[index.size() - 1];
  printf("  forged receipt: %s\n", forged == EG_MERKLE_MISMATCH ? "refused (root mismatch)" : "NOT refused");
  ok = ok && forged == EG_MERKLE_MISMATCH && v.found[0] == 0 && v.found[1] == 0 && v.found[2] == 1;
  return heads < 0 ? ok : heads_check(receipts, log, tree, (size_t)heads) && ok;
}

int main(int argc, char** argv) {
  bool qv = false, json = false, weighted = false, grow = false, board_index = false;
  int devices = 1;
  long precincts = 0, replays = 0, signed_forgeries = -1, revotes = 0, receipts = -1, heads = -1, audits = 0;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--qv")) qv = true;
    else if (!strcmp(argv[i], "--json")) json = true;
    else if (!strcmp(argv[i], "--weighted")) weighted = true;
    else if (!strcmp(argv[i], "--grow")) grow = true;
    else if (!strcmp(argv[i], "--board-index")) board_index = true;
    else if (!strcmp(argv[i], "--devices") && i + 1 < argc) devices = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--precincts") && i + 1 < argc) precincts = atol(argv[++i]);
    else if (!strcmp(argv[i], "--replays") && i + 1 < argc) replays = atol(argv[++i]);
    else if (!strcmp(argv[i], "--signed") && i + 1 < argc) signed_forgeries = atol(argv[++i]);
    else if (!strcmp(argv[i], "--revotes") && i + 1 < argc) revotes = atol(argv[++i]);
    else if (!strcmp(argv[i], "--audits") && i + 1 < argc) audits = atol(argv[++i]);
    else if (!strcmp(argv[i], "--receipts") && i + 1 < argc) receipts = atol(argv[++i]);
    else if (!strcmp(argv[i], "--heads") && i + 1 < argc) heads = atol(argv[++i]);
    else pos.push_back(argv[i]);
  }
  auto arg = [&](size_t k, uint64_t dflt) { return k < pos.size() ? strtoull(pos[k].c_str(), nullptr, 10) : dflt; };
  const size_t votes = (size_t)arg(0, 1000), options = (size_t)arg(1, 5);
  const uint64_t credits = qv ? arg(2, 20) : 0, seed = arg(qv ? 3 : 2, 1);
  if (devices < 1 || devices > 16) { printf("--devices must be in 1..16\n"); return 2; }
  if (replays < 0 || replays > 1000000 || (replays && !votes)) { printf("--replays must be in 0..1000000 and needs a voter to copy\n"); return 2; }
  if (signed_forgeries < -1 || (signed_forgeries >= 0 && (size_t)signed_forgeries > votes) || (signed_forgeries > 0 && votes < 2)) {
    printf("--signed K needs 0 <= K <= votes and two voters to forge\n"); return 2;
  }
  if (revotes < 0 || (revotes && (qv || options < 2 || (size_t)revotes * 7 > votes))) {
    printf("--revotes K is shown for choice ballots with two options or more and needs 7 K <= votes\n"); return 2;
  }
  if (audits < 0 || audits > 1000000 || (audits && (qv || options < 2))) { printf("--audits K is shown for choice ballots with two options or more, K in 0..1000000\n"); return 2; }
  if (receipts < -1 || receipts > 1000000) { printf("--receipts must be in 0..1000000\n"); return 2; }
  if (heads < -1 || heads > 1000000 || (heads >= 0 && receipts < 0)) { printf("--heads must be in 0..1000000 and needs --receipts\n"); return 2; }
  if (grow && receipts < 0) { printf("--grow needs --receipts\n"); return 2; }
  if (precincts < 0 || precincts > (long)EG_TALLY_GROUPS_MAX) { printf("--precincts must be in 0..%u\n", EG_TALLY_GROUPS_MAX); return 2; }

  // one context per device slot; slot d uses GPU d when the process sees that many, else GPU 0
  std::vector<std::unique_ptr<Context>> ctxs;
  for (int d = 0; d < devices; ++d) {
    try { ctxs.push_back(std::make_unique<Context>(d)); }
    catch (const Error&) { if (d == 0) throw; ctxs.push_back(std::make_unique<Context>(0)); }
  }
  const Context& ctx = *ctxs[0];
  Ristretto group{ctx};

  // Keypair::generate: secret scalar from 64 seed-derived bytes, public key = [sk]G
  std::array<uint8_t, 64> wide{};
  for (size_t i = 0; i < 64; ++i) wide[i] = (uint8_t)((seed * 0x9E3779B97F4A7C15ull >> (i % 8 * 8)) + 31 * i);
  const Scalar sk = group.scalar_from_random_bytes(wide);
  const Element pk = group.mul_generator(sk);
  Rng rng{seed ^ 0xC0FFEEull};
  std::vector<uint64_t> expected(options, 0);
  std::vector<std::vector<uint64_t>> expected_by_precinct((size_t)precincts, std::vector<uint64_t>(options, 0));
  bool ok = true;

  if (!qv) {
    std::vector<std::unique_ptr<ChoiceParams>> params;
    for (auto& c : ctxs) params.push_back(std::make_unique<ChoiceParams>(ChoiceParams::single(*c, pk, options)));
    std::vector<size_t> choices(votes);
    for (auto& c : choices) c = (size_t)rng.below(options);                            // rng.random_range(0..options_count)
    Bytes ballots = params[0]->encrypt_single_choices(seed, 0, choices);               // EncryptedChoice::single(&params, choice, rng)
    const size_t forged = votes > 3 ? 3 : votes;                                       // one forged ballot must be rejected
    if (forged < votes) ballots[forged * params[0]->ballot_size() + 64 * options + 40] ^= 1;
    for (size_t i = 0; i < votes; ++i) if (i != forged) expected[choices[i]] += 1;
    for (size_t i = 0; precincts && i < votes; ++i) if (i != forged) expected_by_precinct[i % precincts][choices[i]] += 1;
    std::vector<const ChoiceParams*> per;
    for (auto& p : params) per.push_back(p.get());
    BatchVerdict<ChoiceVerificationError> verdict;
    if (json) {
      // println!("{}", serde_json::to_string_pretty(&encrypted)) per voter (examples/voting.rs:195-198): every ballot is fed as it is made
      // --devices N: ONE parser for all GPUs (eg_verify_choice_json_begin_multi: the packed windows are dealt to the params objects by load),
      // and every ballot's text is handed over without a copy (eg_verify_json_feed_owned: the stream gives the block back when it is through)
      std::unique_ptr<JsonStream> sp(devices > 1 ? new JsonStream(per, 4) : new JsonStream(*params[0], 4));
      JsonStream& stream = *sp;
      const size_t bs = params[0]->ballot_size();
      for (size_t i = 0; i < votes; ++i) {
        std::string text = choice_to_json(ballots.data() + i * bs, options) + "\n";
        if (devices > 1) stream.feed_owned(std::make_shared<const std::string>(std::move(text)));
        else stream.feed(text);
      }
      std::vector<Ciphertext> totals;
      for (uint32_t st : stream.finish(&totals)) verdict.results.push_back(choice_error_from_status(st));
      verdict.totals = totals;
      printf("(%zu ballots went through the JSON stream one at a time%s)\n", stream.objects(), devices > 1 ? ", one parser for all devices, blocks handed over" : "");
    } else
      verdict = devices > 1 ? verify_batch_multi(per, ballots) : params[0]->verify_batch(ballots);   // encrypted.verify(&params)
    printf("%zu of %zu ballots verified\n", verdict.accepted(), votes);
    for (size_t i = 0; i < verdict.results.size(); ++i)
      if (verdict.results[i]) printf("  voter #%zu rejected: %s\n", i + 1, verdict.results[i]->to_string().c_str());
    ok = verdict.accepted() == votes - (forged < votes ? 1 : 0) && tally(ctx, group, sk, verdict.totals, expected, votes);
    if (precincts) ok = precinct_tally(ctx, group, sk, *params[0], ballots, verdict, (uint32_t)precincts, expected_by_precinct, expected, votes) && ok;
    if (weighted) {
      std::vector<uint32_t> one_hot(votes * options, 0u);
      for (size_t i = 0; i < votes; ++i) one_hot[i * options + choices[i]] = 1u;
      ok = weighted_tally(ctx, group, sk, *params[0], ballots, verdict, one_hot, options, 1) && ok;
    }
    if (signed_forgeries >= 0) {
      std::vector<uint32_t> one_hot(votes * options, 0u);
      for (size_t i = 0; i < votes; ++i) one_hot[i * options + choices[i]] = 1u;
      ok = signed_tally(ctx, group, sk, *params[0], ballots, votes, (size_t)signed_forgeries, one_hot, options, votes, seed) && ok;
    }
    if (replays) ok = replayed_tally(ctx, group, sk, *params[0], ballots, votes, (size_t)replays, expected, votes, board_index) && ok;
    if (revotes) ok = revoted_tally(ctx, group, sk, *params[0], ballots, choices, (size_t)revotes, options, (uint32_t)precincts, weighted, seed) && ok;
    if (audits) ok = audited_ballots(*params[0], ballots, votes, (size_t)audits, options, seed, rng) && ok;
    if (receipts >= 0) {
      std::vector<uint32_t> status(votes, 0u);
      for (size_t i = 0; i < votes; ++i) status[i] = verdict.results[i] ? 1u : 0u;
      ok = receipt_check(ctx, ballots, params[0]->ballot_size(), status, (size_t)receipts, seed, heads, grow) && ok;
    }
  } else {
    std::vector<std::unique_ptr<QuadraticVotingParams>> params;
    for (auto& c : ctxs) params.push_back(std::make_unique<QuadraticVotingParams>(*c, pk, options, credits));
    // the reference's vote draw (examples/voting.rs:235-244): add one vote to a random option with probability 0.8 while the credit lasts
    std::vector<uint32_t> all(votes * options, 0u);
    for (size_t i = 0; i < votes; ++i) {
      uint32_t* v = &all[i * options];
      while (rng.chance(0.8)) {
        const size_t k = (size_t)rng.below(options);
        uint64_t credit = 0;
        for (size_t j = 0; j < options; ++j) { const uint64_t x = v[j] + (j == k ? 1u : 0u); credit += x * x; }
        if (credit > credits) break;
        v[k] += 1;
      }
    }
    Bytes ballots = params[0]->encrypt_votes_batch(seed, 0, all);                      // QuadraticVotingBallot::new(&vote_params, &votes, rng)
    const size_t forged = votes > 3 ? 3 : votes;
    if (forged < votes) ballots[forged * params[0]->ballot_size() + params[0]->ballot_size() - 40] ^= 1;
    for (size_t i = 0; i < votes; ++i) if (i != forged) for (size_t k = 0; k < options; ++k) expected[k] += all[i * options + k];
    for (size_t i = 0; precincts && i < votes; ++i)
      if (i != forged) for (size_t k = 0; k < options; ++k) expected_by_precinct[i % precincts][k] += all[i * options + k];
    std::vector<const QuadraticVotingParams*> per;
    for (auto& p : params) per.push_back(p.get());
    auto verdict = devices > 1 ? verify_batch_multi(per, ballots) : params[0]->verify_batch(ballots);   // encrypted.verify(&vote_params)
    printf("%zu of %zu quadratic-voting ballots verified\n", verdict.accepted(), votes);
    for (size_t i = 0; i < verdict.results.size(); ++i)
      if (verdict.results[i]) printf("  voter #%zu rejected (error kind %d)\n", i + 1, (int)verdict.results[i]->kind);
    const uint64_t max_votes = votes * params[0]->max_votes();                          // votes_count * vote_params.max_votes()
    ok = verdict.accepted() == votes - (forged < votes ? 1 : 0) && tally(ctx, group, sk, verdict.totals, expected, max_votes);
    if (precincts) ok = precinct_tally(ctx, group, sk, *params[0], ballots, verdict, (uint32_t)precincts, expected_by_precinct, expected, max_votes) && ok;
    if (weighted) ok = weighted_tally(ctx, group, sk, *params[0], ballots, verdict, all, options, params[0]->max_votes()) && ok;
    if (replays) ok = replayed_tally(ctx, group, sk, *params[0], ballots, votes, (size_t)replays, expected, max_votes, board_index) && ok;
    if (signed_forgeries >= 0) ok = signed_tally(ctx, group, sk, *params[0], ballots, votes, (size_t)signed_forgeries, all, options, max_votes, seed) && ok;
    if (receipts >= 0) {
      std::vector<uint32_t> status(votes, 0u);
      for (size_t i = 0; i < votes; ++i) status[i] = verdict.results[i] ? 1u : 0u;
      ok = receipt_check(ctx, ballots, params[0]->ballot_size(), status, (size_t)receipts, seed, heads, grow) && ok;
    }
  }
  printf("%s: the decrypted totals %s the expected ones\n", ok ? "OK" : "MISMATCH", ok ? "equal" : "differ from");
  return ok ? 0 : 1;
}
