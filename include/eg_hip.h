/*
 * eg_hip.h -- C ABI of libeg_hip.so: the MI355X (gfx950) Ristretto255 backend and batch ballot verifier
 * that stands in for the hot path of slowli/elastic-elgamal.
 *
 * Two tiers:
 *
 *  PRIMITIVE TIER -- batched equivalents of the reference's `Group` plugin trait for `Ristretto`
 *  (src/group/mod.rs:65-255, src/group/ristretto.rs:23-146).  A Rust shim
 *  `impl ScalarOps/ElementOps/Group for HipRistretto` binds these one-to-one.  All
 *  buffers are caller-owned HOST memory, 32-byte little-endian encodings exactly as
 *  serialize_scalar / serialize_element produce them; `n` independent problems per call run on the GPU.
 *
 *  BATCH TIER -- `for ballot in ballots { ballot.verify(&params) }` as one call: the reference has no
 *  equivalent entry point (it verifies one ballot at a time on one thread, examples/voting.rs:189-204);
 *  these are what a Rust host calls instead of the loop.  Ballots are packed back to back in the
 *  reference's own byte formats (see "wire layout" below).  `_device` variants take DEVICE pointers and a
 *  hipStream_t (as void*), so that torch / RCCL owned buffers can be passed without copies.
 *
 * Every function returns EG_OK (0) or a negative eg_error.  Nothing here falls back to the CPU: if no
 * gfx950 device is usable eg_init fails with EG_ERR_NO_DEVICE.
 *
 * TIMING (the `Group` contract, src/group/mod.rs:65-135,183-255): the reference requires scalar arithmetic, element addition,
 * `Element * &Scalar`, `mul_generator` and `multi_mul` to be CONSTANT-TIME and lets only the `vartime_*` methods depend on their
 * operands.  NOTHING in this library is constant-time: every multiplication indexes tables in device memory with digits of its scalar
 * (2^19-entry comb windows), the provers branch on the voter's choice, and a GPU shared with other processes is not a place for
 * secrets in the first place.  The library is the VERIFIER-side backend - `EncryptedChoice::verify`, `QuadraticVotingBallot::verify`
 * and everything under them call `vartime_double_mul_generator` / `vartime_multi_mul` on public data only (src/proofs/ring.rs:342-350,
 * log_equality.rs:160-164, mul.rs:213-247).  eg_mul_generator_batch, eg_scalar_*_batch, eg_point_add_batch and the
 * eg_*_encrypt_* provers exist for completeness of the trait, for tests and for making SYNTHETIC ballots (bench.py); a deployment that
 * encrypts real voters' choices, or multiplies by secret keys, keeps those operations on the CPU's constant-time backend
 * (curve25519-dalek), which is what the shim of INTEGRATION.md section 3 does.
 *
 * Threads: entry points may be called from any thread; calls on one context (and on the params objects created on
 * it) are serialised by a lock inside the context, and eg_last_error is per thread.  Host-pointer functions return
 * when the results are in the caller's buffers (they run on a stream owned by the context; the tally reset / encode host
 * forms first wait for the whole device, so they may follow `_device` calls directly).  `_device` / `_async` functions only
 * enqueue work on the hipStream_t they are given - NULL is HIP's null stream, as everywhere.  The context's per-lane workspace, which
 * every params object of a context and the primitive tier share, is ordered INSIDE the library (each user's stream waits for an event
 * of the previous user: no host synchronisation), so two params objects of one context may have work in flight at the same time - a JSON
 * stream on one, `_device` calls or eg_vartime_multi_mul_batch on the other - whatever the streams.  What a caller that uses several
 * streams with ONE params object must still order itself (events) are that object's own buffers: its chunk workspace and running tally.
 * LONG calls - eg_verify_*_json and eg_verify_*_batch_multi* - do not hold the context's lock from start to end, but they are one call all
 * the same: any other call on a params object they are using WAITS until they are over.
 *
 * RUN-TIME KNOBS.  Every environment variable the library looks at, complete (csrc/eg_hip.hip: struct Knobs, read_knobs - the only
 * place the environment is read).  They are read at TWO moments only - eg_init (context-wide knobs; the context keeps its copy) and the
 * creation of a params object (eg_*_params_create; the engine keeps its copy) - never per call: changing the environment afterwards
 * does nothing to live objects.  None of them changes a verdict or a tally (tests force each and compare with the oracle); the shipped
 * library has NO failure-injection switch (tests build their own copy with fault points: tests/faultlib).
 *
 *   name                  read at        default            effect
 *   EG_ALLOW_ANY_ARCH     eg_init        unset              accept a device that is not gfx950 (development only; kernels are built for gfx950)
 *   EG_COMB_BIG_BITS      eg_init        24                 window width of the WIDE fixed-base comb tables (11.8 GB per base); 0 = never build them
 *   EG_COMB_BIG_MIN       eg_init        524288             items an engine must have verified before the wide tables are built for it
 *   EG_MSM_BLOCKS_PER_CU  eg_init        32                 grid of the table / equation / multi-scalar kernels per CU (sets the 2.4 GB per-lane workspace)
 *   EG_MSM_LANES          eg_init        131072             lanes a multi-scalar call should cover before terms share doubling chains (1 = always chunks of 8)
 *   EG_MSM_BUCKET_MIN     eg_init        1048576            terms per product from which the bucket (Pippenger) method replaces Straus; eg_msm_scratch_bytes follows it
 *   EG_TEETH              params create  by plan (5 or 6)   comb shape of the per-ballot tables: 5 x 51 (2 KiB) or 6 x 43 (4 KiB)
 *   EG_STREAMS            params create  2                  work sets (each with its own stream) the chunks of a call alternate between: 1 or 2
 *   EG_CHUNK              params create  by plan / memory   ballots per chunk and work set (default 2^19, or 2^18 where two sets would pass 40 GB)
 *   EG_RING_GROUP         params create  by plan            ring-group walk of choice ballots: rings whose tables are resident at a time; 0 = all
 *                                                           (default: all below 256 options); a memory knob, 0.6-4 % slower
 *   EG_JSON_RING_KB       params create  1048576            pinned staging ring of eg_verify_*_json, KiB
 *   EG_JSON_WINDOW_KB     params create  98304              JSON text per parser window, KiB
 *   EG_JSON_GROWTH        params create  150                a second JSON submission is enqueued once it is this many per cent of the first
 *   EG_JSON_FIRST_MIN     params create  16384              packed ballots the JSON entry points wait for before their first GPU submission
 *   EG_JSON_ODD_MAX_MB    params create  256                text of ballots whose shape is not the election's that a JSON stream keeps for the
 *                                                           object path (they are resolved at the end); a text with more fails with EG_ERR_NOMEM
 *   EG_JSON_TRACE         params create  unset              timeline of the JSON submissions on stderr
 *
 * The Python mirror adds two of its own (elastic_elgamal_amd/__init__.py, read at import): EG_LIB = path of another build of this
 * library (A/B measurements, the fault-point build of the tests), EG_NO_TORCH_PRELOAD = do not import torch before loading the library.
 */
#ifndef EG_HIP_H
#define EG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  EG_OK = 0,
  EG_ERR_NO_DEVICE = -1,
  EG_ERR_HIP = -2,
  EG_ERR_BAD_ARG = -3,
  EG_ERR_BAD_PUBLIC_KEY = -4, /* PublicKey::from_bytes: invalid element or identity (keys/mod.rs:161-176) */
  EG_ERR_NOMEM = -5
} eg_error;

/* ---- per-ballot status words (uint32): low byte = kind, bits 8.. = detail ------------------------------
 * Kinds mirror the reference's error enums (the *_LEN kinds cannot arise in a packed batch, whose shape is fixed by the
 * params; they are produced by the object-ingest layer, elastic_elgamal_amd/ingest.py); precedence = order of checks in EncryptedChoice::verify
 * (choice.rs:358-380) and QuadraticVotingBallot::verify (quadratic_voting.rs:291-329), preceded by the
 * deserialisation-time rejections of serde (serde.rs:191-206,254-269) in wire order. */
enum {
  EG_ST_OK = 0,
  EG_ST_BAD_SCALAR = 1,           /* non-canonical scalar; detail = index of the 32-byte item in the ballot */
  EG_ST_BAD_POINT = 2,            /* invalid ristretto encoding; detail = item index */
  EG_ST_OPTIONS_LEN = 3,          /* ChoiceVerificationError::OptionsLenMismatch (choice.rs:409) */
  EG_ST_SUM_CHALLENGE = 4,        /* ChoiceVerificationError::Sum(ChallengeMismatch) (choice.rs:416) */
  EG_ST_RANGE_LEN = 5,            /* ...::Range(LenMismatch) (choice.rs:418, proofs/mod.rs:73-80) */
  EG_ST_RANGE_CHALLENGE = 6,      /* ...::Range(ChallengeMismatch) */
  EG_ST_QV_VARIANT_LEN = 7,       /* QuadraticVotingError::Variant{index, LenMismatch}; detail = index */
  EG_ST_QV_VARIANT_CHALLENGE = 8, /* QuadraticVotingError::Variant{index, ChallengeMismatch} */
  EG_ST_QV_CREDIT_RANGE_LEN = 9,
  EG_ST_QV_CREDIT_RANGE_CHALLENGE = 10, /* QuadraticVotingError::CreditRange (quadratic_voting.rs:341) */
  EG_ST_QV_CREDIT_EQUIV_LEN = 11,
  EG_ST_QV_CREDIT_EQUIV_CHALLENGE = 12, /* QuadraticVotingError::CreditEquivalence (:343) */
  EG_ST_MALFORMED = 13,           /* the ballot object does not deserialise at all (bad base64url / byte length, fewer than 2
                                     responses, wrong proof kind: serde.rs:29-80,303-355); object-ingest layer only */
  EG_ST_DUPLICATE = 14,           /* no verdict of the reference: an accepted ballot that repeats a tally ciphertext of the board or of an
                                     earlier ballot; written by eg_*_weed* into status_out only, detail 0 */
  EG_ST_BAD_SIGNATURE = 15,       /* no verdict of the reference: the voter's Ed25519 signature over the item does not hold; written by
                                     eg_ed25519_verify* only, detail = which check failed (EG_ED25519_*) */
  EG_ST_SUPERSEDED = 16,          /* no verdict of the reference: not the one ballot of its voter that counts; written by eg_roll_* into
                                     status_out only, detail = why (EG_ROLL_SUPERSEDED / _OFF_ROLL / _NOT_CAST) */
  EG_ST_BAD_OPENING = 17          /* no verdict of the reference: an opened (audited) ballot does not encrypt what its opening says;
                                     written by eg_*_open_check* only, detail = EG_OPEN_DETAIL(slot, check) */
};
#define EG_STATUS_KIND(s) ((s) & 0xffu)
#define EG_STATUS_DETAIL(s) ((s) >> 8)

typedef struct eg_ctx eg_ctx;           /* one per process and GPU: device, stream, fixed-base table of G */
typedef struct eg_choice_params eg_choice_params; /* ChoiceParams<Ristretto, S> (choice.rs:132-196) */
typedef struct eg_qv_params eg_qv_params;         /* QuadraticVotingParams<Ristretto> (quadratic_voting.rs:47-76) */

/* ---- context ------------------------------------------------------------------------------------------------ */
/* Version of this ABI: bumped whenever an exported function changes its prototype or meaning (6 = round 6: eg_msm_scratch_bytes_ctx,
 * d_ok mandatory in eg_points_prepare_device, the multi-GPU JSON entries; 7 = round 7: EG_PROOF_COMMIT_EQUIV and the
 * eg_commit_equiv_* entries).  A binding checks it once after loading the library. */
#define EG_ABI_VERSION 7
int eg_abi_version(void);
int eg_init(int device, eg_ctx** out);   /* no reference analogue: the backend is a ZST */
void eg_destroy(eg_ctx* ctx);
const char* eg_last_error(void);         /* text of the last failure on this thread */
int eg_device_name(eg_ctx* ctx, char* buf, size_t cap);
int eg_synchronize(eg_ctx* ctx);         /* waits for all work on the context's device, whatever stream it was enqueued on */

/* ---- primitive tier (host buffers; n problems per call) ------------------------------------------------------- */
/* ScalarOps::scalar_from_random_bytes / Scalar::from_bytes_mod_order_wide (ristretto.rs:34-38) */
int eg_scalar_from_wide_batch(eg_ctx*, size_t n, const uint8_t* wide /*64n*/, uint8_t* out /*32n*/);
/* ScalarOps::deserialize_scalar -> is Some (ristretto.rs:59-62) */
int eg_scalar_is_canonical_batch(eg_ctx*, size_t n, const uint8_t* s /*32n*/, uint8_t* ok /*n*/);
/* a*b + c, -a  (Scalar Mul/Add/Neg used at ring.rs:192-193,339) */
int eg_scalar_muladd_batch(eg_ctx*, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out);
int eg_scalar_neg_batch(eg_ctx*, size_t n, const uint8_t* a, uint8_t* out);
/* ScalarOps::invert_scalar / invert_scalars (group/mod.rs:104-118, ristretto.rs:40-52): 1/a mod l; 0 maps to 0 */
int eg_scalar_invert_batch(eg_ctx*, size_t n, const uint8_t* a, uint8_t* out);
/* ElementOps::deserialize_element then serialize_element (ristretto.rs:88-95): ok[i] = 1 for a valid
 * encoding, and out = re-encoding (equal to the input for every valid encoding) */
int eg_point_roundtrip_batch(eg_ctx*, size_t n, const uint8_t* in /*32n*/, uint8_t* out /*32n*/, uint8_t* ok /*n*/);
/* ElementOps::is_identity (ristretto.rs:80-82): is_identity[i] = 1 iff the encoding is valid and is the identity */
int eg_point_is_identity_batch(eg_ctx*, size_t n, const uint8_t* in /*32n*/, uint8_t* is_identity /*n*/, uint8_t* ok /*n*/);
/* Element Add / Sub (ristretto.rs:76-86 via RistrettoPoint ops); ok[i]=0 if an input fails to decode.
 * Element Neg is `subtract` with a = identity (32 zero bytes). */
int eg_point_add_batch(eg_ctx*, size_t n, const uint8_t* a, const uint8_t* b, int subtract, uint8_t* out, uint8_t* ok);
/* TranscriptForGroup's framing (proofs/mod.rs:39-57 over merlin 3.0.0): for each of n messages,
 * Transcript::new(proto); append_message(msg_label, msg_i); challenge_bytes(chal_label, out_len) -> out_i.  Lets known-answer
 * vectors of the transcript layer (the upstream merlin test vector) be checked on the device itself. */
int eg_merlin_challenge_batch(eg_ctx*, size_t n, const char* proto, size_t proto_len, const char* msg_label, size_t msg_label_len,
                              const uint8_t* msgs /* n x msg_len */, size_t msg_len, const char* chal_label, size_t chal_label_len,
                              uint8_t* out /* n x out_len */, size_t out_len);
/* Group::mul_generator / vartime_mul_generator (ristretto.rs:105-121); variable time like everything here (see TIMING): this IS
 * vartime_mul_generator, and stands in for mul_generator only where the scalar is public */
int eg_mul_generator_batch(eg_ctx*, size_t n, const uint8_t* k /*32n*/, uint8_t* out /*32n*/);
/* Group::vartime_double_mul_generator(k, P, r) = [k]P + [r]G (ristretto.rs:131-137) */
int eg_vartime_double_mul_generator_batch(eg_ctx*, size_t n, const uint8_t* k, const uint8_t* p, const uint8_t* r,
                                          uint8_t* out, uint8_t* ok);
/* Group::vartime_multi_mul(scalars, elements) (ristretto.rs:139-145): n problems of `terms` terms each,
 * scalars/points laid out [problem][term][32].  Scalars must be canonical (< l), as in the reference; this holds for every
 * multi-scalar entry below too (the Straus path is only correct below 2^253). */
int eg_vartime_multi_mul_batch(eg_ctx*, size_t n, size_t terms, const uint8_t* scalars, const uint8_t* points,
                               uint8_t* out, uint8_t* ok);
/* The same multi-scalar multiplication on DEVICE buffers, asynchronous on `stream`: out_i = enc( sum_t [k_it]P_it + [r_i]G ).
 * d_r may be NULL (no generator term) unless terms == 0; d_ok may be NULL.  Any number of terms up to 2^24: the terms of a problem
 * are evaluated in chunks of 8 on shared doubling chains (Straus, what dalek's vartime_multiscalar_mul does below 190 terms) and the
 * chunks' partial sums are added up with wavefront shuffles; from 2^20 terms per problem on, the bucket method (Pippenger, dalek's choice
 * above 190 terms; csrc/pippenger.cuh) takes over, one problem after the other: 13 ms instead of 21 for 2^22 terms.  A call that is cut
 * into several chunks per problem (more than 8 terms, or few problems of many terms) or that uses the bucket method needs d_scratch of
 * eg_msm_scratch_bytes_ctx(ctx, n, terms) bytes (0 when it needs none; ~250 bytes per term for the bucket method: 1 GB at 2^22 terms).  A caller
 * that keeps its operands in HBM pays no copy and no synchronisation. */
/* (named _ctx since ABI version 6: earlier builds exported this function under the name without the suffix, first WITHOUT the context
 * argument, then with it - a caller built against the old prototype must fail to link, not link and read a garbage size) */
size_t eg_msm_scratch_bytes_ctx(eg_ctx*, size_t n, size_t terms);   /* by the context: its switch to the bucket method is fixed at eg_init */
int eg_vartime_multi_mul_batch_device(eg_ctx*, size_t n, size_t terms, const void* d_scalars, const void* d_points, const void* d_r,
                                      void* d_scratch, void* d_out, void* d_ok, void* stream);

/* Prepared points.  In the reference an Element IS a decoded point, so Group::vartime_multi_mul (ristretto.rs:139-145) never pays a
 * decoding per product; the entry above, which takes 32-byte encodings, does - 285 field operations per term, a third of the bucket
 * method's time.  A caller that multiplies over one point set repeatedly decodes it once: eg_points_prepare_device writes
 * eg_prepared_point_size() (= 96) bytes per point - affine (x, y, xy), an opaque layout that is valid for this library build only, never
 * a wire format - and d_ok[i] = 1 if encoding i decodes.  An encoding that does not decode is prepared as the IDENTITY and contributes
 * nothing to a product; the reference cannot even construct such an Element (deserialize_element returns None), so d_ok is MANDATORY
 * (EG_ERR_BAD_ARG if NULL): the prepare call is the only place that says which inputs were not elements.  d_prepared must be 16-byte
 * aligned (hipMalloc'd memory is; EG_ERR_BAD_ARG otherwise - the kernels read it in 128-bit words), also in
 * eg_vartime_multi_mul_prepared_batch_device, which is eg_vartime_multi_mul_batch_device over such points (terms per problem x n problems,
 * 96 bytes each, same scratch, same paths) and has no ok output of its own. */
size_t eg_prepared_point_size(void);
int eg_points_prepare_device(eg_ctx*, size_t n, const void* d_encodings, void* d_prepared, void* d_ok, void* stream);
int eg_vartime_multi_mul_prepared_batch_device(eg_ctx*, size_t n, size_t terms, const void* d_scalars, const void* d_prepared, const void* d_r,
                                               void* d_scratch, void* d_out, void* stream);

/* ---- tally stage (examples/voting.rs:122-177) -------------------------------------------------------------------------------
 * Params::combine_shares (src/sharing/mod.rs:302-325, lagrange_coefficients :139-170): combines the FIRST `threshold` of the n given
 * decryption shares (zero-based participant indexes, dh elements of 32 bytes; verify them first: eg_share_params_create) into the
 * decryption [x]R of the shared key.  *combined = 0 (and EG_OK) when fewer than `threshold` shares are given (the reference
 * returns None); an index >= shares or a duplicate index is EG_ERR_BAD_ARG (the reference panics on the former).  All scalar and
 * group arithmetic runs on the GPU primitives. */
int eg_combine_shares(eg_ctx*, uint64_t shares, uint64_t threshold, size_t n, const uint64_t* indexes, const uint8_t* dh_elements,
                      uint8_t out[32], int* combined);
/* The same for a whole VECTOR of ciphertexts in one pass (csrc/share_combine_kernels.cuh): the step between "shares verified" and
 * "element handed to the discrete-log solver" for per-precinct tallies, which are 10^4 .. 10^5 ciphertexts where eg_combine_shares
 * opens one per call.  The k columns are participants: column j holds participant indexes[j]'s m items in the 128-byte layout that
 * eg_share_prove_batch writes and eg_verify_proof_batch reads (R || dh || challenge || response), item c belonging to ciphertext c, and
 * (optionally) the m status words the verify entry wrote for them - a caller verifies each participant's column into its slice of one
 * buffer and passes the buffers on without a copy.
 * PER CIPHERTEXT c the columns are walked in the caller's order.  Column j is usable when its status word is EG_ST_OK (d_status NULL:
 * every share counts as accepted) AND the first 32 bytes of its item equal the first 32 bytes of ciphertext c: a share proven for another
 * ciphertext is never combined into this one (the reference binds R through the `ciphertext` argument of verify_share).  The first
 * `threshold` usable columns are the shares (`.take(self.threshold)`); columns behind them are not looked at.  Fewer than `threshold`
 * usable columns: combined[c] = 0, 32 zero bytes in dh and plain, used[c] = 0 (the reference's None).  Otherwise
 * D = [scale] sum [denominator_j^-1] dh_j with the reference's signed denominators and scale, dh[c] = serialize(D),
 * plain[c] = serialize(B - D) - the element eg_dlog_solver_solve and eg_dlog_table_get take -, combined[c] = 1, and used[c] has bit
 * indexes[j] set for every share used.  Encodings are canonical, so the output is a function of the chosen shares alone and equals
 * eg_combine_shares + eg_point_add_batch on them byte for byte.
 * UNTRUSTED INPUTS.  The library WRITES the three words of `bad`: bad[0] = shares marked accepted, met on the walk, whose R bytes are
 * not the ciphertext's (skipped, the walk goes on); bad[1] = chosen shares whose dh does not decode; bad[2] = ciphertexts whose B does
 * not decode (counted only when d_plain is given).  For bad[1] and bad[2] the ciphertext gets combined = 0 and zero bytes; the call
 * still returns EG_OK.  Shares of columns that are not accepted are never decoded.  The host form returns EG_ERR_BAD_ARG when any word is
 * non-zero, AFTER writing its outputs.
 * EG_ERR_BAD_ARG before anything is launched: shares of 0 or above EG_COMBINE_SHARES_MAX, threshold outside 1..shares, k < 0 or k >
 * shares, an index >= shares, a duplicate index, m >= 2^31, a NULL d_ciphertexts / d_items / d_combined / d_bad / indexes with m > 0 (and
 * k > 0), NULL scratch when the size is not 0, buffers that are not 16-byte aligned (d_used: 8-byte).  k < threshold is valid: every
 * combined is 0.  m == 0 is valid.
 * STATELESS like the grouped tally: no lock, no workspace of the context, nothing allocated; the `_device` form is asynchronous on
 * `stream` and never synchronises with the host.  d_scratch holds eg_combine_shares_batch_scratch_bytes(threshold, m) bytes (0 for
 * arguments that would be refused; it stops growing at 2^17 ciphertexts, which longer vectors pass through one slab after the other).
 * The host form stages into device memory of its own and returns when the results are written; dh, plain and used may be NULL. */
#define EG_COMBINE_SHARES_MAX 64      /* participants of a key set the batch entries accept */
size_t eg_combine_shares_batch_scratch_bytes(uint64_t threshold, size_t m);
int eg_combine_shares_batch_device(eg_ctx*, uint64_t shares, uint64_t threshold, size_t m,
                                   const void* d_ciphertexts /* m x 64: R || B */,
                                   int k, const uint64_t* indexes /* HOST, k zero-based participant indexes */,
                                   const void* d_items /* k x m x 128, column j at j*m*128: R || dh || challenge || response */,
                                   const void* d_status /* k x m uint32, column j at j*m; NULL = every share accepted */,
                                   void* d_dh /* m x 32 or NULL */, void* d_plain /* m x 32 or NULL */,
                                   void* d_combined /* m bytes */, void* d_used /* m x uint64 or NULL */,
                                   void* d_bad /* 3 x uint32 */, void* d_scratch, void* stream);
int eg_combine_shares_batch(eg_ctx*, uint64_t shares, uint64_t threshold, size_t m, const uint8_t* ciphertexts,
                            int k, const uint64_t* indexes, const uint8_t* items, const uint32_t* status /* may be NULL */,
                            uint8_t* dh, uint8_t* plain, uint8_t* combined, uint64_t* used);
/* DiscreteLogTable (src/encryption.rs:260-298): new(values) computes [v]G for every non-zero value on the GPU; get() looks decrypted
 * elements up (found[i] = 0: not among the values; the identity is always 0).  The table itself lives in host memory. */
typedef struct eg_dlog_table eg_dlog_table;
int eg_dlog_table_create(eg_ctx*, size_t n, const uint64_t* values, eg_dlog_table** out);
void eg_dlog_table_destroy(eg_dlog_table*);
int eg_dlog_table_get(const eg_dlog_table*, size_t n, const uint8_t* elements /*32n*/, uint64_t* values, uint8_t* found);
/* The same answers for ranges that no table can hold (10^7 .. 2^48 values): DiscreteLogTable::new(lo..hi).get(e) by baby-step/giant-step
 * on the GPU (csrc/dlog_kernels.cuh).  A solver owns a table of 2^baby_bits multiples of the generator in device memory
 * (eg_dlog_solver_table_bytes: 16 bytes per entry; 0 = the default width, 24), built once; it is independent of any range.
 * eg_dlog_solver_solve answers n elements at once (n = the options of a tally): found[i] = 1 and values[i] = m iff some m in [lo, hi),
 * m != 0, has serialize([m]G) == element i.  The identity (32 zero bytes) is always (0, found), whatever lo - the rule of the reference
 * and of eg_dlog_table_get; an encoding that does not decode gives found = 0 and the call still returns EG_OK.  lo == hi is the empty
 * range, lo > hi is EG_ERR_BAD_ARG, hi may be 2^64 - 1.  The answer is exact: every candidate of the search is confirmed against the
 * element's bytes before it is reported.  A call takes time in proportion to n (hi - lo) / 2^baby_bits, so the span is bounded:
 * hi - lo above eg_dlog_solver_max_span(solver, n) is EG_ERR_BAD_ARG (raise baby_bits, or split the range) - the widest call admitted
 * takes about ten seconds.  Host pointers only; calls take the context's lock like every other entry. */
typedef struct eg_dlog_solver eg_dlog_solver;
int eg_dlog_solver_create(eg_ctx*, int baby_bits /* 0 = default; else 8..28 */, eg_dlog_solver** out);
void eg_dlog_solver_destroy(eg_dlog_solver*);
int eg_dlog_solver_solve(eg_dlog_solver*, size_t n, const uint8_t* elements /*32n*/, uint64_t lo, uint64_t hi, uint64_t* values,
                         uint8_t* found);
uint64_t eg_dlog_solver_max_span(const eg_dlog_solver*, size_t n); /* widest hi - lo a call with n elements accepts */
size_t eg_dlog_solver_table_bytes(const eg_dlog_solver*);

/* ---- batch tier: EncryptedChoice --------------------------------------------------------------------------------
 * wire layout of one ballot (stride = eg_choice_ballot_size):
 *   n_options x Ciphertext::to_bytes (R || B, encryption.rs:155-160)
 *   RingProof::to_bytes            (e0 || s_0 .. s_{2n-1}, ring.rs:383-392)
 *   LogEqualityProof::to_bytes     (c || s, log_equality.rs:184-189)      -- SingleChoice only */
int eg_choice_params_create(eg_ctx*, const uint8_t pk[32], int n_options, int single, eg_choice_params** out);
void eg_choice_params_destroy(eg_choice_params*);
size_t eg_choice_ballot_size(int n_options, int single);
/* EncryptedChoice::verify over a batch + homomorphic tally of the accepted ballots
 * (examples/voting.rs:199-203).  status: n words.
 * Tally semantics (the same for the host and the `_device` forms, and for eg_verify_qv_batch): every call ADDS the
 * ciphertexts of the ballots it accepts to the running tally kept inside `params`; only eg_*_tally_reset clears the running
 * tally, eg_*_tally_add imports into it, eg_*_tally_encode reads it.  tally_out (may be NULL) additionally receives the tally
 * of THIS call's batch alone, n_options x 64 bytes (R || B); it never disturbs the running tally. */
int eg_verify_choice_batch(eg_choice_params*, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out);
/* device-resident variant: d_ballots / d_status are device pointers; the running tally stays on the device
 * inside `params` until eg_choice_tally_* is called.  Asynchronous on `stream` (internally the work forks onto two streams of the
 * params object and joins `stream` again before the call returns control of it), with TWO exceptions that block the host once:
 *  - the first call of a params object (and any later call with a larger batch) allocates the chunk workspace
 *    (hipDeviceSynchronize + hipMalloc; ~45 KB per ballot of a chunk for 5 options, two chunks of up to 2^19 ballots);
 *  - the call with which a params object has seen 2^19 ballots in total builds the WIDE fixed-base comb tables inline: about
 *    12 GB each for the generator (once per context) and the election key (once per params object), ~40 ms, with a
 *    hipStreamSynchronize on `stream`.  A host that needs strict asynchrony (or wants the memory accounted for up front) calls
 *    eg_choice_prepare_wide_tables / eg_qv_prepare_wide_tables right after creating the params; EG_COMB_BIG_BITS=0 switches the
 *    wide tables off (-1..2 % throughput).  If the wide tables do not fit the device memory the narrow ones stay in use. */
int eg_verify_choice_batch_device(eg_choice_params*, size_t n, const void* d_ballots, void* d_status, void* stream);
/* builds the wide comb tables now (synchronous); EG_ERR_NOMEM if they do not fit, EG_OK when they exist or are switched off */
int eg_choice_prepare_wide_tables(eg_choice_params*);
int eg_choice_tally_reset(eg_choice_params*);
int eg_choice_tally_encode(eg_choice_params*, uint8_t* out /* n_options*64 */);
/* running tally += the ciphertexts encoded in `in` (n_options*64 bytes, as eg_choice_tally_encode writes them): resume
 * from a checkpoint, or merge the tally of batches verified elsewhere.  EG_ERR_BAD_ARG (and slots with invalid encodings
 * untouched) if an encoding does not decode. */
int eg_choice_tally_add(eg_choice_params*, const uint8_t* in /* n_options*64 */);
/* asynchronous forms for the multi-GPU path: reset on a stream; write the canonical encodings (n_options*64 bytes)
 * to device memory, ready for an RCCL all-gather; then sum the gathered encodings with eg_points_sum_device. */
int eg_choice_tally_reset_async(eg_choice_params*, void* stream);
int eg_choice_tally_encode_device(eg_choice_params*, void* d_out, void* stream);
/* d_out[k] = encode( sum_r decode(d_in[r][k]) ), k < n_points, r < n_ranks; 32-byte encodings.  d_bad (device uint32, may be
 * NULL; the caller zeroes it) is incremented once per point slot that received an encoding which does not decode: such a
 * term contributes the identity, so a caller merging tallies from other ranks must treat *d_bad != 0 as a failed exchange. */
int eg_points_sum_device(eg_ctx*, int n_ranks, int n_points, const void* d_in, void* d_out, void* d_bad, void* stream);

/* ---- batch tier: QuadraticVotingBallot ------------------------------------------------------------------------------
 * wire layout (stride = eg_qv_ballot_size), serde field order of quadratic_voting.rs:205-217 / range.rs:446-450 /
 * mul.rs:86-93:
 *   n_options x [ ciphertext(64) || partial_ciphertexts(64 each) || common_challenge(32) || ring_responses ]
 *   credit:      [ ciphertext(64) || partial_ciphertexts          || common_challenge     || ring_responses ]
 *   SumOfSquaresProof: challenge(32) || ciphertext_responses(2n x 32) || sum_response(32) */
int eg_qv_params_create(eg_ctx*, const uint8_t pk[32], int n_options, uint64_t credits, eg_qv_params** out);
void eg_qv_params_destroy(eg_qv_params*);
size_t eg_qv_ballot_size(const eg_qv_params*);
int eg_verify_qv_batch(eg_qv_params*, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out);
int eg_verify_qv_batch_device(eg_qv_params*, size_t n, const void* d_ballots, void* d_status, void* stream);
int eg_qv_prepare_wide_tables(eg_qv_params*);      /* as eg_choice_prepare_wide_tables */
int eg_qv_tally_reset(eg_qv_params*);
int eg_qv_tally_encode(eg_qv_params*, uint8_t* out);
int eg_qv_tally_add(eg_qv_params*, const uint8_t* in);
int eg_qv_tally_reset_async(eg_qv_params*, void* stream);
int eg_qv_tally_encode_device(eg_qv_params*, void* d_out, void* stream);

/* ---- small-batch tier: a handful of ballots with low latency ---------------------------------------------------------------
 * The batch entries chain about twenty kernels with one lane per group equation: whatever the batch, a call takes the ~2 ms of one
 * lane's dependent chain.  The _small entries verify each ballot in ONE workgroup of ONE launch, with four lanes per point
 * operation.  Arguments, status words, error precedence, the running tally, tally_out, locking and the refusal while a JSON stream is
 * open are those of eg_verify_*_batch[_device]; n == 0 is EG_OK, n > EG_SMALL_BATCH_MAX is EG_ERR_BAD_ARG.  They work for every election
 * shape the batch entries accept.  Measured crossover (profiles/r09_small_batch.txt, device-resident ballots, call + synchronize,
 * small entry against batch entry): choice ballots - up to 1 024 ballots per call use the _small entry, above it the batch entry
 * (5 options, single choice: 1.09 against 2.13 ms for one ballot, 1.21 against 2.03 for 256, 1.30 against 2.07 for 1 024, 4.44 against
 * 2.11 for 4 096; 3-of-16 multi-choice 1.05 against 2.53 for one, 2.24 against 2.41 for 1 024, 8.28 against 3.23 for 4 096);
 * quadratic-voting ballots - up to 256 per call use the _small entry (3.58 against 6.09 ms for one, 3.94 against 5.76 for 256, 8.27
 * against 5.86 for 1 024).  One workgroup per ballot is sized for latency, not for throughput.  One ballot is faster through the
 * _small entry than on one CPU core of the same host (1.09 against 1.25 ms, the reference-equivalent CPU verifier). */
#define EG_SMALL_BATCH_MAX 4096   /* the flat part of the batch path's latency curve, DESIGN.md section 6 */
int eg_verify_choice_small(eg_choice_params*, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out);
int eg_verify_choice_small_device(eg_choice_params*, size_t n, const void* d_ballots, void* d_status, void* stream);
int eg_verify_qv_small(eg_qv_params*, size_t n, const uint8_t* ballots, uint32_t* status, uint8_t* tally_out);
int eg_verify_qv_small_device(eg_qv_params*, size_t n, const void* d_ballots, void* d_status, void* stream);

/* ---- per-group tally: the accepted ballots of a verified batch, summed by precinct / district / ballot box in one pass ------------
 * The verify entries add every accepted ballot into ONE tally (examples/voting.rs:199-203); an election that publishes results per
 * precinct needs one tally per precinct.  These entries run AFTER a verify entry, over the same packed ballots and the status words it
 * wrote: tallies[g] (n_options x 64 bytes, R || B per option, canonical encodings) is what eg_*_tally_encode would give after verifying
 * only the ballots with groups[b] == g - the sum over the ballots with status[b] == 0 - and 64 zero bytes per option (Ciphertext::zero())
 * for a group without an accepted ballot; counts[g] (optional) = accepted ballots of group g.  groups[b] == EG_GROUP_NONE leaves ballot b
 * out of every group (the spoiled pile, another election's ballots).  Only the ciphertext points are needed, and they are decoded again
 * from the wire bytes (2 n_options decodings per accepted ballot), so the pass is STATELESS: it reads nothing of the params object but its
 * immutable plan, touches no running tally and no workspace, takes no lock, and may run from any thread and on any stream beside verify
 * calls and open JSON streams of the same params object.  The same verified batch may be tallied again under another grouping
 * (precinct, then county) without verifying again.  Results do not depend on the order of the ballots.
 *
 * UNTRUSTED INPUTS.  Every group id is bounds-checked before it indexes anything.  The library WRITES the two words of `bad` (it does
 * not add to them): bad[0] = accepted ballots whose id is >= n_groups and not EG_GROUP_NONE (left out of every group); bad[1] = tally
 * points of accepted ballots that do not decode - the status words were forged or belong to other ballots; such a point contributes the
 * identity, as in eg_points_sum_device.  If either is non-zero the tallies are to be discarded; the host form then returns
 * EG_ERR_BAD_ARG.  Ids and points of REJECTED ballots are never looked at.
 * EG_ERR_BAD_ARG before anything is launched: n_groups == 0 or above EG_TALLY_GROUPS_MAX, n >= 2^31, a NULL d_ballots / d_status /
 * d_groups / d_tallies / d_bad with n > 0, a NULL scratch pointer when the scratch size is not 0, ballots or scratch that are not
 * 16-byte aligned.  n == 0 is valid: all-zero tallies.
 *
 * The `_device` form is asynchronous on `stream`, allocates nothing and never synchronises with the host; d_scratch is the caller's,
 * eg_*_tally_grouped_scratch_bytes(params, n, n_groups) bytes (the convention of eg_msm_scratch_bytes_ctx; 0 for arguments that would be
 * refused): 4 bytes per ballot, ~36 per group and the partial sums, 144 bytes x 2 n_options x (n / 32 + min(n, n_groups)) and a
 * thirty-second of that again.  The host form stages its buffers in device memory of its own and returns when the results are written.
 * MERGING.  Grouped tallies of several calls, slabs or ranks are merged with eg_points_sum_device(ctx, n_parts, n_groups * 2 *
 * n_options, ...), counts by plain addition: no new collective. */
#define EG_GROUP_NONE 0xffffffffu
#define EG_TALLY_GROUPS_MAX (1u << 24)
size_t eg_choice_tally_grouped_scratch_bytes(const eg_choice_params*, size_t n, uint32_t n_groups);
int eg_choice_tally_grouped_device(eg_choice_params*, size_t n, const void* d_ballots, const void* d_status, const void* d_groups,
                                   uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_counts /* may be NULL */,
                                   void* d_bad /* 2 x uint32 */, void* stream);
int eg_choice_tally_grouped(eg_choice_params*, size_t n, const uint8_t* ballots, const uint32_t* status, const uint32_t* groups,
                            uint32_t n_groups, uint8_t* tallies, uint32_t* counts /* may be NULL */);
size_t eg_qv_tally_grouped_scratch_bytes(const eg_qv_params*, size_t n, uint32_t n_groups);
int eg_qv_tally_grouped_device(eg_qv_params*, size_t n, const void* d_ballots, const void* d_status, const void* d_groups,
                               uint32_t n_groups, void* d_scratch, void* d_tallies, void* d_counts /* may be NULL */,
                               void* d_bad /* 2 x uint32 */, void* stream);
int eg_qv_tally_grouped(eg_qv_params*, size_t n, const uint8_t* ballots, const uint32_t* status, const uint32_t* groups,
                        uint32_t n_groups, uint8_t* tallies, uint32_t* counts /* may be NULL */);

/* ---- weighted per-group tally: every accepted ballot counts with a weight of its own (shares, stake, delegated votes) ----------------
 * The reference's Ciphertext has scalar multiplication beside Add and Sub (impl Mul<u64>, src/encryption.rs:197-215); a host that holds
 * one ballot per voter weights votes with `total += ballot.ciphertext * w`.  These entries are the per-group tally above with that
 * product inside: tallies[g][t] = the canonical encoding of the sum of [weights[b]] x (tally point t of ballot b) over the ballots with
 * status[b] == 0, groups[b] == g and weights[b] < 2^weight_bits; 32 zero bytes for an empty sum.  The layout is the grouped entry's.  With
 * every weight 1 the output is byte for byte that of eg_*_tally_grouped.  A weight of 0 is valid: the ballot counts in counts[g] and adds
 * nothing.  groups == NULL puts every ballot into group 0 (n_groups must then be 1).
 * weight_bits (1..64) is the caller's bound on the bit length of a weight.  It fixes the length of every lane's doubling chain for the
 * whole call - 16-bit weights cost 16 doublings per point, not 64 - so it should be as small as the weights allow.
 * weight_sums[g] (optional, two uint64 per group: low word, high word) = the exact sum of the counted weights of group g.  No tally
 * counter can exceed it: it is the upper bound to hand to eg_dlog_solver_solve when the totals are decrypted.  counts[g] as above.
 *
 * UNTRUSTED INPUTS.  The library WRITES the three words of `bad`: bad[0] and bad[1] as in the grouped entry; bad[2] = accepted ballots
 * with a group id in range whose weight is 2^weight_bits or more (never with weight_bits == 64).  Such a ballot is left out of tallies,
 * counts and weight sums alike.  If any word is non-zero the results are to be discarded; the host form then returns EG_ERR_BAD_ARG.
 * Ids and weights of REJECTED ballots are never read.
 * EG_ERR_BAD_ARG before anything is launched: everything the grouped entry refuses, weight_bits outside 1..64, NULL weights with n > 0,
 * NULL groups with n_groups != 1, weights or weight sums that are not 8-byte aligned.  n == 0 is valid: all-zero tallies, sums, counts.
 *
 * STATELESS as the grouped pass: the params object's immutable plan only - no lock, no workspace, no running tally.  The `_device`
 * form is asynchronous on `stream` and allocates nothing; d_scratch holds eg_*_tally_weighted_scratch_bytes(params, n, n_groups) bytes
 * (0 for arguments that would be refused): the grouped pass's scratch and 16 bytes per partial sum of slot 0 for the weight sums.
 * MERGING.  Weighted tallies of slabs or ranks merge with eg_points_sum_device like grouped ones, weight sums and counts by addition. */
size_t eg_choice_tally_weighted_scratch_bytes(const eg_choice_params*, size_t n, uint32_t n_groups);
int eg_choice_tally_weighted_device(eg_choice_params*, size_t n, const void* d_ballots, const void* d_status,
                                    const void* d_weights /* n x uint64 */, int weight_bits /* 1..64 */,
                                    const void* d_groups /* NULL: every ballot in group 0, n_groups must be 1 */, uint32_t n_groups,
                                    void* d_scratch, void* d_tallies, void* d_weight_sums /* n_groups x 2 x uint64 (low, high), may be NULL */,
                                    void* d_counts /* may be NULL */, void* d_bad /* 3 x uint32 */, void* stream);
int eg_choice_tally_weighted(eg_choice_params*, size_t n, const uint8_t* ballots, const uint32_t* status, const uint64_t* weights,
                             int weight_bits, const uint32_t* groups /* may be NULL */, uint32_t n_groups, uint8_t* tallies,
                             uint64_t* weight_sums /* may be NULL */, uint32_t* counts /* may be NULL */);
size_t eg_qv_tally_weighted_scratch_bytes(const eg_qv_params*, size_t n, uint32_t n_groups);
int eg_qv_tally_weighted_device(eg_qv_params*, size_t n, const void* d_ballots, const void* d_status,
                                const void* d_weights /* n x uint64 */, int weight_bits /* 1..64 */,
                                const void* d_groups /* NULL: every ballot in group 0, n_groups must be 1 */, uint32_t n_groups,
                                void* d_scratch, void* d_tallies, void* d_weight_sums /* n_groups x 2 x uint64 (low, high), may be NULL */,
                                void* d_counts /* may be NULL */, void* d_bad /* 3 x uint32 */, void* stream);
int eg_qv_tally_weighted(eg_qv_params*, size_t n, const uint8_t* ballots, const uint32_t* status, const uint64_t* weights,
                         int weight_bits, const uint32_t* groups /* may be NULL */, uint32_t n_groups, uint8_t* tallies,
                         uint64_t* weight_sums /* may be NULL */, uint32_t* counts /* may be NULL */);

/* ---- ballot weeding: accepted ballots that repeat a ciphertext of the bulletin board or of an earlier ballot, flagged in one pass --------
 * The reference's transcripts start from fixed labels and bind the key and the ciphertexts (src/app/choice.rs:72,323,376), nothing of
 * the voter: a byte-for-byte copy of somebody's ballot verifies and would be tallied, and the change in the result reveals the copied
 * vote (Cortier and Smyth, "Attacking and fixing Helios").  These entries run between a verify entry and a tally entry, over the same
 * packed ballots, and say which ballots to drop.
 * KEYS.  A ballot's keys are its tally ciphertexts, the 64 wire bytes R || B behind each pair of tally slots: n_options of them (for
 * quadratic voting the vote ciphertexts; partial ciphertexts and the credit ciphertext are not keys).  Equality is byte equality - accepted
 * ballots have canonical encodings - and nothing is decoded.  Ballot b PARTICIPATES iff status[b] == EG_ST_OK (d_status NULL: every
 * ballot); bytes of other ballots are never read.  The BOARD is the caller's compact array of ciphertexts cast in earlier batches:
 * n_prior x 64 bytes in a buffer with room for board_cap.
 * THE RULE.  dup_of[b] = EG_DUP_NONE for a ballot that does not participate or shares no key; EG_DUP_PRIOR if any key of b is on the
 * board; otherwise the smallest index b' < b of a participating ballot that shares at least one key with b, at any option position.
 * The rule is NOT sequential: b' counts even if b' is itself flagged - A{x,y}, B{y,z}, C{z,w} flags B (0) and C (1) - so the verdict is a
 * pure function of the inputs that depends neither on hash_seed nor on the order in which lanes run.  Honest ballots never share a
 * ciphertext, so only adversarial ballots can tell this from the sequential rule.  The same key twice inside one ballot is no duplicate.
 * status_out (optional, may be d_status itself) = status[b], or EG_ST_DUPLICATE for a flagged ballot: the words to hand to
 * eg_*_tally_grouped / _weighted.  The library WRITES found[0] = ballots flagged against the board, found[1] = ballots flagged against
 * the batch, found[2] = the bad word: non-zero if the table overflowed (it cannot with the library's own sizing; the probe loop is
 * bounded and reports instead of spinning) or if the append below did not fit - discard the results then.
 * APPEND (d_board_count != NULL).  The keys of every participating, unflagged ballot are written behind the first n_prior entries, in
 * ballot order and then option order, and *d_board_count (uint64) = n_prior + appended.  If they do not fit board_cap nothing is
 * appended, the count is n_prior and found[2] is set.
 * hash_seed: 64 bits the caller draws at random per call and does not publish before the call is over (the host form draws its own).
 * The ballots are untrusted: under a public hash, valid ballots with keys on one probe chain would make the pass quadratic.
 *
 * STATELESS as the grouped pass: the params object's immutable plan only - no lock, no workspace, no running tally.  The `_device` form
 * is asynchronous on `stream`, allocates nothing and never synchronises; d_scratch holds eg_*_weed_scratch_bytes(params, n, n_prior)
 * bytes (0 for arguments that would be refused, and for n == 0): 8 bytes per slot of a table of the smallest power of two >= 2 (n
 * n_options + n_prior), at least 1024, and ~4 bytes per ballot.  The host form returns EG_ERR_BAD_ARG AFTER writing its outputs when
 * found[2] != 0; appended (optional, room for n x n_options x 64 bytes) receives the appended keys and *n_appended their number.
 * EG_ERR_BAD_ARG before anything is launched: n >= 2^31, n_prior >= 2^31, n n_options + n_prior above EG_WEED_KEYS_MAX, n_prior >
 * board_cap, a NULL d_ballots / d_dup_of / d_found with n > 0, a NULL d_board with n_prior > 0 or with an append requested, a NULL
 * scratch pointer when the size is not 0, ballots, board or scratch that are not 16-byte aligned.  n == 0 is valid. */
#define EG_DUP_NONE 0xffffffffu
#define EG_DUP_PRIOR 0xfffffffeu
#define EG_WEED_KEYS_MAX (1u << 30) /* n * keys_per_ballot + n_prior */
size_t eg_choice_weed_scratch_bytes(const eg_choice_params*, size_t n, size_t n_prior);
int eg_choice_weed_device(eg_choice_params*, size_t n, const void* d_ballots, const void* d_status /* or NULL */, size_t n_prior,
                          void* d_board /* board_cap x 64 */, size_t board_cap, uint64_t hash_seed, void* d_scratch,
                          void* d_dup_of /* n x uint32 */, void* d_status_out /* or NULL */,
                          void* d_board_count /* uint64, or NULL: no append */, void* d_found /* 3 x uint32 */, void* stream);
int eg_choice_weed(eg_choice_params*, size_t n, const uint8_t* ballots, const uint32_t* status /* or NULL */, size_t n_prior,
                   const uint8_t* board, uint32_t* dup_of, uint32_t* status_out /* or NULL */,
                   uint8_t* appended /* or NULL; room for n * n_options * 64 */, size_t* n_appended);
size_t eg_qv_weed_scratch_bytes(const eg_qv_params*, size_t n, size_t n_prior);
int eg_qv_weed_device(eg_qv_params*, size_t n, const void* d_ballots, const void* d_status /* or NULL */, size_t n_prior,
                      void* d_board /* board_cap x 64 */, size_t board_cap, uint64_t hash_seed, void* d_scratch,
                      void* d_dup_of /* n x uint32 */, void* d_status_out /* or NULL */,
                      void* d_board_count /* uint64, or NULL: no append */, void* d_found /* 3 x uint32 */, void* stream);
int eg_qv_weed(eg_qv_params*, size_t n, const uint8_t* ballots, const uint32_t* status /* or NULL */, size_t n_prior,
               const uint8_t* board, uint32_t* dup_of, uint32_t* status_out /* or NULL */,
               uint8_t* appended /* or NULL; room for n * n_options * 64 */, size_t* n_appended);

/* ---- weeding against a persistent board index: the board's table kept between batches ---------------------------------------------------
 * eg_*_weed_device clears a table for n n_options + n_prior keys and re-inserts the whole board in every call: O(board) time and scratch
 * per batch.  A board that takes batches all day keeps the table instead.  The BOARD INDEX is the open-addressing table over the board's
 * ciphertexts, held by the caller in device memory between calls like the roll and the node store: eg_weed_index_bytes(board_cap) bytes,
 * 4 per slot of a table of the smallest power of two >= 2 board_cap, at least 1024 (0 for board_cap >= 2^31).  A slot holds a board
 * position (below 2^31) or all ones for empty; equal bytes at two board positions share a slot that holds the smaller position.
 *   eg_weed_index_build_device   clears the index and inserts board entries [0, n_prior) (n_prior == 0: an empty index): start-up,
 *                                restoring from an archive, after board_cap has grown, re-seeding.  WRITES found[0] (one uint32) =
 *                                non-zero if the index overflowed (it cannot with the library's own sizing).
 *   eg_weed_index_find_device    read-only: pos[q] = the smallest board position that holds the 64 bytes of key q, or EG_DUP_NONE - "is
 *                                this ciphertext on the board", for a spoil check or a voter.
 *   eg_*_weed_indexed_device     the arguments of eg_*_weed_device plus d_index and index_seed; hash_seed stays the fresh per-call seed of
 *                                the table of the batch's own keys.  dup_of, status_out (may alias d_status), found[0..2], *d_board_count
 *                                and the appended board bytes are BYTE FOR BYTE those of eg_*_weed_device over the same ballots, status
 *                                words and board, under the rule above.  With an append that fits, the index afterwards covers board
 *                                [0, *d_board_count).  If the append does not fit, found[2] is set, the count is n_prior and neither the
 *                                board nor a byte of the index changes.  With d_board_count == NULL the index is only read.  found[2] is
 *                                also set if the index overflows while adding (it cannot with the library's own sizing: the append check
 *                                holds the load at or below 0.5); the caller then rebuilds the index.
 * d_scratch holds eg_*_weed_indexed_scratch_bytes(params, n) bytes, a function of n alone: the table of the batch's n n_options keys (8
 * bytes per slot) and ~4 bytes per ballot.  The cost of a call is O(batch).
 * CONTRACT.  The index was built and maintained over exactly board [0, n_prior) with this board_cap and this index_seed.  One writer at a
 * time per index (build, or an indexed pass with an append); the read-only forms (find, an indexed pass without an append) may run
 * concurrently with each other.  index_seed stays unpublished for the LIFE OF THE INDEX, not for one call; build with a fresh seed
 * re-seeds at O(board) whenever the host wishes.  Under a wrong or garbage index the verdicts are undefined, but every probe loop is
 * bounded by the slot count and no reference at or above n_prior is ever dereferenced.  Nothing is ever removed from an index, and it
 * does not grow past board_cap: allocate a larger one and build.  Each GPU keeps its own index over its copy of the board.
 * EG_ERR_BAD_ARG before anything is launched: what eg_*_weed_device refuses; a NULL index; an index, keys, board, ballots or scratch that
 * are not 16-byte aligned; board_cap >= 2^31; n n_options above EG_WEED_KEYS_MAX (the board no longer counts against that limit); for
 * find, n_q >= 2^31 and NULL keys or pos with n_q > 0.  There are no host-buffer forms: a host that holds its board in host memory has
 * eg_*_weed. */
size_t eg_weed_index_bytes(size_t board_cap);
int eg_weed_index_build_device(eg_ctx*, size_t n_prior, const void* d_board /* board_cap x 64 */, size_t board_cap, uint64_t index_seed,
                               void* d_index, void* d_found /* 1 x uint32: overflow */, void* stream);
int eg_weed_index_find_device(eg_ctx*, size_t n_q, const void* d_keys /* n_q x 64 */, size_t n_prior, const void* d_board, size_t board_cap,
                              const void* d_index, uint64_t index_seed, void* d_pos /* n_q x uint32 */, void* stream);
size_t eg_choice_weed_indexed_scratch_bytes(const eg_choice_params*, size_t n);
int eg_choice_weed_indexed_device(eg_choice_params*, size_t n, const void* d_ballots, const void* d_status /* or NULL */, size_t n_prior,
                                  void* d_board /* board_cap x 64 */, size_t board_cap, void* d_index, uint64_t index_seed,
                                  uint64_t hash_seed, void* d_scratch, void* d_dup_of /* n x uint32 */, void* d_status_out /* or NULL */,
                                  void* d_board_count /* uint64, or NULL: no append, the index is only read */,
                                  void* d_found /* 3 x uint32 */, void* stream);
size_t eg_qv_weed_indexed_scratch_bytes(const eg_qv_params*, size_t n);
int eg_qv_weed_indexed_device(eg_qv_params*, size_t n, const void* d_ballots, const void* d_status /* or NULL */, size_t n_prior,
                              void* d_board /* board_cap x 64 */, size_t board_cap, void* d_index, uint64_t index_seed, uint64_t hash_seed,
                              void* d_scratch, void* d_dup_of /* n x uint32 */, void* d_status_out /* or NULL */,
                              void* d_board_count /* uint64, or NULL: no append, the index is only read */,
                              void* d_found /* 3 x uint32 */, void* stream);

/* ---- ballot audits (the Benaloh challenge): opened ballots re-encrypted and compared in one pass ---------------------------------------
 * The reference's proofs show that a ballot encrypts SOME admissible value.  A voting device that encrypts option 2 when the voter pressed
 * option 4 passes every stage of the chain.  Helios, and with guardians in place of the device ElectionGuard, let the voter CHALLENGE the
 * device before casting: it opens the ballot it has just committed to - reveals the value and the encryption randomness of every
 * ciphertext -, anyone re-encrypts and compares, and the opened ballot is SPOILED, never counted.  Boards publish these openings in bulk;
 * these entries re-check a pile of them.
 * INPUTS.  A ballot's SLOTS are its tally ciphertexts in tally order, exactly the keys of weeding: n_options of them (for quadratic voting
 * the vote ciphertexts; partial ciphertexts and the credit ciphertext are not opened).  An OPENING of ballot b is, per slot t, a value
 * values[b n_slots + t] (uint64) and the 32 bytes rand[(b n_slots + t) 32 ..] of a scalar r, little-endian.  Ballot b PARTICIPATES iff
 * status_in[b] == EG_ST_OK (status_in NULL: every ballot).  The bytes of other ballots and of their openings are never read, and their
 * status word is handed on.
 * THE RULE.  For a participating ballot, in slot order and within a slot in this order:
 *   EG_OPEN_BAD_SCALAR 1  r is not a canonical scalar, r >= l.  ([r + l]G and [r]G have the same encoding: without this check an opening
 *                         could be published in two forms.)
 *   EG_OPEN_R          2  the canonical Ristretto encoding of [r]G is not the 32 wire bytes R of the slot
 *   EG_OPEN_B          3  the encoding of [v]G + [r]K is not the wire bytes B
 * The comparison is byte equality.  Nothing of the ballot is decoded, so a non-canonical or invalid wire encoding is simply a mismatch.
 * The FIRST failure wins: status_out[b] = EG_ST_BAD_OPENING | EG_OPEN_DETAIL(slot, check) << 8, and EG_ST_OK otherwise.  status_out may be
 * status_in itself.  The library WRITES found[0] = ballots that participated, found[1] = ballots that failed.  The verdict is a pure
 * function of the inputs.  v is any uint64: the pass says what the ballot opens to, not whether that value is admissible - that is the
 * verify entry's job.  r = 0 and v = 0 are valid; the identity encodes as 32 zero bytes.
 * SPOILING.  The randomness of an opened ballot is public, so it must never be counted, whatever its verdict.  The recipe needs no entry
 * of its own: put the 64-byte keys R || B of every audited ballot onto weeding's board as prior entries (run eg_*_weed over the audited
 * pile with an append, or copy the keys); a later ballot that re-uses an opened ciphertext is then flagged EG_DUP_PRIOR by eg_*_weed.
 * examples/voting.cpp --audits does this.
 *
 * STATELESS as weeding: the params object's immutable plan and the narrow comb tables of G and K only - no lock, no workspace, no running
 * tally, no wide tables, any stream, beside a verifying thread.  The `_device` form is asynchronous on `stream`, allocates nothing and
 * never synchronises; d_scratch holds eg_*_open_check_scratch_bytes(params, n) bytes (0 for arguments that would be refused, and for
 * n == 0): 4 bytes per (ballot, slot).  The host form is the same on host arrays, synchronous, with its own scratch.
 * EG_ERR_BAD_ARG before anything is launched: n >= 2^31; a NULL ballots / values / rand / status_out / found with n > 0; ballots or scratch
 * that are not 16-byte aligned, values not 8-byte aligned, rand, status_in, status_out or found not 4-byte aligned (device form); NULL
 * params; n x n_slots above EG_OPEN_ITEMS_MAX; a NULL scratch pointer when the size is not 0.  n == 0 is valid: found (where given) is
 * zero. */
enum { EG_OPEN_BAD_SCALAR = 1, EG_OPEN_R = 2, EG_OPEN_B = 3 };                  /* the check that failed */
#define EG_OPEN_DETAIL(slot, check) ((uint32_t)(slot) * 4u + (uint32_t)(check))    /* detail of EG_ST_BAD_OPENING */
#define EG_OPEN_DETAIL_SLOT(detail) ((detail) >> 2)
#define EG_OPEN_DETAIL_CHECK(detail) ((detail) & 3u)
#define EG_OPEN_ITEMS_MAX (1u << 31) /* n * n_slots */
size_t eg_choice_open_check_scratch_bytes(const eg_choice_params*, size_t n);
int eg_choice_open_check_device(eg_choice_params*, size_t n, const void* d_ballots, const void* d_status_in /* uint32[n] or NULL */,
                                const void* d_values /* uint64[n x n_options] */, const void* d_rand /* n x n_options x 32 */,
                                void* d_status_out /* uint32[n] */, void* d_found /* 2 x uint32 */, void* d_scratch, void* stream);
int eg_choice_open_check(eg_choice_params*, size_t n, const uint8_t* ballots, const uint32_t* status_in /* or NULL */,
                         const uint64_t* values, const uint8_t* rand, uint32_t* status_out, uint32_t* found /* 2 */);
size_t eg_qv_open_check_scratch_bytes(const eg_qv_params*, size_t n);
int eg_qv_open_check_device(eg_qv_params*, size_t n, const void* d_ballots, const void* d_status_in /* uint32[n] or NULL */,
                            const void* d_values /* uint64[n x n_options] */, const void* d_rand /* n x n_options x 32 */,
                            void* d_status_out /* uint32[n] */, void* d_found /* 2 x uint32 */, void* d_scratch, void* stream);
int eg_qv_open_check(eg_qv_params*, size_t n, const uint8_t* ballots, const uint32_t* status_in /* or NULL */, const uint64_t* values,
                     const uint8_t* rand, uint32_t* status_out, uint32_t* found /* 2 */);

/* ---- voter signatures: Ed25519 (RFC 8032, pure EdDSA) of a batch checked in one pass ------------------------------------------------
 * The reference's proofs bind nothing of the voter: a fresh, valid ballot cast by someone who is not on the roll, or in another voter's
 * name, verifies.  A deployment wraps the ballot in a signature under a registered voter key; this pass checks those signatures where
 * the ballots already are.  Ed25519 lives on the engine's curve: the Ristretto generator is the Ed25519 base point B.
 *
 * THE RULE.  For item b the message is M_b = prefix || msg_b: `prefix` is 0..255 bytes, one per call (domain separation: the election
 * id); msg_b is msg_len bytes at msgs + b * msg_stride (a packed ballot buffer is passed as it is, msg_stride = msg_len = ballot size).
 * The key is A_b = keys[b] when key_index is NULL, else keys[key_index[b]] out of a roster of n_keys keys (the voter id selects the
 * registered key; a signature counts only under that key).  The signature is sig_b = R(32) || S(32).  The checks run in this order,
 * the first failure wins, and every failure is status EG_ST_BAD_SIGNATURE with the detail in EG_STATUS_DETAIL:
 *   EG_ED25519_BAD_INDEX   5  key_index[b] >= n_keys
 *   EG_ED25519_BAD_S       1  S is not canonical (S >= l)
 *   EG_ED25519_BAD_KEY     2  A does not decode (RFC 8032 5.1.3, STRICT: y >= p is refused, x = 0 with the sign bit set is refused,
 *                             no square root is refused)
 *   EG_ED25519_SMALL_ORDER 3  [8]A is the identity
 *   EG_ED25519_MISMATCH    4  with h = SHA-512(R || A || M_b) mod l and R' = [S]B - [h]A, the RFC 8032 5.1.2 encoding of R' differs from
 *                             the 32 bytes R
 * R is never decoded, so a non-canonical R can never match; a small-order R is not separately refused.  This is the COFACTORLESS byte
 * comparison that OpenSSL makes (not the cofactored equation [8][S]B = [8]R + [8][h]A that RFC 8032 also allows), so the verdict of
 * every item is that of a one-by-one check: no random linear combination, no batch equation.
 * status_in (optional): a lane whose word is not 0 does nothing and hands the word on, status_out[b] = status_in[b] - the pass chains
 * with verify, weeding and the tallies in either order; none of that item's bytes are read.  status_out may be status_in itself.
 *
 * TIMING: variable time throughout.  The verifier sees public data only.  The SIGNER (eg_ed25519_keypair_*, eg_ed25519_sign_*) is a maker
 * of test and benchmark items like the provers: its branches and table lookups depend on the secret scalar - it is not for a voter client.
 * Ed25519 is deterministic, so the signer reproduces the bytes of any RFC 8032 signer (seed(32) -> SHA-512 -> clamp -> A = [a]B;
 * r = SHA-512(hash prefix || M) mod l; R = [r]B; S = r + h a mod l).
 *
 * eg_ed25519_verify_device is asynchronous on `stream`, allocates nothing, never synchronises and takes no lock; `prefix` is HOST memory
 * and is copied during the call; d_scratch holds eg_ed25519_verify_scratch_bytes(ctx, n) bytes (h of every item and the lanes' tables
 * of -A, sized by the grid).  d_keys, d_sigs, d_key_index and the status arrays must be 4-byte aligned; the messages may lie anywhere.
 * Refused with EG_ERR_BAD_ARG before anything is launched: NULL mandatory pointers with n > 0, prefix_len > 255, a NULL prefix with
 * prefix_len > 0, msg_stride < msg_len, n >= 2^31, n_keys == 0 with n > 0, key_index == NULL with n_keys != n, a scratch that is too
 * small.  n == 0 is EG_OK.  eg_ed25519_verify_batch: the same on host buffers, synchronous, with its own scratch. */
enum { EG_ED25519_BAD_S = 1, EG_ED25519_BAD_KEY = 2, EG_ED25519_SMALL_ORDER = 3, EG_ED25519_MISMATCH = 4, EG_ED25519_BAD_INDEX = 5 };
size_t eg_ed25519_verify_scratch_bytes(const eg_ctx*, size_t n);
int eg_ed25519_verify_device(eg_ctx*, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix /* host */,
                             size_t prefix_len, const void* d_keys /* n_keys x 32 */, size_t n_keys,
                             const void* d_key_index /* uint32[n] or NULL */, const void* d_sigs /* n x 64 */,
                             const void* d_status_in /* uint32[n] or NULL */, void* d_status_out /* uint32[n] */, void* d_scratch,
                             size_t scratch_bytes, void* stream);
int eg_ed25519_verify_batch(eg_ctx*, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix,
                            size_t prefix_len, const uint8_t* keys /* n_keys x 32 */, size_t n_keys,
                            const uint32_t* key_index /* n or NULL */, const uint8_t* sigs /* n x 64 */,
                            const uint32_t* status_in /* n or NULL */, uint32_t* status_out /* n */);
/* the signer (VARIABLE TIME, see TIMING): public keys of n seeds; signatures of n messages, item b under seeds[b].  The _device forms
 * take device pointers (d_prefix too: prefix_len bytes in device memory, or NULL with prefix_len 0), are asynchronous on `stream` and
 * take no lock; d_seeds anywhere, d_keys / d_sigs 4-byte aligned. */
int eg_ed25519_keypair_batch(eg_ctx*, size_t n, const uint8_t* seeds /* n x 32 */, uint8_t* keys /* n x 32 */);
int eg_ed25519_keypair_batch_device(eg_ctx*, size_t n, const void* d_seeds, void* d_keys, void* stream);
int eg_ed25519_sign_batch(eg_ctx*, size_t n, const uint8_t* seeds /* n x 32 */, const uint8_t* msgs, size_t msg_stride, size_t msg_len,
                          const uint8_t* prefix, size_t prefix_len, uint8_t* sigs /* n x 64 */);
int eg_ed25519_sign_batch_device(eg_ctx*, size_t n, const void* d_seeds, const void* d_msgs, size_t msg_stride, size_t msg_len,
                                 const void* d_prefix, size_t prefix_len, void* d_sigs, void* stream);
/* SHA-512(prefix || msg_b) of n messages of one length, in the same prefix / stride form: the hash of the pass as a primitive */
int eg_sha512_batch(eg_ctx*, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                    uint8_t* digests /* n x 64 */);
int eg_sha512_batch_device(eg_ctx*, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const void* d_prefix,
                           size_t prefix_len, void* d_digests /* n x 64, 4-byte aligned */, void* stream);

/* ---- voter roll: one counted ballot per voter, by a policy, across batches and GPUs ----------------------------------------------------
 * Weeding flags a byte-for-byte copy and the signature pass a ballot that is not signed under a registered key; neither limits how many
 * fresh, validly signed ballots ONE registered voter gets counted.  Systems that allow re-voting as a defence against coercion count one
 * of them (Helios, Estonia: the last).  This pass says, per ballot, whether it is the one ballot of its voter that counts, and hands the
 * voter's precinct and weight to the tally FROM THE ROSTER, so that a voter cannot choose either by sending other arrays.
 * ORDER IN THE CHAIN: signatures -> verify -> weed -> roll -> tally.  A superseded ballot's ciphertexts are public, so they still belong
 * on the weeding board (weed first, over every accepted ballot); a weeded copy must not claim its voter's slot (roll after weeding, over
 * weeding's status_out).
 *
 * INPUTS.  key_index[b] (uint32) = the roster index of the voter who signed ballot b: the array the signature pass takes.  Ballot b has
 * the global SEQUENCE NUMBER s_b = seq_base + b; seq_base is the caller's count of ballots before this batch.  Ballot b PARTICIPATES iff
 * status_in == NULL or status_in[b] == EG_ST_OK; nothing else of a ballot that does not participate is read.
 * THE ROLL is the caller's array of n_keys uint64 words, zero-initialised, kept between calls, one word per roster key.  0 = no counted
 * ballot yet; otherwise the word is a PRIORITY that encodes the sequence number s of the counted ballot:
 *   EG_ROLL_LAST   word = s + 1             (the last ballot of a voter counts)
 *   EG_ROLL_FIRST  word = 2^63 - 1 - s      (the first one does)
 * s <= 2^63 - 2, so every word is in [1, 2^63 - 1] and signed and unsigned order agree.  Under either policy THE LARGER WORD WINS.  A roll
 * belongs to one policy.  EG_ROLL_WORD(seq, policy) / EG_ROLL_SEQ(word, policy) convert.
 * CAST.  For a voter v let C_v be the old roll[v] (if non-zero) together with the words of the participating ballots with key_index[b]
 * == v.  The new roll[v] = max C_v; voters without a ballot in the batch are not touched.  Ballot b is KEPT iff it participates,
 * key_index[b] < n_keys and its word equals the new roll[v].  The rule is a maximum, hence commutative and idempotent: batches may be
 * cast in any order, casting a batch twice changes nothing, and rolls of slabs, ranks or GPUs MERGE by the element-wise maximum of the
 * 64-bit words (as int64 or uint64: the words are below 2^63).
 * OUTPUTS per ballot.  superseded_by[b] (uint64) = EG_SEQ_NONE for a kept ballot, one that does not participate, and one without a winner
 * (off the roll, not cast); otherwise the sequence number decoded from the winning word.  status_out[b] (optional, may be status_in
 * itself) = status_in[b] (0 without one) for kept ballots and those that do not participate, otherwise EG_ST_SUPERSEDED with the detail
 *   EG_ROLL_SUPERSEDED 1  another ballot of the voter wins
 *   EG_ROLL_OFF_ROLL   2  key_index[b] >= n_keys; the value is never used as an index.  The signature pass refuses it already, so it
 *                         appears only with forged or skipped status words
 *   EG_ROLL_NOT_CAST   3  the check entries only: roll[v] == 0
 * groups_out[b] (optional, needs roster_groups[n_keys], uint32) = roster_groups[v] for a kept ballot, EG_GROUP_NONE otherwise;
 * weights_out[b] (optional, needs roster_weights[n_keys], uint64) = the roster weight for a kept ballot, 0 otherwise: exactly the arrays
 * eg_*_tally_grouped / _weighted take, beside status_out.
 * DISPLACED (optional, room for n entries of two uint64; comes with displaced_count).  For every voter whose NON-ZERO old word was
 * replaced in this call one entry (old sequence number, new sequence number), in ascending order of the winning ballot's index b;
 * *displaced_count (uint64) = their number.  It tells a host that keeps an archive or running tallies which earlier ballots have just
 * stopped counting.
 * FOUND.  The library WRITES three uint32 words: found[0] = participating ballots superseded (detail 1), found[1] = displaced entries
 * (counted with or without the array), found[2] = participating ballots off the roll.
 * CHECK.  eg_roll_check* takes the same inputs against a READ-ONLY roll - the final one at the close of the election, or a merged one.
 * Ballot b is kept iff it participates, its index is in range and roll[v] == EG_ROLL_WORD(s_b, policy).  The outputs are the same
 * without `displaced`; found[1] counts EG_ROLL_NOT_CAST.  It lets every archived batch be re-judged against the final roll before the
 * tally, and it is the second half of the MULTI-GPU RECIPE: every rank casts its slabs into a roll of its own (global sequence numbers),
 * the rolls are merged by one element-wise maximum (an all-reduce with MAX over int64), and every rank checks its slabs against the
 * merged roll.  The kept set is that of one cast over the concatenation.
 *
 * STATELESS with respect to the engine, as weeding and the signature pass: device pointers and a stream, no lock, no workspace of the
 * context; the verdict is a pure function of the inputs and does not depend on the order in which lanes run.  The `_device` forms are
 * asynchronous on `stream`, allocate nothing and never synchronise.  d_scratch of a cast holds eg_roll_cast_scratch_bytes(ctx, n, n_keys)
 * bytes (0 for arguments that would be refused, and for n == 0): 4 bytes per roster key, ~4 bytes per ballot.  The roll must not be read
 * or written by anything else while a cast that was given it is in flight.  eg_roll_cast / eg_roll_check: the same on host arrays
 * (the roll in and out), synchronous, with their own scratch.
 * EG_ERR_BAD_ARG before anything is launched: n >= 2^31; n_keys == 0 with n > 0; n_keys > EG_ROLL_KEYS_MAX; seq_base + n > 2^63 - 1; a
 * policy other than the two; a NULL key_index / roll / superseded_by / found with n > 0; groups_out without roster_groups; weights_out
 * without roster_weights; displaced without displaced_count or the reverse; a scratch that is NULL or too small; 64-bit arrays (roll,
 * roster_weights, superseded_by, weights_out, displaced, displaced_count) that are not 8-byte aligned, 32-bit arrays (the others and the
 * scratch) that are not 4-byte aligned.  The argument rules come before the context is looked at.  n == 0 is EG_OK: the roll is
 * untouched, the count and the found words (where given) are zero. */
enum { EG_ROLL_FIRST = 1, EG_ROLL_LAST = 2 };                                   /* policy */
enum { EG_ROLL_SUPERSEDED = 1, EG_ROLL_OFF_ROLL = 2, EG_ROLL_NOT_CAST = 3 };    /* detail of EG_ST_SUPERSEDED */
#define EG_SEQ_NONE (~(uint64_t)0)
#define EG_ROLL_KEYS_MAX (1u << 31)
#define EG_ROLL_SEQ_END (((uint64_t)1 << 63) - 1u)   /* seq_base + n may reach it */
#define EG_ROLL_WORD(seq, policy) ((policy) == EG_ROLL_LAST ? (uint64_t)(seq) + 1u : EG_ROLL_SEQ_END - (uint64_t)(seq))
#define EG_ROLL_SEQ(word, policy) ((policy) == EG_ROLL_LAST ? (uint64_t)(word) - 1u : EG_ROLL_SEQ_END - (uint64_t)(word))
size_t eg_roll_cast_scratch_bytes(const eg_ctx*, size_t n, size_t n_keys);
int eg_roll_cast_device(eg_ctx*, size_t n, const void* d_key_index /* uint32[n] */, const void* d_status_in /* uint32[n] or NULL */,
                        uint64_t seq_base, int policy, void* d_roll /* uint64[n_keys], in and out */, size_t n_keys,
                        const void* d_roster_groups /* uint32[n_keys] or NULL */, const void* d_roster_weights /* uint64[n_keys] or NULL */,
                        void* d_superseded_by /* uint64[n] */, void* d_status_out /* uint32[n] or NULL */,
                        void* d_groups_out /* uint32[n] or NULL */, void* d_weights_out /* uint64[n] or NULL */,
                        void* d_displaced /* n x 2 x uint64 or NULL */, void* d_displaced_count /* uint64 or NULL */,
                        void* d_found /* 3 x uint32 */, void* d_scratch, size_t scratch_bytes, void* stream);
int eg_roll_cast(eg_ctx*, size_t n, const uint32_t* key_index, const uint32_t* status_in /* or NULL */, uint64_t seq_base, int policy,
                 uint64_t* roll /* n_keys, in and out */, size_t n_keys, const uint32_t* roster_groups /* or NULL */,
                 const uint64_t* roster_weights /* or NULL */, uint64_t* superseded_by, uint32_t* status_out /* or NULL */,
                 uint32_t* groups_out /* or NULL */, uint64_t* weights_out /* or NULL */, uint64_t* displaced /* n x 2, or NULL */,
                 uint64_t* displaced_count /* or NULL */, uint32_t* found /* 3 */);
int eg_roll_check_device(eg_ctx*, size_t n, const void* d_key_index, const void* d_status_in /* or NULL */, uint64_t seq_base, int policy,
                         const void* d_roll /* uint64[n_keys] */, size_t n_keys, const void* d_roster_groups /* or NULL */,
                         const void* d_roster_weights /* or NULL */, void* d_superseded_by, void* d_status_out /* or NULL */,
                         void* d_groups_out /* or NULL */, void* d_weights_out /* or NULL */, void* d_found /* 3 x uint32 */, void* stream);
int eg_roll_check(eg_ctx*, size_t n, const uint32_t* key_index, const uint32_t* status_in /* or NULL */, uint64_t seq_base, int policy,
                  const uint64_t* roll /* n_keys */, size_t n_keys, const uint32_t* roster_groups /* or NULL */,
                  const uint64_t* roster_weights /* or NULL */, uint64_t* superseded_by, uint32_t* status_out /* or NULL */,
                  uint32_t* groups_out /* or NULL */, uint64_t* weights_out /* or NULL */, uint32_t* found /* 3 */);

/* ---- receipt log: a Merkle tree over the posted ballots, built and checked on the GPU ---------------------------------------------------
 * Every stage above decides which ballots count; none lets anyone check that a ballot which was accepted is still on the board when the
 * tally is made.  Weeding's bulletin board is a bare array of ciphertexts: no commitment over it, nothing for a voter to hold, nothing
 * that tells an auditor a board that silently dropped or swapped a ballot from an honest one.  Deployed systems close the gap with a hash
 * commitment over the posted ballots (Helios and Belenios publish ballot hashes, ElectionGuard issues tracking codes, Certificate
 * Transparency keeps the append-only log of RFC 6962).  These entries build that log, its tree, the receipts and the check of many
 * receipts at once.
 * ORDER IN THE CHAIN: signatures -> verify -> weed -> LEAVES -> roll -> tally.  The log is normally fed weeding's status_out: a superseded
 * ballot stays on the board as its ciphertexts do (it was posted, and its voter holds a receipt), a copy is not posted.
 *
 * THE RULE.  H(x) = the first 32 bytes of SHA-512(x).  The tree is RFC 6962 2.1:
 *   leaf_b     = H(0x00 || prefix || msg_b || extra_b)     prefix: 0..255 bytes per call (the election id, as for the signatures); msg_b:
 *                msg_len bytes at msgs + b * msg_stride (a packed ballot buffer is passed as it is); extra_b: optionally extra_len
 *                bytes at extra + b * extra_stride (the 64-byte signature, so that a receipt binds the signed envelope); extra == NULL
 *                with extra_len == 0 is valid
 *   node(l, r) = H(0x01 || l || r)
 *   MTH of N leaves: the empty tree is H of the empty string, one leaf is its own root, otherwise node(MTH of the first k, MTH of the
 *                rest) with k the largest power of two below N.  Equivalent, and what the kernels do: level L + 1 has ceil(n_L / 2)
 *                nodes, node i = node(a[2i], a[2i + 1]), and an odd last node is promoted unchanged.
 * eg_merkle_depth(N) = ceil(log2 N), 0 for N <= 1.  THE LOG is the caller's array of leaves, 32 bytes each (level 0).  THE NODE STORE
 * holds levels 1 .. depth back to back: eg_merkle_nodes_bytes(N) bytes, level L at the byte offset and with the node count that
 * eg_merkle_level names (level 0: offset 0 and N, the log itself).
 * RECEIPT of leaf i in a tree of N leaves: (i, N, leaf, path), path = the audit path of RFC 6962 2.1.1: bottom-up, at each level the
 * sibling i ^ 1 if that index exists at the level, otherwise nothing, and then i >>= 1.  Its length is a function of (i, N), at most
 * depth(N).
 * CHECK: the algorithm of RFC 9162 2.1.3.2.  The verdict of a receipt is a uint32, the first failure in this order wins:
 *   0                        proven
 *   EG_MERKLE_BAD_INDEX   1  i >= N
 *   EG_MERKLE_BAD_LENGTH  2  path_len is not the length that (i, N) demands; no path byte is read then
 *   EG_MERKLE_MISMATCH    3  the recomputed root differs from the given one
 *
 * LEAVES.  Ballot b PARTICIPATES iff status_in == NULL or status_in[b] == EG_ST_OK; bytes of other ballots are never read.
 * leaf_index[b] (uint64) = n_prior + the rank of b among the participating ballots, EG_LEAF_NONE otherwise: the index a voter's receipt
 * carries.  leaves_out (optional, n x 32 bytes) = the leaf of every ballot, zeroed for ballots that do not participate.  APPEND
 * (log_count != NULL): the participating leaves are written in ballot order behind the first n_prior entries of the caller's log
 * (log_cap x 32 bytes) and *log_count (uint64) = n_prior + appended.  If they do not fit log_cap nothing is appended, the count is
 * n_prior and found[1] is set.  The library WRITES found[0] = the number of leaves, found[1] = non-zero if the append did not fit.
 * TREE.  Every call is a FULL REBUILD over the N leaves of the log: root (32 bytes) and, optionally, the node store.  There is no
 * incremental frontier state (eg_merkle_grow, below, builds the next store out of the last one).  One launch per 10 levels: two launches up to 2^20 leaves, three above.  Without a node store the top
 * level of every launch goes through eg_merkle_tree_scratch_bytes(N) bytes of scratch (0 up to 1024 leaves).
 * PATHS.  For m requested leaf indices (uint64), one lane each, out of the log and the node store: paths (m x depth(N) x 32 bytes, the
 * unused tail of a row zeroed) and path_len (uint32[m]); an index >= N gives EG_MERKLE_NO_PATH and a zeroed row.
 * CHECK of m receipts (index, leaf, path, path_len) against a shared (N, root): receipt j's path is path_len[j] entries at paths + j *
 * path_stride; verdict (uint32[m]) by the rule above; found[0..2] = the numbers of BAD_INDEX, BAD_LENGTH and MISMATCH verdicts.
 * MULTI-GPU: slabs hash their leaves on their own GPUs with the global n_prior of each slab and no append; the leaves_out rows are
 * gathered in slab order with the existing byte all-gather (distributed.gather_tallies; equal rows, so slabs are padded to the largest
 * and leaf_index says which rows hold a leaf) and the tree is built where they land.  No new collective.
 *
 * TIMING: variable time throughout; the log, the receipts and the root are public data.
 * STATELESS as weeding and the roll: the `_device` forms take device pointers and a stream, take no lock, use no workspace of the
 * context, allocate nothing and never synchronise (`prefix` is HOST memory and is copied during the call).  The host forms do the same
 * on host arrays, synchronous, with their own scratch; eg_merkle_leaves returns EG_ERR_BAD_ARG AFTER writing its outputs when the
 * append did not fit.  eg_merkle_depth, eg_merkle_nodes_bytes, eg_merkle_level and the two scratch sizes are pure host functions.
 * EG_ERR_BAD_ARG before anything is launched: NULL mandatory pointers with work to do (msgs, leaf_index, found; root, the log of a
 * non-empty tree; index, path_len and, for N > 1, log, nodes and paths; the arrays of a check); prefix_len > 255 or a NULL prefix with a
 * length; msg_stride < msg_len or extra_stride < extra_len; a NULL extra with a length; n, m, N or n_prior >= EG_MERKLE_LEAVES_MAX;
 * with an append n_prior > log_cap or a NULL log; a path_stride below 32 depth(N) or no multiple of 4; a scratch that is NULL or too
 * small; leaf, node, path, root, status, verdict and found arrays and the scratch not 4-byte aligned; 64-bit arrays (leaf_index,
 * log_count, index) not 8-byte aligned.  Messages and extras may lie anywhere.  The argument rules come before the context is looked
 * at.  n == 0 / m == 0 is EG_OK: the count is n_prior and the found words (where given) are zero. */
enum { EG_MERKLE_BAD_INDEX = 1, EG_MERKLE_BAD_LENGTH = 2, EG_MERKLE_MISMATCH = 3 };   /* verdict of a receipt */
#define EG_MERKLE_HASH_BYTES 32
#define EG_MERKLE_LEAVES_MAX (1u << 31)
#define EG_LEAF_NONE (~(uint64_t)0)
#define EG_MERKLE_NO_PATH 0xffffffffu
int eg_merkle_depth(uint64_t n_leaves);
size_t eg_merkle_nodes_bytes(uint64_t n_leaves);
int eg_merkle_level(uint64_t n_leaves, int level, uint64_t* offset /* bytes into the node store */, uint64_t* count /* nodes */);
size_t eg_merkle_leaves_scratch_bytes(size_t n);
size_t eg_merkle_tree_scratch_bytes(uint64_t n_leaves);
int eg_merkle_leaves_device(eg_ctx*, size_t n, const void* d_msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix /* host */,
                            size_t prefix_len, const void* d_extra /* or NULL */, size_t extra_stride, size_t extra_len,
                            const void* d_status_in /* uint32[n] or NULL */, uint64_t n_prior, void* d_leaf_index /* uint64[n] */,
                            void* d_leaves_out /* n x 32 or NULL */, void* d_log /* log_cap x 32, or NULL without an append */,
                            uint64_t log_cap, void* d_log_count /* uint64, or NULL: no append */, void* d_found /* 2 x uint32 */,
                            void* d_scratch, size_t scratch_bytes, void* stream);
int eg_merkle_leaves(eg_ctx*, size_t n, const uint8_t* msgs, size_t msg_stride, size_t msg_len, const uint8_t* prefix, size_t prefix_len,
                     const uint8_t* extra /* or NULL */, size_t extra_stride, size_t extra_len, const uint32_t* status_in /* or NULL */,
                     uint64_t n_prior, uint64_t* leaf_index, uint8_t* leaves_out /* or NULL */, uint8_t* log /* log_cap x 32, or NULL */,
                     uint64_t log_cap, uint64_t* log_count /* or NULL: no append */, uint32_t* found /* 2 */);
int eg_merkle_tree_device(eg_ctx*, uint64_t n_leaves, const void* d_log /* n_leaves x 32 */, void* d_root /* 32 */,
                          void* d_nodes /* eg_merkle_nodes_bytes, or NULL */, void* d_scratch /* used without d_nodes */,
                          size_t scratch_bytes, void* stream);
int eg_merkle_tree(eg_ctx*, uint64_t n_leaves, const uint8_t* log, uint8_t* root, uint8_t* nodes /* or NULL */);
int eg_merkle_paths_device(eg_ctx*, size_t m, const void* d_index /* uint64[m] */, uint64_t n_leaves, const void* d_log, const void* d_nodes,
                           void* d_paths /* m x depth x 32 */, void* d_path_len /* uint32[m] */, void* stream);
int eg_merkle_paths(eg_ctx*, size_t m, const uint64_t* index, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes, uint8_t* paths,
                    uint32_t* path_len);
int eg_merkle_check_device(eg_ctx*, size_t m, const void* d_index /* uint64[m] */, const void* d_leaves /* m x 32 */, const void* d_paths,
                           size_t path_stride, const void* d_path_len /* uint32[m] */, uint64_t n_leaves, const void* d_root /* 32 */,
                           void* d_verdict /* uint32[m] */, void* d_found /* 3 x uint32 */, void* stream);
int eg_merkle_check(eg_ctx*, size_t m, const uint64_t* index, const uint8_t* leaves, const uint8_t* paths, size_t path_stride,
                    const uint32_t* path_len, uint64_t n_leaves, const uint8_t* root, uint32_t* verdict, uint32_t* found /* 3 */);
/* The receipt log, continued: PAST HEADS and CONSISTENCY PROOFS (RFC 6962 2.1.2, RFC 9162 2.1.4).  A receipt proves "my ballot is under
 * root R_N"; these entries prove "the board that published (m, R_m) earlier is the same board, grown, that now publishes (N, R_N)": the
 * holder of an old head checks it once against the new one, and every receipt that proved against R_m counts for good, with no
 * re-issue.  Nothing is added to the tree: node j of level L of the node store is the tree hash of leaves [j 2^L, min((j + 1) 2^L, N)),
 * the promoted ragged last node included, and every node that is needed is one of those.  R_m = MTH of the first m leaves, 1 <= m <= N.
 * PAST HEAD.  R_0 = H("").  For m >= 1 walk the bits of m from the bottom: x = m at level L = 0; where x is odd take node (L, x - 1), a
 * complete subtree wholly inside the first m leaves, and fold it on the left, acc = node(that, acc) (the first node taken is acc itself);
 * then x >>= 1, L += 1.  At most depth(N) node hashes; R_N is the root.
 * CONSISTENCY PROOF of (m, N) = PROOF(m, D[N]) of RFC 9162 2.1.4.1, read out of the store: empty for m == N; otherwise node = m - 1 at
 * level L = 0, and while node is odd node >>= 1, L += 1.  If node != 0 the first entry is store node (L, node), THE SEED: the last
 * complete piece of the old tree (node == 0: m is a power of two and there is no seed).  Then the audit path of node (L, node) inside
 * the N-tree, bottom-up as for a receipt: at each level with more than one node the sibling node ^ 1 if that index exists at the level,
 * then node >>= 1.  eg_merkle_consistency_len(m, N) is that count: 0 for m == N, at most depth(N) + 1 (reached, e.g. (3, 6) -> 4),
 * EG_MERKLE_NO_PATH for m == 0 or m > N.
 * CHECK of a proof: the algorithm of RFC 9162 2.1.4.2.  The verdict is a uint32, the first failure in this order wins:
 *   0                           proven
 *   EG_MERKLE_BAD_INDEX      1  old_size == 0 or old_size > N
 *   EG_MERKLE_BAD_LENGTH     2  proof_len is not eg_merkle_consistency_len(old_size, N); no proof byte is read then
 *   EG_MERKLE_MISMATCH_OLD   4  the old root recomputed from the proof differs from the given old root
 *   EG_MERKLE_MISMATCH       3  the new root recomputed differs from the given new root
 * With the length exact the walk is driven by (m, N) alone: fr = sr = entry 0 if there is a seed, else the given old root; at each level
 * with an existing sibling c: if the node index is odd fr = node(c, fr) and sr = node(c, sr), otherwise sr = node(sr, c); then fr is
 * compared with the old root and sr with the new one.  For m == N fr = sr = the given old root, so unequal roots give EG_MERKLE_MISMATCH.
 * HEADS of m sizes (uint64) out of the log and the node store of N leaves: heads (m x 32 bytes); size 0 gives H(""), a size above N a
 * zeroed row, counted in found[0].  CONSISTENCY of m old sizes: proofs (m x (depth(N) + 1) x 32 bytes, the unused tail of a row zeroed)
 * and proof_len (uint32[m]); old_size 0 or above N gives EG_MERKLE_NO_PATH and a zeroed row.  CONSISTENCY_CHECK of m proofs (old_size,
 * old_root, proof, proof_len) against a shared (N, root): proof j is proof_len[j] entries at proofs + j * proof_stride; found[0..3] = the
 * numbers of BAD_INDEX, BAD_LENGTH, MISMATCH and MISMATCH_OLD verdicts.
 * The contract is the one above: variable time on public data; stateless; the `_device` forms take no lock, allocate nothing and never
 * synchronise; m == 0 is EG_OK with zeroed found words; the argument rules come before the context is looked at, EG_ERR_BAD_ARG for
 * NULL mandatory pointers with work to do (the log may be NULL for N == 0, the nodes for N <= 1, the proofs of a check for N <= 1), m or
 * N >= EG_MERKLE_LEAVES_MAX, a proof_stride below 32 (depth(N) + 1) or no multiple of 4, 32-bit arrays not 4-byte aligned, 64-bit
 * arrays (size, old_size) not 8-byte aligned.  eg_merkle_consistency_len is a pure host function. */
enum { EG_MERKLE_MISMATCH_OLD = 4 };                                                  /* verdict of a consistency proof */
uint32_t eg_merkle_consistency_len(uint64_t old_size, uint64_t n_leaves);
int eg_merkle_heads_device(eg_ctx*, size_t m, const void* d_size /* uint64[m] */, uint64_t n_leaves, const void* d_log, const void* d_nodes,
                           void* d_heads /* m x 32 */, void* d_found /* 1 x uint32 */, void* stream);
int eg_merkle_heads(eg_ctx*, size_t m, const uint64_t* size, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes, uint8_t* heads,
                    uint32_t* found /* 1 */);
int eg_merkle_consistency_device(eg_ctx*, size_t m, const void* d_old_size /* uint64[m] */, uint64_t n_leaves, const void* d_log,
                                 const void* d_nodes, void* d_proofs /* m x (depth + 1) x 32 */, void* d_proof_len /* uint32[m] */,
                                 void* stream);
int eg_merkle_consistency(eg_ctx*, size_t m, const uint64_t* old_size, uint64_t n_leaves, const uint8_t* log, const uint8_t* nodes,
                          uint8_t* proofs, uint32_t* proof_len);
int eg_merkle_consistency_check_device(eg_ctx*, size_t m, const void* d_old_size /* uint64[m] */, const void* d_old_root /* m x 32 */,
                                       const void* d_proofs, size_t proof_stride, const void* d_proof_len /* uint32[m] */, uint64_t n_leaves,
                                       const void* d_root /* 32 */, void* d_verdict /* uint32[m] */, void* d_found /* 4 x uint32 */,
                                       void* stream);
int eg_merkle_consistency_check(eg_ctx*, size_t m, const uint64_t* old_size, const uint8_t* old_root, const uint8_t* proofs, size_t proof_stride,
                                const uint32_t* proof_len, uint64_t n_leaves, const uint8_t* root, uint32_t* verdict, uint32_t* found /* 4 */);
/* The receipt log, continued: GROW.  A board that publishes a head after every batch would pay eg_merkle_tree's full rebuild per batch,
 * re-hashing nodes that cannot have changed.  eg_merkle_grow builds the node store and the root of the N-leaf log out of the node store
 * of its first m leaves (old_size) and hashes only what the append changed.
 * RESULT: nodes and root are byte for byte what eg_merkle_tree(N, log, root, nodes) writes, in the same layout, so paths, heads,
 * consistency and the two checks work on the grown store unchanged.
 * WORK.  Store node (L, j) is unchanged by the append exactly when (j + 1) 2^L <= m, but every level above the first starts at another
 * offset once N grows.  The launches are the tree's: launch k reduces input level L0 = 10 k in tiles of 1024 input nodes.  Its first
 * tile0 = (m >> L0) >> 10 tiles lie wholly inside the old tree: their nodes on every level of the launch are COPIED from the old store to
 * the new offset.  The tiles from tile0 on are reduced as eg_merkle_tree reduces them: O(N - m + 1024 depth(N) / 10) hashes.  m == 0 is
 * a full build; m == N copies the whole tiles and reduces the ragged last tile of each launch again (nothing at all if N is a power of
 * 1024); N == 0 gives H(""), N == 1 the leaf; the depth may grow by any amount between m and N.
 * NEVER READ: leaves of the log below (m >> 10) << 10, and old-store nodes with (j + 1) 2^L > m, the old tree's ragged and promoted
 * nodes.
 * OUT OF PLACE: the old store is left untouched and stays a valid store for (m, R_m), so receipts against the old head can be served
 * while the new store is built.  The byte ranges [nodes_old, + eg_merkle_nodes_bytes(m)) and [nodes, + eg_merkle_nodes_bytes(N)) must
 * not overlap.
 * The contract is the one above: variable time on public data; stateless; the `_device` form takes no lock, uses no workspace of the
 * context, allocates nothing, never synchronises and needs no scratch: one copy launch, then the tile launches and the root on the one
 * stream.  The host form does the same on host arrays, synchronous; the leaves that are never read are not sent to the device either.
 * EG_ERR_BAD_ARG before anything is launched, and before the context is looked at: old_size > N; old_size or N >=
 * EG_MERKLE_LEAVES_MAX; a NULL root; a NULL log with N > 0; NULL nodes with N > 1; NULL nodes_old with old_size > 1; overlapping stores;
 * in the `_device` form any array not 4-byte aligned. */
int eg_merkle_grow_device(eg_ctx*, uint64_t old_size, const void* d_nodes_old /* eg_merkle_nodes_bytes(old_size); may be NULL for old_size <= 1 */,
                          uint64_t n_leaves /* >= old_size */, const void* d_log /* n_leaves x 32 */,
                          void* d_nodes /* eg_merkle_nodes_bytes(n_leaves); may be NULL for n_leaves <= 1 */, void* d_root /* 32 */, void* stream);
int eg_merkle_grow(eg_ctx*, uint64_t old_size, const uint8_t* nodes_old, uint64_t n_leaves, const uint8_t* log, uint8_t* nodes, uint8_t* root);

/* ---- batch tier on several GPUs of ONE process (SURVEY.md 8b `device_mask`; the reference's host is one single-threaded process,
 * examples/voting.rs:179-213) -----------------------------------------------------------------------------------------------------
 * per_device[d], d < n_dev: params objects of the SAME election (same key, options, kind), each created on its own context
 * (eg_init(d, ..): one per GPU; two contexts on one GPU work too).
 *
 * eg_verify_*_batch_multi (HOST buffers): the batch is cut into contiguous slabs - slab d = ballots [n d / n_dev, n (d + 1) / n_dev) -
 * and one host thread per params object inside the library runs eg_verify_*_batch on its slab (its own device, streams, uploads; pin
 * the ballots with hipHostRegister / hipHostMalloc for full upload speed).  status: n words, in ballot order.
 *
 * eg_verify_*_batch_multi_device (DEVICE buffers): slab d is ALREADY RESIDENT on GPU d - a host that generated or received its ballots
 * per GPU pays no copy.  n_per_dev[d] ballots at d_ballots[d], verdicts to d_status[d] (n_per_dev[d] words), both device pointers on
 * per_device[d]'s device; streams[d] a hipStream_t of that device (streams == NULL: the null streams).  One host thread per slab
 * enqueues eg_verify_*_batch_device on its stream and waits for that stream: the call returns with every verdict written.
 *
 * Tallies.  Every params object ADDS the accepted ballots of its slab to its OWN running tally; tally_out (may be NULL, n_options*64
 * bytes) receives the tally of this call's whole batch alone, the slabs' tallies merged with the element addition of the primitive
 * tier - the in-process counterpart of the RCCL all-gather of the one-process-per-GPU path (examples/tally_exchange.cpp).
 * eg_*_tally_encode_multi = the sum of the running tallies (every encoding is checked: a running tally that does not decode, or params
 * objects of different elections, fail the call).
 *
 * A multi call HOLDS its params objects from its first check to its merge: it waits for a one-shot eg_verify_*_json that is running on
 * one of them, fails with EG_ERR_BAD_ARG - before it has touched anything - when an explicitly opened JSON stream owns one, and calls of
 * other threads on a held object wait until it is over.  Nothing in it drains a device: the running tallies are set aside behind an event
 * of the object's last asynchronous call, and slab d starts behind that copy on streams[d].  The calling thread's current HIP device is
 * put back to what it was when the call returns (the multi-GPU JSON entries do the same).
 *
 * AFTER A FAILURE.  An error in any slab fails the whole call; eg_last_error names the slab.  Verdicts of other slabs may have been
 * written, but NO running tally has advanced: every multi verify call sets the running tallies aside before it starts (a
 * device-to-device copy of 2 n_options points on each GPU) and puts them back when any slab, or the final merge, fails - the caller may simply retry the batch, or go on with
 * the next one, without resetting anything.  Only if putting them back fails as well (the device is gone) does the error text say
 * "could not be restored"; then reset every params object (eg_*_tally_reset) and re-import the last checkpoint (eg_*_tally_add).
 * Nothing thrown inside a slab's thread crosses the ABI: it becomes that slab's error. */
int eg_verify_choice_batch_multi(eg_choice_params* const* per_device, int n_dev, size_t n, const uint8_t* ballots, uint32_t* status,
                                 uint8_t* tally_out);
int eg_verify_qv_batch_multi(eg_qv_params* const* per_device, int n_dev, size_t n, const uint8_t* ballots, uint32_t* status,
                             uint8_t* tally_out);
int eg_verify_choice_batch_multi_device(eg_choice_params* const* per_device, int n_dev, const size_t* n_per_dev, const void* const* d_ballots,
                                        void* const* d_status, void* const* streams, uint8_t* tally_out);
int eg_verify_qv_batch_multi_device(eg_qv_params* const* per_device, int n_dev, const size_t* n_per_dev, const void* const* d_ballots,
                                    void* const* d_status, void* const* streams, uint8_t* tally_out);
int eg_choice_tally_encode_multi(eg_choice_params* const* per_device, int n_dev, uint8_t* out /* n_options*64 */);
int eg_qv_tally_encode_multi(eg_qv_params* const* per_device, int n_dev, uint8_t* out /* n_options*64 */);

/* ---- batch tier: single-ciphertext proofs --------------------------------------------------------------
 * PublicKey::verify_zero (keys/impls.rs:59-69)   item = ciphertext(64) || challenge || response              128 B
 * PublicKey::verify_bool (keys/impls.rs:100-112) item = ciphertext(64) || e0 || s0 || s1                     160 B
 * PublicKey::verify_range(keys/impls.rs:142-151) item = ciphertext(64) || partial_ciphertexts || e0 || responses
 *   with RangeDecomposition::optimal(upper_bound) (range.rs:148-153); eg_proof_item_size gives the stride.
 * status: EG_ST_OK, EG_ST_BAD_*, EG_ST_SUM_CHALLENGE (zero: ChallengeMismatch) or EG_ST_RANGE_CHALLENGE (bool/range). */
typedef struct eg_proof_params eg_proof_params;
enum { EG_PROOF_ZERO = 0, EG_PROOF_BOOL = 1, EG_PROOF_RANGE = 2, EG_PROOF_SHARE = 3, EG_PROOF_SUMSQ = 4, EG_PROOF_COMMIT_EQUIV = 5 };
int eg_proof_params_create(eg_ctx*, const uint8_t pk[32], int kind, uint64_t upper_bound, eg_proof_params** out);
/* PublicKeySet::verify_share (sharing/key_set.rs:209-228) for one participant: item = the ciphertext's
 * random element R(32) || decryption share dh(32) || challenge || response; status EG_ST_SUM_CHALLENGE on ChallengeMismatch.
 * Verify with eg_verify_proof_batch. */
int eg_share_params_create(eg_ctx*, const uint8_t shared_key[32], uint64_t shares, uint64_t threshold, uint64_t index,
                           const uint8_t participant_key[32], eg_proof_params** out);
/* SumOfSquaresProof::verify(ciphertexts, sum_of_squares_ciphertext, receiver, transcript) (mul.rs:190-260) with
 * transcript = Transcript::new(label) (tests/snapshots.rs:133-153 uses b"test"): item = n_values value ciphertexts (64 B each) ||
 * sum-of-squares ciphertext (64) || challenge || ciphertext_responses (2 n_values x 32) || sum_response; status EG_ST_OK,
 * EG_ST_BAD_* or EG_ST_QV_CREDIT_EQUIV_CHALLENGE (ChallengeMismatch).  A wrong number of responses (LenMismatch, mul.rs:197-202)
 * cannot be expressed in a packed item.  Verify with eg_verify_proof_batch. */
int eg_sumsq_params_create(eg_ctx*, const uint8_t pk[32], int n_values, const char* label, size_t label_len, eg_proof_params** out);
/* CommitmentEquivalenceProof::verify(ciphertext, receiver, commitment, commitment_blinding_base, transcript) (proofs/commitment.rs:186-238)
 * with transcript = Transcript::new(label) (tests/snapshots.rs:163-177 uses b"test"): an ElGamal ciphertext (R, B) under `pk` and a
 * Pedersen commitment C = [v]G + [r_c]H hide the same value.  item (224 B) = R || B (Ciphertext::to_bytes) || C || challenge ||
 * randomness_response || value_response || commitment_response (struct order, commitment.rs:115-124); status EG_ST_OK, EG_ST_BAD_* with
 * the item index 0..6, or EG_ST_SUM_CHALLENGE (ChallengeMismatch).  Verify with eg_verify_proof_batch.  A caller that goes on to use
 * the transcript after the proof (examples/equivalence.rs hands it to Bulletproofs) is not served: every item starts a fresh transcript.
 * blinding_base = H, the third fixed base of the params object, with comb tables of its own (0.8 GB, and the wide form with the other
 * two).  It must decode and must NOT be the identity (EG_ERR_BAD_ARG): the reference accepts any element, but a commitment over the
 * identity hides nothing, and an identity comb table is a case nothing in this library has ever built.  pk as for every params object
 * (EG_ERR_BAD_PUBLIC_KEY); label up to 255 bytes. */
int eg_commit_equiv_params_create(eg_ctx*, const uint8_t pk[32], const uint8_t blinding_base[32], const char* label, size_t label_len,
                                  eg_proof_params** out);
void eg_proof_params_destroy(eg_proof_params*);
size_t eg_proof_item_size(const eg_proof_params*);
int eg_verify_proof_batch(eg_proof_params*, size_t n, const uint8_t* items, uint32_t* status);
int eg_verify_proof_batch_device(eg_proof_params*, size_t n, const void* d_items, void* d_status, void* stream);

/* ---- synthetic ballots and proofs on the GPU (EncryptedChoice::new / QuadraticVotingBallot::new, and the provers
 * of every proof kind that eg_verify_proof_batch checks) ---------
 * VARIABLE TIME in the choices / votes / values and in every RNG-drawn secret, and for the decryption-share prover in the SECRET SHARE
 * itself (a radix-16 ladder indexed by its digits; see TIMING at the top): these entry points make test and benchmark inputs; they are
 * not a voting client and not a tallier.
 * Ballot i of the call is produced from ChaChaRng::seed_from_u64(base_seed + first + i) with the reference's
 * RNG draw order (choice.rs:313-349, ring.rs:54-194, log_equality.rs:114-139, range.rs:462-534, mul.rs:107-181);
 * the voter's selection comes from a second stream seeded with the complemented seed.  n_selected is only
 * used for multi-choice params.  A ballot's secrets live in a per-lane workspace in device memory sized from the election's
 * shape, so the generators accept every election the verifiers accept (n_options up to 4000 / 256). */
int eg_choice_encrypt_batch_device(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, int n_selected,
                                   void* d_out, void* stream);
int eg_choice_encrypt_batch(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, int n_selected,
                            uint8_t* out /* host, n * eg_choice_ballot_size */);
int eg_qv_encrypt_batch_device(eg_qv_params*, uint64_t base_seed, size_t first, size_t n, void* d_out, void* stream);
/* The same provers with the CALLER's choices: EncryptedChoice::single(params, choice, rng) / ::new(params, &[bool], rng)
 * (choice.rs:296-349) and QuadraticVotingBallot::new(params, votes, rng) (quadratic_voting.rs:234-284).  selection:
 * ceil(n_options / 32) uint32 per ballot, bit k of the bitmask set <=> option k chosen (single-choice: exactly one bit); votes:
 * n_options uint32 per ballot with
 * sum(v^2) <= credits.  rng_skip = number of 64-byte draws the ballot's RNG, ChaChaRng::seed_from_u64(base_seed + first + i), has
 * already served: tests/snapshots.rs:107-161 draw the keypair first, so (12345, rng_skip = 1) reproduces the reference's
 * `encrypted-choice`, `encrypted-multi-choice` and `qv-ballot` snapshots byte for byte.  The host forms validate the choices
 * (EG_ERR_BAD_ARG); the device forms trust them, as the reference trusts its caller's assertions. */
int eg_choice_encrypt_selected_batch(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                     const uint32_t* selection /* n x ceil(n_options / 32) */, uint8_t* out);
int eg_choice_encrypt_selected_batch_device(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                            const void* d_selection, void* d_out, void* stream);
int eg_qv_encrypt_votes_batch(eg_qv_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                              const uint32_t* votes /* n x n_options */, uint8_t* out);
int eg_qv_encrypt_votes_batch_device(eg_qv_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                     const void* d_votes, void* d_out, void* stream);

/* THE OPENER of the synthetic ballots above, VARIABLE TIME like the generators (see TIMING): it makes test and benchmark openings for
 * eg_*_open_check.  A real voting device opens its ballots on its own CPU, in constant time where its threat model asks for it; this is
 * not that.  The entries reproduce the values and the encryption randomness of the ballots that the generator entries make from the
 * SAME arguments: eg_choice_encrypt_selected_batch / eg_qv_encrypt_votes_batch with a selection / votes, eg_choice_encrypt_batch /
 * eg_qv_encrypt_batch_device (rng_skip 0) with NULL, where the choice or the votes come from the second stream.  No point is multiplied: one
 * ChaCha block and one reduction mod l per slot, at the position the generator drew it.  Choice: option k's r is draw rng_skip + 2k +
 * #{j < k : option j not chosen}.  Quadratic voting: vote k's r is draw rng_skip + k D, D = rings + sum of the ring sizes of the vote
 * range.  values_out: n x n_options uint64 (8-byte aligned), rand_out: n x n_options x 32 bytes (4-byte aligned).  Stateless: no lock, no
 * workspace.  EG_ERR_BAD_ARG: n >= 2^31, NULL outputs with n > 0, misaligned device pointers, NULL params, n x n_options above
 * EG_OPEN_ITEMS_MAX, n_selected out of range (multi-choice without a selection); the host forms validate the choices as the generators'
 * host forms do. */
int eg_choice_open_batch_device(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, int n_selected, uint64_t rng_skip,
                                const void* d_selection /* or NULL */, void* d_values_out, void* d_rand_out, void* stream);
int eg_choice_open_batch(eg_choice_params*, uint64_t base_seed, size_t first, size_t n, int n_selected, uint64_t rng_skip,
                         const uint32_t* selection /* n x ceil(n_options / 32), or NULL */, uint64_t* values_out, uint8_t* rand_out);
int eg_qv_open_batch_device(eg_qv_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                            const void* d_votes /* or NULL */, void* d_values_out, void* d_rand_out, void* stream);
int eg_qv_open_batch(eg_qv_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                     const uint32_t* votes /* n x n_options, or NULL */, uint64_t* values_out, uint8_t* rand_out);

/* CommitmentEquivalenceProof::new (proofs/commitment.rs:134-181) on a commitment-equivalence params object, VARIABLE TIME like the other
 * generators (see TIMING): test and benchmark inputs only.  Item i encrypts values[i] and commits to it, drawing from
 * ChaChaRng::seed_from_u64(base_seed + first + i) after rng_skip 64-byte draws, in the reference's order: r (CiphertextWithValue::new),
 * r_c (SecretKey::generate), e_r, e_v, e_c.  (12345, rng_skip = 1), value 123, label "test" and the Bulletproofs blinding base
 * reproduce the reference's `commitment-equiv-proof` snapshot byte for byte.  blindings (may be NULL): r_c of every item, 32 bytes
 * each - what a caller needs to prove anything further about the commitment. */
int eg_commit_equiv_prove_batch_device(eg_proof_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                       const void* d_values /* n x uint64 */, void* d_items /* n x 224 */,
                                       void* d_blindings /* n x 32 or NULL */, void* stream);
int eg_commit_equiv_prove_batch(eg_proof_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                const uint64_t* values, uint8_t* items, uint8_t* blindings /* or NULL */);

/* The provers of the other single-item proofs, on the params objects that verify them (eg_proof_params_create, eg_sumsq_params_create):
 *   EG_PROOF_ZERO   PublicKey::encrypt_zero (keys/impls.rs:31-52): no input; draws r, x.
 *   EG_PROOF_BOOL   PublicKey::encrypt_bool (:77-89): one uint64 per item, 0 or 1.
 *   EG_PROOF_RANGE  PublicKey::encrypt_range (:124-133) with RangeDecomposition::optimal(upper_bound): one uint64 per item, < upper_bound.
 *   EG_PROOF_SUMSQ  SumOfSquaresProof::new (mul.rs:107-181) on fresh ciphertexts, as tests/snapshots.rs:128-150 makes them: n_values
 *                   uint64 per item; the ciphertext of sum(v^2) is drawn FIRST, then one per value, then the proof's own draws.
 * Item i draws from ChaChaRng::seed_from_u64(base_seed + first + i) after rng_skip 64-byte draws, in the reference's order, and is
 * written in the layout eg_verify_proof_batch reads (eg_proof_item_size).  (12345, rng_skip = 1) reproduces the reference's
 * `zero-encryption`, `bool-encryption` (true), `range-encryption` (bound 100, value 42) and `sum-sq-proof` ([1, 3, 3, 7, 5], label
 * "test") snapshots byte for byte.  eg_proof_prove_input_size = bytes of input per item (0, 8, 8, 8 n_values; d_inputs / inputs may be
 * NULL for EG_PROOF_ZERO only).  EG_ERR_BAD_ARG for EG_PROOF_SHARE (needs the secret: below) and EG_PROOF_COMMIT_EQUIV (its own entry
 * above also returns the blindings).  The host form refuses, with EG_ERR_BAD_ARG, what makes the reference panic or overflow: a bool
 * above 1, a value >= upper_bound, a sum of squares >= 2^64; the device form trusts its inputs. */
size_t eg_proof_prove_input_size(const eg_proof_params*);
int eg_proof_prove_batch_device(eg_proof_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                                const void* d_inputs /* uint64 values; NULL for zero */, void* d_items, void* stream);
int eg_proof_prove_batch(eg_proof_params*, uint64_t base_seed, size_t first, size_t n, uint64_t rng_skip,
                         const uint64_t* inputs, uint8_t* items);
/* ActiveParticipant::decrypt_share (sharing/participant.rs:163-186) on a params object of eg_share_params_create, for the participant
 * whose key it holds: item i = R_i || dh = [secret_share]R_i || challenge || response (128 B, what eg_verify_proof_batch reads) for the
 * ciphertext random element R_i = ct_random + 32 i; draws x only.  ok[i] = 0 and a zeroed item where R_i does not decode; the other
 * items are unaffected.  It is NOT checked that [secret_share]G is the participant key: a wrong share gives items that do not verify,
 * as in the reference (log_equality.rs:111-113).  The host form refuses a non-canonical secret_share (EG_ERR_BAD_ARG). */
int eg_share_prove_batch_device(eg_proof_params*, const uint8_t secret_share[32], uint64_t base_seed, size_t first, size_t n,
                                uint64_t rng_skip, const void* d_ct_random /* n x 32 */, void* d_items /* n x 128 */,
                                void* d_ok /* n bytes */, void* stream);
int eg_share_prove_batch(eg_proof_params*, const uint8_t secret_share[32], uint64_t base_seed, size_t first, size_t n,
                         uint64_t rng_skip, const uint8_t* ct_random, uint8_t* items, uint8_t* ok);

/* ---- wire ingest (host only, no GPU needed) ------------------------------------------------------------
 * The reference's serde layout in human-readable formats (src/serde.rs:19-80,179-355: every scalar / element an unpadded base64url
 * string; structures as derived on EncryptedChoice, RingProof, LogEqualityProof, QuadraticVotingBallot, RangeProof,
 * SumOfSquaresProof, Ciphertext) -> packed ballots.  `json` holds the ballots as ONE JSON array of objects or as objects back to
 * back / one per line (what examples/voting.rs:195-198 prints); object k is written to packed + k * ballot_size (zeroed unless
 * status[k] == EG_ST_OK) and gets status[k] =
 *   EG_ST_OK         packed;
 *   EG_ST_MALFORMED  does not deserialise: bad alphabet / padding / non-zero trailing bits / byte length != 32
 *                    (serde.rs:29-47,197,260), fewer than 2 ring_responses or ciphertext_responses (VecHelper<_, 2>, :303-355),
 *                    missing or duplicate field, sum_proof of the wrong kind;
 *   EG_PACK_RESHAPE  deserialises, but the number of choices / responses / partial ciphertexts is not the election's
 *                    (OptionsLenMismatch / LenMismatch, choice.rs:149-158, proofs/mod.rs:73-99): such objects go through the object
 *                    path (elastic_elgamal_amd/ingest.py), which applies the reference's order of checks.
 * Canonicity of scalars and validity of elements are decided later, by the GPU verifier (EG_ST_BAD_SCALAR / EG_ST_BAD_POINT with
 * the item index).  `threads` host threads parse in parallel.  *n_objects = number of objects found; EG_ERR_BAD_ARG if the text is
 * not a sequence of objects or holds more than max_objects of them. */
#define EG_PACK_RESHAPE 0xfffffffeu
int eg_choice_pack_json(int n_options, int single, const char* json, size_t json_len, int threads, size_t max_objects,
                        uint8_t* packed, uint32_t* status, size_t* n_objects);
int eg_qv_pack_json(int n_options, uint64_t credits, const char* json, size_t json_len, int threads, size_t max_objects,
                    uint8_t* packed, uint32_t* status, size_t* n_objects);
size_t eg_qv_ballot_size_for(int n_options, uint64_t credits);   /* eg_qv_ballot_size without a params object (host only) */

/* ---- the JSON text in PIECES (examples/voting.rs:195-198 prints ballots one at a time; src/serde.rs:19-80 is the layout) ----------------
 * eg_verify_{choice,qv}_json_begin opens a stream on a params object; eg_verify_json_feed takes the next piece of the text - ANY size, a
 * ballot (a string, an escape sequence) may straddle any number of pieces; the text as a whole is what eg_verify_*_json accepts: one JSON
 * array of objects, or objects back to back / one per line; eg_verify_json_end closes it.  Verdicts and tally are exactly those of the
 * one-shot entry on the concatenated text.
 *   feed   hands the piece to the stream's worker thread, which cuts it, packs its complete ballots on `threads` host threads into a
 *          pinned ring, and enqueues GPU work without waiting for it (the first submission once EG_JSON_FIRST_MIN ballots are packed, at
 *          most two in flight).  A piece below 8 MB is copied (one memcpy on the caller's thread; feed returns at once unless four 16 MB
 *          blocks - 64 MB of text - are already waiting); a larger piece is read in place and feed returns when the worker is through with it.  Either
 *          way nothing of `text` is referenced after feed returns.  *n_objects (may be NULL): complete objects the worker has cut so
 *          far - it may lag behind the pieces fed.  An error of the text (not a sequence of objects) or of the GPU found in a copied
 *          piece is reported by a LATER feed or take, and at the latest by end.
 *   take   (optional; waits at most for the worker to finish the window of the piece it is cutting - which, while the staging ring is
 *          full, includes the worker's own wait for the oldest submission - never for the GPU to drain) sends what has been copied so
 *          far to the worker, lets an idle GPU start on whatever is packed, and hands out, in order, the verdicts that are final so far: those of every ballot before the first one
 *          that is still on the GPU or whose shape is not the election's (such a ballot gets its OptionsLenMismatch / LenMismatch
 *          verdict from the object path, which runs at the end).
 *   end    waits for the GPU, resolves the ballots of another shape, writes the verdicts not yet taken (status: room for `cap`; if more
 *          are left the call fails with EG_ERR_BAD_ARG, *n_taken = the number that is left, and the stream stays open: call again with
 *          that much room, or abort), *n_objects = objects
 *          in the whole text, tally_out (may be NULL) = the tally of the STREAM's ballots; the params object's running tally has them
 *          added.  Destroys the stream - also when it reports an error of the text (not a sequence of objects, truncated) or of the GPU.
 *   abort  destroys the stream; the running tally is what it was before begin.  A failed feed leaves the stream dead: end returns the
 *          same error and cleans up, with the running tally as it was.
 * Host memory of a stream: the staging ring (EG_JSON_RING_KB), at most four 16 MB blocks of copied text, one status word per object, and the
 * TEXT of every ballot whose shape is not the election's (kept for the object path at the end): at most EG_JSON_ODD_MAX_MB (256 MB), beyond
 * which the stream fails with EG_ERR_NOMEM instead of buffering its input.
 * Between begin and end / abort the params object belongs to the stream: every other verify / tally call on it fails with EG_ERR_BAD_ARG
 * (the multi-GPU entries included: they refuse before they touch anything).
 * One stream per params object; several params objects (contexts, GPUs) may stream at the same time from different threads.
 * (The one-shot entries eg_verify_*_json run on the same pipeline, but a one-shot call is ONE call like any other: while it runs, calls of
 * other threads on the same params object - verify, tally, another one-shot, a begin - WAIT for it, they are not refused.) */
typedef struct eg_json_stream eg_json_stream;
int eg_verify_choice_json_begin(eg_choice_params*, int threads, eg_json_stream** out);
int eg_verify_qv_json_begin(eg_qv_params*, int threads, eg_json_stream** out);
int eg_verify_json_feed(eg_json_stream*, const char* text, size_t len, size_t* n_objects);
/* feed WITHOUT a copy and without waiting for the worker: the block stays the caller's memory but belongs to the library until it calls
 * release(user, text, len) - exactly once per successful call, from the stream's worker thread (or from the thread that ends / aborts the
 * stream, for blocks the worker never got to); release must not call back into the stream.  What a producer that receives the text in
 * its own buffers (a socket, a file mapping) uses: nothing is copied on its thread (eg_verify_json_feed copies a piece below 8 MB).
 * Returns at once unless ~64 MB of text are already waiting.  If the call FAILS, release is not called: the block is still the caller's. */
typedef void (*eg_json_release_fn)(void* user, const char* text, size_t len);
int eg_verify_json_feed_owned(eg_json_stream*, const char* text, size_t len, eg_json_release_fn release, void* user, size_t* n_objects);
/* a ready-made eg_json_release_fn: adds one to the size_t that `user` points to (atomically; NULL: does nothing).  For a caller that keeps its
 * blocks alive itself until the stream has ended and only wants to know that every block came back - and for bindings whose own callbacks
 * are expensive on a foreign thread (a Python callback takes the interpreter lock on the stream's worker thread, once per block). */
void eg_json_release_count(void* user, const char* text, size_t len);
int eg_verify_json_take(eg_json_stream*, uint32_t* status, size_t cap, size_t* n_taken);
int eg_verify_json_end(eg_json_stream*, uint32_t* status, size_t cap, size_t* n_taken, size_t* n_objects, uint8_t* tally_out);
void eg_verify_json_abort(eg_json_stream*);
/* JSON text -> verdicts and tally in one call (what a service that receives the output of examples/voting.rs:195-198 needs).  A pool of
 * `threads` host threads cuts the text into windows and packs them into a pinned ring (<= 1 GiB) while the calling thread uploads the
 * finished windows and enqueues their verification, two submissions in flight; memory: the ring, as much device staging, the chunk
 * workspace of the params object.  status[k]: the verify verdict of object k (as eg_verify_*_batch); EG_ST_MALFORMED for an object that
 * does not deserialise; for an object that deserialises with another shape than the election's, the reference's verdict from the object
 * path (EG_ST_OPTIONS_LEN, the LenMismatch variants, or whatever verify() says after them: src/app/choice.rs:358-380,
 * src/proofs/mod.rs:73-99).  Tally semantics as eg_verify_*_batch.  *n_objects = objects found; EG_ERR_BAD_ARG if the text is not a
 * sequence of JSON objects or holds more than max_objects (then no verdict of the call is valid; the call breaks off as soon as the parser
 * has cut one object too many - nothing further is parsed or verified). */
int eg_verify_choice_json(eg_choice_params*, const char* json, size_t json_len, int threads, size_t max_objects, uint32_t* status,
                          size_t* n_objects, uint8_t* tally_out);
int eg_verify_qv_json(eg_qv_params*, const char* json, size_t json_len, int threads, size_t max_objects, uint32_t* status,
                      size_t* n_objects, uint8_t* tally_out);

/* ---- the JSON entries over several GPUs of ONE process (the parser delivers 10 M ballots/s on 16 threads, one GPU verifies 6) ----
 * per_device[d]: params objects of the SAME election, each on its own context (as for eg_verify_*_batch_multi).  ONE parser - one splitter,
 * one pool of `threads` host threads - cuts and packs the text; every packed window (a few thousand ballots) goes to the params object with
 * the fewest ballots waiting or in flight, each of which has its own pinned ring, device staging and two submissions in flight (the pinned
 * budget of EG_JSON_RING_KB is divided among them, at least 128 MiB each).  status[k] is the verdict of object k of the TEXT, whichever GPU
 * verified it; every params object adds the accepted ballots of the windows it verified to its OWN running tally; tally_out = the tally of
 * the call's (the stream's) whole text, the lanes' tallies merged with the element addition of the primitive tier (eg_*_tally_encode_multi
 * sums the running tallies).  Ballots of another shape than the election's are resolved through the first object.  Everything else -
 * pieces of any size, feed / feed_owned / take / end / abort, errors, the params objects belonging to the stream - as for one object. */
int eg_verify_choice_json_multi(eg_choice_params* const* per_device, int n_dev, const char* json, size_t json_len, int threads, size_t max_objects,
                                uint32_t* status, size_t* n_objects, uint8_t* tally_out);
int eg_verify_qv_json_multi(eg_qv_params* const* per_device, int n_dev, const char* json, size_t json_len, int threads, size_t max_objects,
                            uint32_t* status, size_t* n_objects, uint8_t* tally_out);
int eg_verify_choice_json_begin_multi(eg_choice_params* const* per_device, int n_dev, int threads, eg_json_stream** out);
int eg_verify_qv_json_begin_multi(eg_qv_params* const* per_device, int n_dev, int threads, eg_json_stream** out);

/* ---- host-only introspection (no GPU needed; used by the CPU-side tests of the host logic) -------------------------------------
 * RangeDecomposition::optimal(upper_bound).to_string() (range.rs:110-124,148-305): the string hashed into the transcript */
int eg_range_decomposition(uint64_t upper_bound, char* buf, size_t cap);
/* JSON summary of the verification plan: kind 0 single-choice, 1 multi-choice, 2 quadratic voting (credits), 3 verify_zero,
 * 4 verify_bool, 5 verify_range (upper bound), 6 sum-of-squares proof over n_options values, 7 commitment-equivalence proof */
int eg_plan_describe(int kind, int n_options, uint64_t credits_or_bound, char* buf, size_t cap);

/* ---- re-encryption shuffles: verifying a mixer's proof (csrc/shuffle_kernels.cuh; no reference analogue) -----------------------------
 * Ballots that cannot be summed (ranked choice, write-ins) leave through a re-encryption mix-net: every mixer permutes and re-encrypts
 * the posted ciphertexts and proves it; anyone checks the proofs; the last mixer's outputs are decrypted with
 * eg_combine_shares_batch.  These entries CHECK such a proof - the Terelius-Wikstrom proof as restated by Haenni, Locher, Koenig and
 * Dubuis (the CHVote pseudo-code), additively over Ristretto255.  The model tests/shuffle_ref.py holds the same rule and a prover; a
 * prover entry is not part of the library.
 * FORMS.  A ciphertext is the 64 bytes R || B with R = [r]G, B = [m]G + [r]K (weeding's board layout), K the election key.  Rows are
 * zero-based, i = 0 .. N-1.  H32(x) = the first 32 bytes of SHA-512(x); MTH = the receipt log's tree over 32-byte leaves;
 * wide(x) = SHA-512(x) read as a little-endian integer mod l.  le64 / le32 are little-endian.
 * COMMITMENT KEY: H_0 .. H_cap, 32 bytes each (eg_shuffle_key_bytes(cap) = 32 (cap + 1)).  H_j = the first 32 bytes, top bit cleared, of
 *   SHA-512("eg-shuffle-v1/generator" || byte(seed_len) || seed || le64(j) || le32(ctr)) for the smallest ctr >= 0 at which those bytes
 * decode (the decoder's rule) to an element other than the identity; about one candidate in eight does.  A lane gives up after
 * EG_SHUFFLE_KEY_TRIES candidates: its 32 bytes are zero, the device form counts such lanes in *d_exhausted (uint32) and the host form
 * returns EG_ERR_BAD_ARG after writing the key.  A key derived for cap serves every N <= cap.
 * STATEMENT: in[N], out[N], K, the key and a per-call prefix of 0 .. 255 bytes (election id || mixer number).  PROOF: one blob of
 * eg_shuffle_proof_bytes(N) = 288 + 160 N bytes: the head t1 || t2 || t3 || t41 || t42 (points) || s1 || s2 || s3 || s4 (scalars), then
 * five planar arrays of N x 32 bytes: c (permutation commitment), c^ (chain), t^, s^, s'.
 * CHALLENGES.
 *   leaf1_i = H32(0x00 || in_i || out_i || c_i || H_(i+1)),  root1 = MTH(leaf1)
 *   seed1   = SHA-512("eg-shuffle-v1/seed" || byte(prefix_len) || prefix || le64(N) || K || H_0 || root1)       (all 64 bytes are used)
 *   u_i     = wide("eg-shuffle-v1/u" || seed1 || le64(i)),  u = the product of all u_i mod l
 *   leaf2_i = H32(0x00 || c^_i || t^_i),  root2 = MTH(leaf2)
 *   x       = wide("eg-shuffle-v1/c" || seed1 || root2 || t1 || t2 || t3 || t41 || t42)
 * The commitment key and N are inside the hash on purpose: commitment parameters left out of the Fiat-Shamir input broke a deployed
 * shuffle verifier in 2019.
 * EQUATIONS, with c^_(-1) = H_0, (R_i, B_i) = in_i, (R'_i, B'_i) = out_i, sums over all rows:
 *   T1     t1   = [-x](sum c_i - sum H_(i+1)) + [s1]G
 *   T2     t2   = [-x](c^_(N-1) - [u]H_0) + [s2]G
 *   T3     t3   = [-x] sum [u_i]c_i + [s3]G + sum [s'_i]H_(i+1)
 *   T41    t41  = [-x] sum [u_i]B_i - [s4]K + sum [s'_i]B'_i
 *   T42    t42  = [-x] sum [u_i]R_i - [s4]G + sum [s'_i]R'_i
 *   CHAIN  t^_i = [-x]c^_i + [s^_i]G + [s'_i]c^_(i-1)                                                           (one per row)
 * Equality is Ristretto equality: the canonical encoding of the right-hand side is compared with the given 32 bytes, as the Ed25519 pass
 * compares R.  The given side (t1 .. t42, t^_i) is never decoded, so a non-canonical t can never match.
 * VERDICT: one uint32 bit mask, 0 = accepted; bits, not "first failure", so the word does not depend on lane order.
 *   EG_SHUFFLE_BAD_ENCODING  some in, out, c, c^, H_0 .. H_N or K does not decode, or some scalar (s1 .. s4, s^_i, s'_i) is >= l.
 *                            Every other bit is then 0: products over undecodable inputs mean nothing.
 *   EG_SHUFFLE_T1 .. _T42    that equation fails
 *   EG_SHUFFLE_CHAIN         at least one row fails CHAIN
 * rows (optional uint32[N]): per row EG_SHUFFLE_ROW_BAD if in_i, out_i, c_i or c^_i does not decode or s^_i or s'_i is >= l;
 * EG_SHUFFLE_ROW_CHAIN if the row's CHAIN fails.  CHAIN of row i is evaluated only where c^_i and c^_(i-1) decode and s^_i, s'_i are
 * canonical (otherwise the bit is 0), whatever the verdict says.  found (uint32[4]): the rows with ROW_BAD, the rows with ROW_CHAIN, the
 * smallest index of each (0xffffffff for none).
 * STATELESS like the receipt log: the `_device` forms are asynchronous on `stream`, allocate nothing and never synchronise; K, prefix
 * and seed are HOST memory and are copied during the call.  The two roots come from eg_merkle_tree_device and the five sums from
 * eg_vartime_multi_mul_batch_device (which takes the context's lock for its launches): four products of 2N terms in one call, T2 and
 * [-s4]K in a second.  d_scratch holds eg_shuffle_verify_scratch_bytes(ctx, N) bytes, the product entry's own scratch included (545
 * bytes a row, 2304 bytes of tables for each lane of the chain kernel's grid - at most 1024 lanes a compute unit, 604 MB on 256 of them
 * whatever N - and, from 2N = 2^20 terms on, the bucket method's ~250 bytes a term).  The host forms do the same on
 * host arrays, synchronous, with their own staging.
 * EG_ERR_BAD_ARG before anything is launched: N or key_cap above EG_SHUFFLE_ROWS_MAX (2N terms must fit the product entry); N > key_cap;
 * prefix_len or seed_len > 255 or a NULL prefix / seed with a length; NULL verdict or found; with N > 0 a NULL in, out, K, key or proof;
 * arrays not 4-byte aligned; a scratch that is NULL, too small or not 16-byte aligned.  The argument rules come before the context is
 * looked at.  N == 0 is EG_OK with verdict 0 and found = {0, 0, 0xffffffff, 0xffffffff}.  TIMING: variable time; a proof is public. */
enum { EG_SHUFFLE_BAD_ENCODING = 1, EG_SHUFFLE_T1 = 2, EG_SHUFFLE_T2 = 4, EG_SHUFFLE_T3 = 8, EG_SHUFFLE_T41 = 16, EG_SHUFFLE_T42 = 32,
       EG_SHUFFLE_CHAIN = 64 };
enum { EG_SHUFFLE_ROW_BAD = 1, EG_SHUFFLE_ROW_CHAIN = 2 };
#define EG_SHUFFLE_ROWS_MAX (1u << 23)
#define EG_SHUFFLE_KEY_TRIES 4096
size_t eg_shuffle_key_bytes(uint64_t cap);                     /* 0 for cap > EG_SHUFFLE_ROWS_MAX */
size_t eg_shuffle_proof_bytes(uint64_t n);                     /* 0 for n > EG_SHUFFLE_ROWS_MAX */
int eg_shuffle_key_derive_device(eg_ctx*, const uint8_t* seed /* host */, size_t seed_len, uint64_t cap, void* d_key /* 32 (cap + 1) */,
                                 void* d_exhausted /* uint32 */, void* stream);
int eg_shuffle_key_derive(eg_ctx*, const uint8_t* seed, size_t seed_len, uint64_t cap, uint8_t* key /* 32 (cap + 1) */);
size_t eg_shuffle_verify_scratch_bytes(const eg_ctx*, uint64_t n);
int eg_shuffle_verify_device(eg_ctx*, uint64_t n, const void* d_in /* n x 64 */, const void* d_out /* n x 64 */, const uint8_t* K /* host, 32 */,
                             const uint8_t* prefix /* host */, size_t prefix_len, const void* d_key /* 32 (key_cap + 1) */, uint64_t key_cap,
                             const void* d_proof /* eg_shuffle_proof_bytes(n) */, void* d_verdict /* uint32 */, void* d_rows /* uint32[n] or NULL */,
                             void* d_found /* 4 x uint32 */, void* d_scratch, size_t scratch_bytes, void* stream);
int eg_shuffle_verify(eg_ctx*, uint64_t n, const uint8_t* in, const uint8_t* out, const uint8_t* K, const uint8_t* prefix, size_t prefix_len,
                      const uint8_t* key, uint64_t key_cap, const uint8_t* proof, uint32_t* verdict, uint32_t* rows /* or NULL */,
                      uint32_t* found /* 4 */);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------------------------------
 * Average duration in milliseconds of the dominant kernel (k_eq_table<false, T>: the ring equations) over the launches since the last reset,
 * measured with HIP events on the stream the kernel was launched on; launches = number of launches averaged.
 * enable = 2: also run the chunks of a call one after the other on one work set instead of alternating between two streams, so that a
 * launch shares the chip with nothing and its duration is its own (a measurement mode: slower, same results). */
int eg_profile_enable(eg_ctx*, int enable);
int eg_profile_read(eg_ctx*, double* msm_ms_total, uint64_t* msm_launches, double* all_ms_total);
/* same for the second kernel (k_base_tables), covering the launches folded in by the last eg_profile_read */
int eg_profile_read_tables(eg_ctx*, double* tables_ms_total, uint64_t* tables_launches);

/* The VALU roof of the box the library runs on: the shipped field multiplication (csrc/fe25519.cuh: fe_mul, the function the table and
 * equation kernels inline) in a bare dependent chain on changing operands, three waves per SIMD, launched back to back for `seconds`
 * (0 < seconds <= 30); *fmul_g_per_s = 10^9 multiplications per second chip-wide and *sclk_mhz (may be NULL) = the shader clock the chip
 * held (s_memtime / s_memrealtime), both over the second half of the run.  bench.py divides its achieved field-multiplication rate by this
 * figure (`valu_roofline.box`) instead of by a constant measured on another box of the pool.  The call holds the context for its length
 * (other threads' calls on the context wait) and keeps the whole chip busy: a measurement hook, not something to call beside production
 * work.  No reference analogue (the reference's own helper-multiplication benches: benches/basics.rs:284-319). */
int eg_selfbench_fmul(eg_ctx*, double seconds, double* fmul_g_per_s, double* sclk_mhz);

/* ---- self-check of the fixed-base comb tables (election setup; no reference analogue: dalek's basepoint table is a compile-time
 * constant) ---------------------------------------------------------------------------------------------------------------------
 * The tables of G are built on the device run by run with one batched inversion per run.  This recomputes `samples` entries (the
 * corners of windows and runs first, the rest drawn from `seed`) one at a time from the generator and counts the entries that differ.
 * wide = 0: the table built by eg_init (EG_COMB_BITS windows); wide = 1: the wide table that large batches use (built now if absent;
 * EG_ERR_NOMEM if it does not fit).  *mismatches must come back 0. */
int eg_selfcheck_generator_table(eg_ctx*, int wide, size_t samples, uint64_t seed, uint64_t* mismatches);
/* window widths of the generator's comb tables: the one built by eg_init, and the wide one (0 until an engine of this context has
 * verified enough items to get it, or eg_selfcheck_generator_table(wide = 1) built it) */
int eg_comb_table_bits(eg_ctx*, int* narrow_bits, int* wide_bits);

#ifdef __cplusplus
}
#endif
#endif
