"""The reference's verifiers on decoded objects, structured as the Rust is (slowli/elastic-elgamal; lines cited per item).

Scalars are integers below l, elements are point tuples of ristretto.py.  A failed verification raises VerificationError with
`kind` "challenge" or "len" (src/proofs/mod.rs:63-99); the application-level verifiers wrap it as the reference's enums do
(ChoiceVerificationError, QuadraticVotingError)."""
import math
from dataclasses import dataclass
from typing import Optional

from . import ristretto as R
from .field import L, scalar_from_wide
from .merlin import Transcript


# ------------------------------------------------------------------ src/proofs/mod.rs
class VerificationError(Exception):
    def __init__(self, kind: str, collection: str = ""):
        super().__init__(kind, collection)
        self.kind, self.collection = kind, collection


def check_lengths(collection: str, expected: int, actual: int) -> None:
    """mod.rs:84-98"""
    if expected != actual:
        raise VerificationError("len", collection)


def start_proof(t: Transcript, label: bytes) -> None:
    t.append_message(b"dom-sep", label)                  # mod.rs:40-42


def append_element_bytes(t: Transcript, label: bytes, element_bytes: bytes) -> None:
    t.append_message(label, element_bytes)               # mod.rs:44-46


def append_element(t: Transcript, label: bytes, element) -> None:
    append_element_bytes(t, label, R.encode(element))    # mod.rs:48-52: serialize_element, then the bytes


def challenge_scalar(t: Transcript, label: bytes) -> int:
    # mod.rs:54-56 -> Ristretto::scalar_from_random_bytes (group/ristretto.rs:34-38): 64 bytes, reduced
    return scalar_from_wide(t.challenge_bytes(label, 64))


# ------------------------------------------------------------------ keys, ciphertexts
@dataclass(frozen=True)
class PublicKey:
    """src/keys/mod.rs: an element together with its serialisation (`as_bytes` is what transcripts absorb)."""
    element: tuple
    bytes: bytes

    @classmethod
    def from_bytes(cls, b: bytes) -> Optional["PublicKey"]:
        """keys/mod.rs:161-176: invalid encodings and the identity are refused."""
        pt = R.decode(b)
        if pt is None or R.is_identity(pt):
            return None
        return cls(pt, bytes(b))

    @classmethod
    def from_element(cls, element) -> "PublicKey":
        return cls(element, R.encode(element))


@dataclass(frozen=True)
class Ciphertext:
    """src/encryption.rs: (random_element, blinded_element) = (R, B)."""
    random_element: tuple
    blinded_element: tuple

    @classmethod
    def zero(cls) -> "Ciphertext":
        return cls(R.IDENTITY, R.IDENTITY)

    def __add__(self, other: "Ciphertext") -> "Ciphertext":
        return Ciphertext(R.add(self.random_element, other.random_element), R.add(self.blinded_element, other.blinded_element))

    def __sub__(self, other: "Ciphertext") -> "Ciphertext":
        return Ciphertext(R.sub(self.random_element, other.random_element), R.sub(self.blinded_element, other.blinded_element))

    def to_bytes(self) -> bytes:
        """encryption.rs:155-160: R || B"""
        return R.encode(self.random_element) + R.encode(self.blinded_element)


# ------------------------------------------------------------------ src/proofs/log_equality.rs
@dataclass(frozen=True)
class LogEqualityProof:
    challenge: int
    response: int

    def verify(self, log_base: PublicKey, powers, transcript: Transcript) -> None:
        """log_equality.rs:153-180"""
        neg_challenge = -self.challenge % L
        commitments = (
            R.double_mul_generator(neg_challenge, powers[0], self.response),
            R.multi_mul((neg_challenge, self.response), (powers[1], log_base.element)),
        )
        start_proof(transcript, b"log_eq")
        append_element_bytes(transcript, b"K", log_base.bytes)
        append_element(transcript, b"[r]G", powers[0])
        append_element(transcript, b"[r]K", powers[1])
        append_element(transcript, b"[x]G", commitments[0])
        append_element(transcript, b"[x]K", commitments[1])
        if challenge_scalar(transcript, b"c") != self.challenge:
            raise VerificationError("challenge")


# ------------------------------------------------------------------ src/proofs/ring.rs
@dataclass(frozen=True)
class RingProof:
    common_challenge: int
    ring_responses: tuple

    def total_rings_size(self) -> int:
        return len(self.ring_responses)                  # ring.rs:376-378

    def verify(self, receiver: PublicKey, admissible_values, ciphertexts, transcript: Transcript) -> None:
        """ring.rs:302-374.  admissible_values: one sequence of elements per ring; ciphertexts: one per ring."""
        admissible_values = list(admissible_values)
        total_rings_size = sum(len(values) for values in admissible_values)
        check_lengths("items in all rings", self.total_rings_size(), total_rings_size)          # :310-315

        start_proof(transcript, b"multi_ring_enc")                                              # :290-293
        append_element_bytes(transcript, b"K", receiver.bytes)
        initial_ring_transcript = transcript.clone()                                            # :320

        starting_response = 0
        for ring_index, (values, ciphertext) in enumerate(zip(admissible_values, ciphertexts)):
            challenge = self.common_challenge
            commitments = (R.BASEPOINT, R.BASEPOINT)                                            # :326, never absorbed for a non-empty ring
            ring_transcript = initial_ring_transcript.clone()
            start_proof(ring_transcript, b"ring_enc")
            ring_transcript.append_message(b"enc", ciphertext.to_bytes())
            ring_transcript.append_u64(b"i", ring_index)
            responses = self.ring_responses[starting_response:]
            for eq_index, (admissible_value, response) in enumerate(zip(values, responses)):
                dh_element = R.sub(ciphertext.blinded_element, admissible_value)
                neg_challenge = -challenge % L
                commitments = (
                    R.double_mul_generator(neg_challenge, ciphertext.random_element, response),
                    R.multi_mul((response, neg_challenge), (receiver.element, dh_element)),
                )
                if eq_index + 1 < len(values):                                                  # :354-360
                    eq_transcript = ring_transcript.clone()
                    eq_transcript.append_u64(b"j", eq_index)
                    append_element(eq_transcript, b"R_G", commitments[0])
                    append_element(eq_transcript, b"R_K", commitments[1])
                    challenge = challenge_scalar(eq_transcript, b"c")
            starting_response += len(values)
            append_element(transcript, b"R_G", commitments[0])                                  # :364-365
            append_element(transcript, b"R_K", commitments[1])

        if challenge_scalar(transcript, b"c") != self.common_challenge:                         # :368-373
            raise VerificationError("challenge")


# ------------------------------------------------------------------ src/proofs/range.rs
@dataclass(frozen=True)
class RingSpec:
    size: int
    step: int


class RangeDecomposition:
    """range.rs:105-324"""

    def __init__(self, rings):
        self.rings = list(rings)

    def __str__(self) -> str:
        """range.rs:110-124: the string the range proof's transcript absorbs"""
        parts = []
        for spec in self.rings:
            parts.append((f"{spec.step} * " if spec.step > 1 else "") + f"0..{spec.size}")
        return " + ".join(parts)

    @classmethod
    def just(cls, capacity: int) -> "RangeDecomposition":
        return cls([RingSpec(capacity, 1)])                                                     # :155-161

    def combine_mul(self, new_ring_size: int, multiplier: int) -> "RangeDecomposition":
        """:163-176: the inner rings keep their order in FRONT, scaled; the new ring of step 1 goes LAST"""
        return RangeDecomposition([RingSpec(s.size, s.step * multiplier) for s in self.rings] + [RingSpec(new_ring_size, 1)])

    def upper_bound(self) -> int:
        return sum((s.size - 1) * s.step for s in self.rings) + 1                               # :179-185

    def rings_size(self) -> int:
        return sum(s.size for s in self.rings)                                                  # :188-190

    @staticmethod
    def lower_len_estimate(upper_bound: int) -> int:
        return math.ceil(math.log2(float(upper_bound)) * 3.0)                                   # :302-305 (the std build)

    @classmethod
    def optimal(cls, upper_bound: int) -> "RangeDecomposition":
        assert upper_bound >= 2                                                                 # :149
        return cls._optimize(upper_bound, {})[1]

    @classmethod
    def _optimize(cls, upper_bound: int, optimal_values: dict):
        """:238-300; returns (optimal_len, decomposition)"""
        if upper_bound in optimal_values:
            return optimal_values[upper_bound]
        opt_len, opt = upper_bound + 2, cls.just(upper_bound)
        first_ring_size = 2
        while first_ring_size + 2 <= opt_len:                                                   # :251-255
            remaining_capacity = upper_bound - first_ring_size
            for multiplier in range(2, first_ring_size + 1):
                if remaining_capacity % multiplier != 0:
                    continue
                inner_upper_bound = remaining_capacity // multiplier + 1
                if inner_upper_bound < 2:
                    break
                if first_ring_size + 2 + cls.lower_len_estimate(inner_upper_bound) > opt_len:
                    continue
                inner_len, inner = cls._optimize(inner_upper_bound, optimal_values)
                candidate_len = first_ring_size + 2 + inner_len
                candidate_rings = 1 + len(inner.rings)
                # :279-281: strictly shorter, or as short with strictly fewer rings; the first such candidate stays
                if candidate_len < opt_len or (candidate_len == opt_len and candidate_rings < len(opt.rings)):
                    opt_len, opt = candidate_len, inner.combine_mul(first_ring_size, multiplier)
            first_ring_size += 1
        optimal_values[upper_bound] = (opt_len, opt)
        return opt_len, opt


class PreparedRange:
    """range.rs:329-355: the decomposition with [i * step]G for every ring"""

    def __init__(self, decomposition: RangeDecomposition):
        self.inner = decomposition
        self.admissible_values = []
        multiples = {0: R.IDENTITY}

        def multiple(k: int):
            if k not in multiples:
                multiples[k] = R.mul_generator(k)
            return multiples[k]

        for spec in decomposition.rings:
            step_g = multiple(spec.step)
            values = [R.IDENTITY]
            for _ in range(1, spec.size):
                values.append(R.add(values[-1], step_g))  # [i * step]G, :344-346
            self.admissible_values.append(values)


@dataclass(frozen=True)
class RangeProof:
    partial_ciphertexts: tuple
    inner: RingProof

    def verify(self, receiver: PublicKey, prepared: PreparedRange, ciphertext: Ciphertext, transcript: Transcript) -> None:
        """range.rs:547-577"""
        check_lengths("admissible values", len(self.partial_ciphertexts) + 1, len(prepared.admissible_values))   # :555-559
        start_proof(transcript, b"encryption_range_proof")
        transcript.append_message(b"range", str(prepared.inner).encode())
        ciphertext_sum = Ciphertext.zero()
        for partial in self.partial_ciphertexts:
            ciphertext_sum = ciphertext_sum + partial
        ciphertexts = list(self.partial_ciphertexts) + [ciphertext - ciphertext_sum]            # :568-572
        self.inner.verify(receiver, prepared.admissible_values, ciphertexts, transcript)


# ------------------------------------------------------------------ src/proofs/mul.rs
@dataclass(frozen=True)
class SumOfSquaresProof:
    challenge: int
    ciphertext_responses: tuple
    sum_response: int

    def verify(self, ciphertexts, sum_of_squares_ciphertext: Ciphertext, receiver: PublicKey, transcript: Transcript) -> None:
        """mul.rs:190-260"""
        ciphertexts = list(ciphertexts)
        check_lengths("ciphertext responses", len(self.ciphertext_responses), len(ciphertexts) * 2)            # :197-202
        start_proof(transcript, b"sum_of_squares")                                              # :96-99
        append_element_bytes(transcript, b"K", receiver.bytes)
        neg_challenge = -self.challenge % L
        for index, ciphertext in enumerate(ciphertexts):
            r_response, v_response = self.ciphertext_responses[2 * index], self.ciphertext_responses[2 * index + 1]
            append_element(transcript, b"R_x", ciphertext.random_element)
            append_element(transcript, b"X", ciphertext.blinded_element)
            random_commitment = R.double_mul_generator(neg_challenge, ciphertext.random_element, r_response)
            append_element(transcript, b"[e_r]G", random_commitment)
            value_commitment = R.multi_mul((v_response, r_response, neg_challenge),
                                           (R.BASEPOINT, receiver.element, ciphertext.blinded_element))
            append_element(transcript, b"[e_x]G + [e_r]K", value_commitment)
        # :232-247: the odd-indexed responses (the value responses), then the sum response, then -challenge
        scalars = list(self.ciphertext_responses[1::2]) + [self.sum_response, neg_challenge]
        random_sum_commitment = R.multi_mul(
            scalars, [c.random_element for c in ciphertexts] + [R.BASEPOINT, sum_of_squares_ciphertext.random_element])
        value_sum_commitment = R.multi_mul(
            scalars, [c.blinded_element for c in ciphertexts] + [receiver.element, sum_of_squares_ciphertext.blinded_element])
        append_element(transcript, b"R_z", sum_of_squares_ciphertext.random_element)
        append_element(transcript, b"Z", sum_of_squares_ciphertext.blinded_element)
        append_element(transcript, b"[e_x]R_x + [e_z]G", random_sum_commitment)
        append_element(transcript, b"[e_x]X + [e_z]K", value_sum_commitment)
        if challenge_scalar(transcript, b"c") != self.challenge:
            raise VerificationError("challenge")


# ------------------------------------------------------------------ src/proofs/commitment.rs
@dataclass(frozen=True)
class CommitmentEquivalenceProof:
    challenge: int
    randomness_response: int
    value_response: int
    commitment_response: int

    def verify(self, ciphertext: Ciphertext, receiver: PublicKey, commitment, commitment_blinding_base, transcript: Transcript) -> None:
        """commitment.rs:186-238"""
        start_proof(transcript, b"commitment_equivalence")
        append_element_bytes(transcript, b"K", receiver.bytes)
        append_element(transcript, b"R", ciphertext.random_element)
        append_element(transcript, b"B", ciphertext.blinded_element)
        append_element(transcript, b"C", commitment)
        neg_challenge = -self.challenge % L
        random_commitment = R.double_mul_generator(neg_challenge, ciphertext.random_element, self.randomness_response)
        append_element(transcript, b"[e_r]G", random_commitment)
        enc_blinding_commitment = R.multi_mul((self.value_response, self.randomness_response, neg_challenge),
                                              (R.BASEPOINT, receiver.element, ciphertext.blinded_element))
        append_element(transcript, b"[e_v]G + [e_r]K", enc_blinding_commitment)
        commitment_commitment = R.multi_mul((self.value_response, self.commitment_response, neg_challenge),
                                            (R.BASEPOINT, commitment_blinding_base, commitment))
        append_element(transcript, b"[e_v]G + [e_c]H", commitment_commitment)
        if challenge_scalar(transcript, b"c") != self.challenge:
            raise VerificationError("challenge")


# ------------------------------------------------------------------ src/keys/impls.rs
BOOL_VALUES = (R.IDENTITY, R.BASEPOINT)


def verify_zero(receiver: PublicKey, ciphertext: Ciphertext, proof: LogEqualityProof) -> None:
    """impls.rs:59-69"""
    proof.verify(receiver, (ciphertext.random_element, ciphertext.blinded_element), Transcript(b"zero_encryption"))


def verify_bool(receiver: PublicKey, ciphertext: Ciphertext, proof: RingProof) -> None:
    """impls.rs:101-113"""
    proof.verify(receiver, [BOOL_VALUES], [ciphertext], Transcript(b"bool_encryption"))


def verify_range(receiver: PublicKey, prepared: PreparedRange, ciphertext: Ciphertext, proof: RangeProof) -> None:
    """impls.rs:143-151"""
    proof.verify(receiver, prepared, ciphertext, Transcript(b"ciphertext_range"))


# ------------------------------------------------------------------ src/sharing/key_set.rs
def verify_share(shares: int, threshold: int, shared_key: PublicKey, key_share, dh_element, ciphertext_random_element, index: int,
                 proof: LogEqualityProof) -> None:
    """key_set.rs:209-228 with commit() of :167-171.  key_share = participant_keys[index] as an element."""
    transcript = Transcript(b"elgamal_decryption_share")
    transcript.append_u64(b"n", shares)
    transcript.append_u64(b"t", threshold)
    append_element_bytes(transcript, b"K", shared_key.bytes)
    transcript.append_u64(b"i", index)
    proof.verify(PublicKey.from_element(ciphertext_random_element), (key_share, dh_element), transcript)


# ------------------------------------------------------------------ src/app/choice.rs
class ChoiceVerificationError(Exception):
    """choice.rs:407-419: which = "options_len" | "sum" | "range"; `error` the VerificationError underneath"""

    def __init__(self, which: str, error: Optional[VerificationError] = None):
        super().__init__(which, error)
        self.which, self.error = which, error


@dataclass(frozen=True)
class ChoiceParams:
    receiver: PublicKey
    options_count: int
    single: bool


@dataclass(frozen=True)
class EncryptedChoice:
    choices: tuple
    range_proof: RingProof
    sum_proof: Optional[LogEqualityProof]

    def verify(self, params: ChoiceParams):
        """choice.rs:358-380; returns the choice ciphertexts"""
        if params.options_count != len(self.choices):                                           # :362, :149-158
            raise ChoiceVerificationError("options_len")
        sum_of_ciphertexts = self.choices[0]
        for choice in self.choices[1:]:
            sum_of_ciphertexts = sum_of_ciphertexts + choice
        if params.single:                                                                       # :366-368 -> :77-94
            powers = (sum_of_ciphertexts.random_element, R.sub(sum_of_ciphertexts.blinded_element, R.BASEPOINT))
            try:
                self.sum_proof.verify(params.receiver, powers, Transcript(b"choice_encryption_sum"))
            except VerificationError as e:
                raise ChoiceVerificationError("sum", e) from None
        try:
            self.range_proof.verify(params.receiver, [BOOL_VALUES] * len(self.choices), self.choices,
                                    Transcript(b"encrypted_choice_ranges"))
        except VerificationError as e:
            raise ChoiceVerificationError("range", e) from None
        return self.choices


# ------------------------------------------------------------------ src/app/quadratic_voting.rs
class QuadraticVotingError(Exception):
    """quadratic_voting.rs:335-354: which = "options_len" | "variant" (with index) | "credit_range" | "credit_equivalence" """

    def __init__(self, which: str, error: Optional[VerificationError] = None, index: int = 0):
        super().__init__(which, error, index)
        self.which, self.error, self.index = which, error, index


def isqrt(x: int) -> int:
    """quadratic_voting.rs:127-143"""
    root, power_of_4 = 0, 1 << 62
    while power_of_4 > x:
        power_of_4 //= 4
    while power_of_4 > 0:
        if x >= root + power_of_4:
            x -= root + power_of_4
            root = root // 2 + power_of_4
        else:
            root //= 2
        power_of_4 //= 4
    return root


class QuadraticVotingParams:
    """quadratic_voting.rs:63-76"""

    def __init__(self, receiver: PublicKey, options: int, credits: int):
        assert options > 0 and credits > 0
        self.vote_count_range = PreparedRange(RangeDecomposition.optimal(isqrt(credits) + 1))
        self.credit_range = PreparedRange(RangeDecomposition.optimal(credits + 1))
        self.options_count = options
        self.receiver = receiver


@dataclass(frozen=True)
class CiphertextWithRangeProof:
    ciphertext: Ciphertext
    range_proof: RangeProof


@dataclass(frozen=True)
class QuadraticVotingBallot:
    votes: tuple
    credit: CiphertextWithRangeProof
    credit_equivalence_proof: SumOfSquaresProof

    def verify(self, params: QuadraticVotingParams):
        """quadratic_voting.rs:291-329; returns the vote ciphertexts"""
        if params.options_count != len(self.votes):
            raise QuadraticVotingError("options_len")
        for i, vote_count in enumerate(self.votes):
            try:
                vote_count.range_proof.verify(params.receiver, params.vote_count_range, vote_count.ciphertext,
                                              Transcript(b"quadratic_voting_variant"))
            except VerificationError as e:
                raise QuadraticVotingError("variant", e, i) from None
        try:
            self.credit.range_proof.verify(params.receiver, params.credit_range, self.credit.ciphertext,
                                           Transcript(b"quadratic_voting_credit_range"))
        except VerificationError as e:
            raise QuadraticVotingError("credit_range", e) from None
        try:
            self.credit_equivalence_proof.verify([v.ciphertext for v in self.votes], self.credit.ciphertext, params.receiver,
                                                 Transcript(b"quadratic_voting_credit_equiv"))
        except VerificationError as e:
            raise QuadraticVotingError("credit_equivalence", e) from None
        return [v.ciphertext for v in self.votes]
