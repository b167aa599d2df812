"""The project boundary (include/eg_hip.h): packed items -> the full status word, and the tally of the accepted ballots.

A packed object is a run of 32-byte items whose shape the verifier's parameters fix.  The status word has the kind in its low byte
and the detail above (EG_STATUS_KIND / EG_STATUS_DETAIL).  Precedence, as the header states it: first the deserialisation-time
rejections of serde in WIRE ORDER -- the first item that is no canonical scalar (BAD_SCALAR) or no element (BAD_POINT), with its
item index as detail --, then the order of checks of the reference's own verify().

Every verifier class has `layout` (a string of "P" / "S", one letter an item), `size` and `verify(blob) -> status word`; the
election verifiers also have `tally(blobs, words)`."""
from . import protocol as proto
from . import ristretto as R
from .field import scalar_from_canonical_bytes
from .merlin import Transcript

OK, BAD_SCALAR, BAD_POINT, OPTIONS_LEN, SUM_CHALLENGE, RANGE_LEN, RANGE_CHALLENGE = range(7)
QV_VARIANT_LEN, QV_VARIANT_CHALLENGE, QV_CREDIT_RANGE_LEN, QV_CREDIT_RANGE_CHALLENGE = 7, 8, 9, 10
QV_CREDIT_EQUIV_LEN, QV_CREDIT_EQUIV_CHALLENGE = 11, 12


def status(kind: int, detail: int = 0) -> int:
    return kind | (detail << 8)


def split(blob: bytes) -> list:
    assert len(blob) % 32 == 0
    return [blob[i : i + 32] for i in range(0, len(blob), 32)]


def deserialize(layout: str, blob: bytes):
    """(status word, None) for the first malformed item in wire order, else (0, decoded items): integers for "S", points for "P"."""
    items = split(blob)
    assert len(items) == len(layout), (len(items), len(layout))
    out = []
    for index, (kind, item) in enumerate(zip(layout, items)):
        if kind == "P":
            value = R.decode(item)                       # ElementHelper, src/serde.rs:254-269
            if value is None:
                return status(BAD_POINT, index), None
        else:
            value = scalar_from_canonical_bytes(item)    # ScalarHelper, src/serde.rs:191-206
            if value is None:
                return status(BAD_SCALAR, index), None
        out.append(value)
    return OK, out


def _word(error: proto.VerificationError, on_len: int, on_challenge: int, detail: int = 0) -> int:
    return status(on_len if error.kind == "len" else on_challenge, detail)


def choice_status(error: proto.ChoiceVerificationError) -> int:
    if error.which == "options_len":
        return status(OPTIONS_LEN)
    if error.which == "sum":
        return _word(error.error, SUM_CHALLENGE, SUM_CHALLENGE)      # a log-equality proof has no length to mismatch
    return _word(error.error, RANGE_LEN, RANGE_CHALLENGE)


def qv_status(error: proto.QuadraticVotingError) -> int:
    if error.which == "options_len":
        return status(OPTIONS_LEN)
    if error.which == "variant":
        return _word(error.error, QV_VARIANT_LEN, QV_VARIANT_CHALLENGE, error.index)
    if error.which == "credit_range":
        return _word(error.error, QV_CREDIT_RANGE_LEN, QV_CREDIT_RANGE_CHALLENGE)
    return _word(error.error, QV_CREDIT_EQUIV_LEN, QV_CREDIT_EQUIV_CHALLENGE)


def _ct(values, at: int) -> proto.Ciphertext:
    return proto.Ciphertext(values[at], values[at + 1])


def _sum_encoded(columns) -> bytes:
    """columns: per tally slot, the list of ciphertexts to add; the encoding of each sum, R || B (zero: 64 zero bytes)."""
    out = b""
    for cts in columns:
        total = proto.Ciphertext.zero()
        for c in cts:
            total = total + c
        out += total.to_bytes()
    return out


def range_layout(decomposition: proto.RangeDecomposition) -> str:
    """ciphertext || partial ciphertexts (one fewer than rings) || common challenge || responses (eg_hip.h, "single-ciphertext proofs")"""
    return "P" * (2 * len(decomposition.rings)) + "S" * (1 + decomposition.rings_size())


def _range_block(values, n_rings: int, n_responses: int):
    """the decoded items of one `ciphertext || range proof` block -> (Ciphertext, RangeProof)"""
    ciphertext = _ct(values, 0)
    partials = tuple(_ct(values, 2 + 2 * i) for i in range(n_rings - 1))
    e0 = 2 * n_rings
    ring = proto.RingProof(values[e0], tuple(values[e0 + 1 : e0 + 1 + n_responses]))
    return ciphertext, proto.RangeProof(partials, ring)


class _Verifier:
    layout = ""

    @property
    def size(self) -> int:
        return 32 * len(self.layout)

    def verify(self, blob: bytes) -> int:
        word, values = deserialize(self.layout, blob)
        if word != OK:
            return word
        return self._verify(values)


class ChoiceVerifier(_Verifier):
    """n_options x (R || B) || e0 || 2 n_options responses || [challenge || response] (eg_hip.h, "batch tier: EncryptedChoice")"""

    def __init__(self, public_key: bytes, n_options: int, single: bool):
        receiver = proto.PublicKey.from_bytes(public_key)
        assert receiver is not None and n_options > 0
        self.params = proto.ChoiceParams(receiver, n_options, single)
        self.n_options, self.single = n_options, single
        self.layout = "P" * (2 * n_options) + "S" * (1 + 2 * n_options + (2 if single else 0))

    def parse(self, values) -> proto.EncryptedChoice:
        n = self.n_options
        choices = tuple(_ct(values, 2 * i) for i in range(n))
        ring = proto.RingProof(values[2 * n], tuple(values[2 * n + 1 : 4 * n + 1]))
        sum_proof = proto.LogEqualityProof(values[4 * n + 1], values[4 * n + 2]) if self.single else None
        return proto.EncryptedChoice(choices, ring, sum_proof)

    def _verify(self, values) -> int:
        try:
            self.parse(values).verify(self.params)
        except proto.ChoiceVerificationError as e:
            return choice_status(e)
        return OK

    def tally(self, blobs, words) -> bytes:
        columns = [[] for _ in range(self.n_options)]
        for blob, word in zip(blobs, words):
            if word == OK:
                items = split(blob)
                for k in range(self.n_options):
                    columns[k].append(proto.Ciphertext(R.decode(items[2 * k]), R.decode(items[2 * k + 1])))
        return _sum_encoded(columns)


class QvVerifier(_Verifier):
    """n_options vote blocks, the credit block, challenge || 2 n_options responses || sum response (eg_hip.h, "batch tier:
    QuadraticVotingBallot")"""

    def __init__(self, public_key: bytes, n_options: int, credits: int):
        receiver = proto.PublicKey.from_bytes(public_key)
        assert receiver is not None
        self.params = proto.QuadraticVotingParams(receiver, n_options, credits)
        self.n_options, self.credits = n_options, credits
        self.vote_dec = self.params.vote_count_range.inner
        self.credit_dec = self.params.credit_range.inner
        self.vote_layout, self.credit_layout = range_layout(self.vote_dec), range_layout(self.credit_dec)
        self.layout = self.vote_layout * n_options + self.credit_layout + "S" * (2 * n_options + 2)

    def parse(self, values) -> proto.QuadraticVotingBallot:
        n, vs = self.n_options, len(self.vote_layout)
        votes = []
        for i in range(n):
            ct, rp = _range_block(values[i * vs : (i + 1) * vs], len(self.vote_dec.rings), self.vote_dec.rings_size())
            votes.append(proto.CiphertextWithRangeProof(ct, rp))
        at = n * vs
        ct, rp = _range_block(values[at : at + len(self.credit_layout)], len(self.credit_dec.rings), self.credit_dec.rings_size())
        at += len(self.credit_layout)
        sumsq = proto.SumOfSquaresProof(values[at], tuple(values[at + 1 : at + 1 + 2 * n]), values[at + 1 + 2 * n])
        return proto.QuadraticVotingBallot(tuple(votes), proto.CiphertextWithRangeProof(ct, rp), sumsq)

    def _verify(self, values) -> int:
        try:
            self.parse(values).verify(self.params)
        except proto.QuadraticVotingError as e:
            return qv_status(e)
        return OK

    def tally(self, blobs, words) -> bytes:
        columns = [[] for _ in range(self.n_options)]
        vs = len(self.vote_layout)
        for blob, word in zip(blobs, words):
            if word == OK:
                items = split(blob)
                for k in range(self.n_options):
                    columns[k].append(proto.Ciphertext(R.decode(items[k * vs]), R.decode(items[k * vs + 1])))
        return _sum_encoded(columns)


class ZeroVerifier(_Verifier):
    """ciphertext || challenge || response; ChallengeMismatch is EG_ST_SUM_CHALLENGE"""
    layout = "PPSS"

    def __init__(self, public_key: bytes):
        self.receiver = proto.PublicKey.from_bytes(public_key)
        assert self.receiver is not None

    def _verify(self, values) -> int:
        try:
            proto.verify_zero(self.receiver, _ct(values, 0), proto.LogEqualityProof(values[2], values[3]))
        except proto.VerificationError:
            return status(SUM_CHALLENGE)
        return OK


class BoolVerifier(_Verifier):
    """ciphertext || e0 || s0 || s1; ChallengeMismatch is EG_ST_RANGE_CHALLENGE"""
    layout = "PPSSS"

    def __init__(self, public_key: bytes):
        self.receiver = proto.PublicKey.from_bytes(public_key)
        assert self.receiver is not None

    def _verify(self, values) -> int:
        try:
            proto.verify_bool(self.receiver, _ct(values, 0), proto.RingProof(values[2], (values[3], values[4])))
        except proto.VerificationError as e:
            return _word(e, RANGE_LEN, RANGE_CHALLENGE)
        return OK


class RangeVerifier(_Verifier):
    """ciphertext || partial ciphertexts || e0 || responses with RangeDecomposition::optimal(upper_bound)"""

    def __init__(self, public_key: bytes, upper_bound: int):
        self.receiver = proto.PublicKey.from_bytes(public_key)
        assert self.receiver is not None
        self.decomposition = proto.RangeDecomposition.optimal(upper_bound)
        self.prepared = proto.PreparedRange(self.decomposition)
        self.layout = range_layout(self.decomposition)

    def _verify(self, values) -> int:
        ct, rp = _range_block(values, len(self.decomposition.rings), self.decomposition.rings_size())
        try:
            proto.verify_range(self.receiver, self.prepared, ct, rp)
        except proto.VerificationError as e:
            return _word(e, RANGE_LEN, RANGE_CHALLENGE)
        return OK


class ShareVerifier(_Verifier):
    """R (the ciphertext's random element) || dh || challenge || response for one participant; EG_ST_SUM_CHALLENGE"""
    layout = "PPSS"

    def __init__(self, shared_key: bytes, shares: int, threshold: int, index: int, participant_key: bytes):
        self.shared_key = proto.PublicKey.from_bytes(shared_key)
        self.key_share = R.decode(participant_key)
        assert self.shared_key is not None and self.key_share is not None
        self.shares, self.threshold, self.index = shares, threshold, index

    def _verify(self, values) -> int:
        try:
            proto.verify_share(self.shares, self.threshold, self.shared_key, self.key_share, values[1], values[0], self.index,
                               proto.LogEqualityProof(values[2], values[3]))
        except proto.VerificationError:
            return status(SUM_CHALLENGE)
        return OK


class SumOfSquaresVerifier(_Verifier):
    """n value ciphertexts || sum-of-squares ciphertext || challenge || 2 n responses || sum response under Transcript::new(label);
    ChallengeMismatch is EG_ST_QV_CREDIT_EQUIV_CHALLENGE"""

    def __init__(self, public_key: bytes, n_values: int, label: bytes):
        self.receiver = proto.PublicKey.from_bytes(public_key)
        assert self.receiver is not None
        self.n, self.label = n_values, label
        self.layout = "P" * (2 * n_values + 2) + "S" * (2 * n_values + 2)

    def _verify(self, values) -> int:
        n = self.n
        cts = [_ct(values, 2 * i) for i in range(n)]
        at = 2 * n + 2
        proof = proto.SumOfSquaresProof(values[at], tuple(values[at + 1 : at + 1 + 2 * n]), values[at + 1 + 2 * n])
        try:
            proof.verify(cts, _ct(values, 2 * n), self.receiver, Transcript(self.label))
        except proto.VerificationError as e:
            return _word(e, QV_CREDIT_EQUIV_LEN, QV_CREDIT_EQUIV_CHALLENGE)
        return OK


class CommitmentEquivalenceVerifier(_Verifier):
    """R || B || C || challenge || randomness, value, commitment responses under Transcript::new(label); EG_ST_SUM_CHALLENGE"""
    layout = "PPPSSSS"

    def __init__(self, public_key: bytes, blinding_base: bytes, label: bytes):
        self.receiver = proto.PublicKey.from_bytes(public_key)
        self.blinding_base = R.decode(blinding_base)
        assert self.receiver is not None and self.blinding_base is not None
        self.label = label

    def _verify(self, values) -> int:
        proof = proto.CommitmentEquivalenceProof(*values[3:7])
        try:
            proof.verify(_ct(values, 0), self.receiver, values[2], self.blinding_base, Transcript(self.label))
        except proto.VerificationError:
            return status(SUM_CHALLENGE)
        return OK
