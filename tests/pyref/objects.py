"""The reference's own object form: serde's layout in a human-readable format, every scalar and element an unpadded base64url
string (src/serde.rs:19-80), structures as derived on EncryptedChoice (src/app/choice.rs:276-280), RingProof
(src/proofs/ring.rs:282-287), LogEqualityProof (src/proofs/log_equality.rs:96-101), QuadraticVotingBallot and
CiphertextWithRangeProof (src/app/quadratic_voting.rs:205-217), RangeProof (src/proofs/range.rs:446-450, `inner` flattened),
SumOfSquaresProof (src/proofs/mul.rs:86-93), Ciphertext (src/encryption.rs).

An object is walked in the order its structs declare their fields (NOT the order of keys in a document); that walk is the wire
order of the packed form, so `pack` gives the packed bytes and `verify_*` the status word of an object of ANY shape, including
the length mismatches a packed batch cannot express."""
import base64
import binascii

from . import packed as pk
from . import protocol as proto

MALFORMED = 13                                           # EG_ST_MALFORMED: the object does not deserialise at all


class Malformed(ValueError):
    pass


def b64url(text) -> bytes:
    """serde.rs:29-47: unpadded URL-safe base64 of exactly 32 bytes"""
    if not isinstance(text, str) or "=" in text:
        raise Malformed("expected an unpadded base64url string")
    try:
        raw = base64.urlsafe_b64decode(text + "=" * (-len(text) % 4))
    except (binascii.Error, ValueError):
        raise Malformed("invalid base64url") from None
    if base64.urlsafe_b64encode(raw).rstrip(b"=").decode() != text or len(raw) != 32:
        raise Malformed("non-canonical string or wrong byte length")
    return raw


class _Walk:
    """Collects (kind, bytes) in wire order."""

    def __init__(self):
        self.kinds, self.items = [], []

    def scalar(self, text):
        self.kinds.append("S")
        self.items.append(b64url(text))

    def ciphertext(self, obj):
        for field in ("random_element", "blinded_element"):
            self.kinds.append("P")
            self.items.append(b64url(obj[field]))

    def scalars(self, texts, minimum=2):
        if len(texts) < minimum:                         # VecHelper<_, 2>, serde.rs:303-355
            raise Malformed("too few items")
        for t in texts:
            self.scalar(t)

    def ring_proof(self, obj):
        self.scalar(obj["common_challenge"])
        self.scalars(obj["ring_responses"])

    def range_block(self, ciphertext, range_proof):
        self.ciphertext(ciphertext)
        for partial in range_proof["partial_ciphertexts"]:
            self.ciphertext(partial)
        self.ring_proof(range_proof)

    def decoded(self):
        return pk.deserialize("".join(self.kinds), b"".join(self.items))


def _walk_choice(obj, single: bool) -> _Walk:
    w = _Walk()
    for c in obj["choices"]:
        w.ciphertext(c)
    w.ring_proof(obj["range_proof"])
    sp = obj.get("sum_proof")
    if single != (sp is not None):
        raise Malformed("sum_proof of the wrong kind")
    if single:
        w.scalar(sp["challenge"])
        w.scalar(sp["response"])
    return w


def _walk_qv(obj) -> _Walk:
    w = _Walk()
    for v in obj["votes"]:
        w.range_block(v["ciphertext"], v["range_proof"])
    w.range_block(obj["credit"]["ciphertext"], obj["credit"]["range_proof"])
    p = obj["credit_equivalence_proof"]
    w.scalar(p["challenge"])
    w.scalars(p["ciphertext_responses"])
    w.scalar(p["sum_response"])
    return w


def _walk_range_encryption(obj) -> _Walk:
    w = _Walk()
    w.range_block(obj["ciphertext"], obj["proof"])
    return w


def pack_choice(obj, single: bool) -> bytes:
    return b"".join(_walk_choice(obj, single).items)


def pack_qv(obj) -> bytes:
    return b"".join(_walk_qv(obj).items)


def pack_range_encryption(obj) -> bytes:
    return b"".join(_walk_range_encryption(obj).items)


def _range_from(values, at: int, n_partials: int, n_responses: int):
    ct = proto.Ciphertext(values[at], values[at + 1])
    partials = tuple(proto.Ciphertext(values[at + 2 + 2 * i], values[at + 3 + 2 * i]) for i in range(n_partials))
    e0 = at + 2 + 2 * n_partials
    ring = proto.RingProof(values[e0], tuple(values[e0 + 1 : e0 + 1 + n_responses]))
    return ct, proto.RangeProof(partials, ring), e0 + 1 + n_responses


def verify_choice(public_key: bytes, n_options: int, single: bool, obj) -> int:
    """EncryptedChoice::verify on an object of any shape -> status word"""
    try:
        w = _walk_choice(obj, single)
    except (Malformed, KeyError, TypeError):
        return MALFORMED
    word, values = w.decoded()
    if word != pk.OK:
        return word
    n, m = len(obj["choices"]), len(obj["range_proof"]["ring_responses"])
    choices = tuple(proto.Ciphertext(values[2 * i], values[2 * i + 1]) for i in range(n))
    ring = proto.RingProof(values[2 * n], tuple(values[2 * n + 1 : 2 * n + 1 + m]))
    sum_proof = proto.LogEqualityProof(values[2 * n + 1 + m], values[2 * n + 2 + m]) if single else None
    params = proto.ChoiceParams(proto.PublicKey.from_bytes(public_key), n_options, single)
    try:
        proto.EncryptedChoice(choices, ring, sum_proof).verify(params)
    except proto.ChoiceVerificationError as e:
        return pk.choice_status(e)
    return pk.OK


def verify_qv(public_key: bytes, n_options: int, credits: int, obj) -> int:
    """QuadraticVotingBallot::verify on an object of any shape -> status word"""
    try:
        w = _walk_qv(obj)
    except (Malformed, KeyError, TypeError):
        return MALFORMED
    word, values = w.decoded()
    if word != pk.OK:
        return word
    at, blocks = 0, []
    for block in list(obj["votes"]) + [obj["credit"]]:
        rp = block["range_proof"]
        ct, proof, at = _range_from(values, at, len(rp["partial_ciphertexts"]), len(rp["ring_responses"]))
        blocks.append(proto.CiphertextWithRangeProof(ct, proof))
    m = len(obj["credit_equivalence_proof"]["ciphertext_responses"])
    sumsq = proto.SumOfSquaresProof(values[at], tuple(values[at + 1 : at + 1 + m]), values[at + 1 + m])
    params = proto.QuadraticVotingParams(proto.PublicKey.from_bytes(public_key), n_options, credits)
    try:
        proto.QuadraticVotingBallot(tuple(blocks[:-1]), blocks[-1], sumsq).verify(params)
    except proto.QuadraticVotingError as e:
        return pk.qv_status(e)
    return pk.OK


def verify_range_encryption(public_key: bytes, upper_bound: int, obj) -> int:
    """PublicKey::verify_range on {"ciphertext", "proof"} (tests/snapshots.rs:93-105) -> status word"""
    try:
        w = _walk_range_encryption(obj)
    except (Malformed, KeyError, TypeError):
        return MALFORMED
    word, values = w.decoded()
    if word != pk.OK:
        return word
    rp = obj["proof"]
    ct, proof, _ = _range_from(values, 0, len(rp["partial_ciphertexts"]), len(rp["ring_responses"]))
    prepared = proto.PreparedRange(proto.RangeDecomposition.optimal(upper_bound))
    try:
        proto.verify_range(proto.PublicKey.from_bytes(public_key), prepared, ct, proof)
    except proto.VerificationError as e:
        return pk.status(pk.RANGE_LEN if e.kind == "len" else pk.RANGE_CHALLENGE)
    return pk.OK

