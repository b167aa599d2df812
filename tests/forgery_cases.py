"""Corpus of WELL-FORMED FORGERIES (test infrastructure; built at test time from the oracle, deterministically from fixed seeds).

A random bit flip leaves a string that does not decode, or a scalar and a point unrelated to the true ones: every verifier rejects
it.  The inputs here are the ones a slightly wrong verifier accepts.  Every family (an election or a proof kind under one key)
starts from ordinary valid objects (uniform randomness, so every item is bound to the verdict) and applies to EVERY item:

1. same value, other representation: a scalar s as s + l, an element with field encoding s as p - s (the negative representative)
   and as s with bit 255 set.  A verifier that reduces instead of refusing accepts these, or (the transcripts absorb the wire bytes
   of an element) reports a failed proof where the item is to be refused; expected BAD_SCALAR / BAD_POINT at the item.
2. algebraic neighbours, all well formed: X + G, X + K, -X, [2]X; s + 1, s - 1, -s, 2s, s + 2^(32w) for w = 0..7 (mod l).
3. sum-preserving pairs on single-choice ballots: the sum proof still holds, so the range proof alone must reject.
4. true proofs of other statements: re-randomised ciphertexts, another key, a neighbouring bound / credits of the same size, another
   label, another participant index.
5. the prover lying: two ones, no one, credits + 1, a vote above its range, a range proof of value = bound.
6. transplants between two valid objects: every single item, the whole proof, the sum proof / sum-of-squares block only.
7. two failures at once (the precedence of the status word), and malformed items before and after a well-formed break.  The mutants
   named `..._malformed_...` hold a family-1 item by construction; every other mutant of families 2-8 is well formed.
8. one challenge word.  Every challenge here is compared with a hash of commitments that are computed FROM that challenge, so a
   changed challenge changes every word of the recomputed one -- unless the commitments do not depend on it, which is the case when
   the elements they multiply it with are the identity.  These bases are valid objects with all encryption randomness 0 (and values
   0 where a value enters); their challenge items get s + 2^(32w), so that the sent and the recomputed challenge differ in exactly
   one 32-bit word.  A compare that skips a word accepts one of them.  Only challenge items are touched: the other items of such
   objects are not all bound (edge_ballots.py).  Decryption shares have no such base (their first commitment multiplies the challenge
   with the participant's key) and a single-choice ballot has one for its sum proof only (a chosen option is never the identity).

Item layouts (which 32-byte items are elements, which scalars) are derived from the serde layout (elastic_elgamal_amd/serde.py,
ingest.unpack_qv_ballot) and the product's range_decomposition, never from the bytes.
"""
from __future__ import annotations

import dataclasses
import functools
import random
from dataclasses import dataclass, field
from math import isqrt

import commit_equiv_ref as CE
import edge_ballots as E
from oracle import oracle as o

L = o.L
P = 2**255 - 19
IDENTITY = E.IDENTITY


def G() -> bytes:
    return E.element(1)


OTHER_KEY = "2G"
ELECTIONS = ("single5", "single9", "multi20", "qv4x12")
PROOFS = ("zero", "bool", "range12", "range15", "range1000", "share", "sumsq2", "commit_equiv")
FAMILIES = tuple((n, "golden") for n in ELECTIONS + PROOFS) + (("single5", OTHER_KEY), ("zero", OTHER_KEY))
N_VALID = {"single": 66, "multi": 10, "qv": 10}          # valid neighbours kept per family (proofs: 8)
LABEL = b"test"                                          # the label of oracle.sumsq_snapshot
OTHER_LABELS = (b"tesu", b"Test")                        # one byte away, at either end


@dataclass(frozen=True)
class Forgery:
    name: str
    family: str
    blob: bytes
    what_bug_it_catches: str
    mutation: int = 0            # 1..8, the list in the module docstring
    item: int = -1               # family 1: the item that must be reported


@dataclass
class Family(E.Family):
    """E.Family (oracle verdicts, HIP verifier, tally) plus the kinds sumsq and commit_equiv, the item layout, valid objects and
    the forgeries."""
    layout: str = ""
    valid: list = field(default_factory=list)
    forgeries: list = field(default_factory=list)

    @property
    def size(self) -> int:
        return len(self.layout) * 32

    @property
    def label(self) -> str:
        return f"{self.name}/{self.key_name}"

    def verify(self, blob: bytes) -> int:
        if self.kind == "sumsq":
            n = self.n_options
            return self.oracle_params.verify_sumsq(blob[: 64 * n], blob[64 * n : 64 * n + 64], blob[64 * n + 64 :], self.extra["label"])
        if self.kind == "commit_equiv":
            return CE.verify(self.key, self.extra["h"], self.extra["label"], blob)
        return super().verify(blob)

    def gpu_params(self, eg, ctx):
        if self.kind == "sumsq":
            return eg.SumOfSquaresVerifier(ctx, self.key, self.n_options, self.extra["label"])
        if self.kind == "commit_equiv":
            return eg.CommitmentEquivalenceVerifier(ctx, self.key, self.extra["h"], self.extra["label"])
        return super().gpu_params(eg, ctx)

    def with_label(self, label: bytes) -> "Family":
        """The verifier of the same statements under another label (sumsq, commit_equiv): this family's VALID objects are true
        proofs of another statement there.  The oracle's sum-of-squares prover fixes its label, so for that kind the label moves
        on the verifier's side."""
        return dataclasses.replace(self, extra={**self.extra, "label": label}, valid=[], forgeries=[])

    def well_formed(self, blob: bytes) -> bool:
        return all((o.point_roundtrip(it) is not None) if k == "P" else o.sc_is_canonical(it) for k, it in zip(self.layout, items(blob)))


# ------------------------------------------------------------------ bytes, scalars, elements
def items(blob: bytes) -> list:
    return [blob[i : i + 32] for i in range(0, len(blob), 32)]


def put(blob: bytes, changes: dict) -> bytes:
    b = bytearray(blob)
    for i, v in changes.items():
        assert len(v) == 32
        b[32 * i : 32 * i + 32] = v
    return bytes(b)


def num(b: bytes) -> int:
    return int.from_bytes(b, "little")


def sc(x: int) -> bytes:
    return (x % L).to_bytes(32, "little")


def add(a: bytes, b: bytes) -> bytes:
    return o.point_add(a, b)


def sub(a: bytes, b: bytes) -> bytes:
    return o.point_add(a, b, True)


def other_representations(kind: str, it: bytes) -> list:
    """Family 1: (tag, bytes) of the same value in encodings a strict verifier refuses."""
    s = num(it)
    if kind == "S":
        return [("s+l", (s + L).to_bytes(32, "little"))] if s + L < 2**256 else []
    return [("p-s", (P - s).to_bytes(32, "little")), ("bit255", (s | 1 << 255).to_bytes(32, "little"))]


def neighbours(kind: str, it: bytes, key: bytes) -> list:
    """Family 2: (tag, bytes) of well-formed values next to the true one."""
    if kind == "P":
        return [("+G", add(it, G())), ("+K", add(it, key)), ("neg", sub(IDENTITY, it)), ("dbl", add(it, it))]
    s = num(it)
    return [("+1", sc(s + 1)), ("-1", sc(s - 1)), ("neg", sc(-s)), ("dbl", sc(2 * s))] + [(f"+2^{32 * w}", sc(s + (1 << 32 * w))) for w in range(8)]


# ------------------------------------------------------------------ layouts
def _layout_from_object(obj, n_items: int) -> str:
    """`obj` is the serde-layout object unpacked from a blob whose item i holds the number i: the field a string sits under says
    whether it is an element (random_element, blinded_element) or a scalar, its value which item it is."""
    from elastic_elgamal_amd import serde

    kinds = [None] * n_items

    def walk(x, name=None):
        if isinstance(x, dict):
            for k, v in x.items():
                walk(v, k)
        elif isinstance(x, list):
            for v in x:
                walk(v, name)
        elif isinstance(x, str):
            kinds[num(serde.b64url_decode(x))] = "P" if name in ("random_element", "blinded_element") else "S"

    walk(obj)
    assert None not in kinds
    return "".join(kinds)


def _numbered(n_items: int) -> bytes:
    return b"".join(i.to_bytes(32, "little") for i in range(n_items))


def range_rings(bound: int) -> list:
    """Ring sizes of RangeDecomposition::optimal(bound), by the product's host code."""
    import elastic_elgamal_amd as eg
    from elastic_elgamal_amd import ingest

    return [size for _, size in ingest.parse_range(eg.range_decomposition(bound))]


def range_layout(bound: int) -> str:
    """ciphertext || partial ciphertexts || common challenge || ring responses (serde._range_proof)."""
    rings = range_rings(bound)
    return "P" * (2 * len(rings)) + "S" * (1 + sum(rings))


def choice_layout(n: int, single: bool) -> str:
    from elastic_elgamal_amd import serde

    n_items = 2 * n + 1 + 2 * n + (2 if single else 0)
    return _layout_from_object(serde.unpack_encrypted_choice(_numbered(n_items), n, single), n_items)


def qv_layout(n: int, credits: int) -> str:
    from elastic_elgamal_amd import ingest

    n_items = n * len(range_layout(isqrt(credits) + 1)) + len(range_layout(credits + 1)) + 2 * n + 2
    return _layout_from_object(ingest.unpack_qv_ballot(_numbered(n_items), n, credits), n_items)


# ------------------------------------------------------------------ bases
def _split(raw: bytes, size: int) -> list:
    return [raw[i : i + size] for i in range(0, len(raw), size)]


def _zero_randomness(make, values=None):
    """make() with every encryption randomness the prover draws pinned to 0 (or to `values[role]`): family 8's bases."""
    with o.Script() as s:
        make()
    pins = {t: 0 for t in s.trace if t[0] in ("ct_r", "value_r")}
    pins.update(values or {})
    with o.Script(pins):
        return make()


class _Builder:
    def __init__(self, fam: Family):
        self.fam = fam
        self.seen = set(fam.valid)

    def add(self, mutation: int, name: str, blob: bytes, why: str, item: int = -1, base: bytes | None = None):
        """Skips a mutant equal to its original (and one already in the corpus)."""
        f = self.fam
        assert len(blob) == f.size, name
        if blob == base or blob in self.seen:
            return
        self.seen.add(blob)
        f.forgeries.append(Forgery(name, f.label, blob, why, mutation, item))

    # families 1, 2, 6 (single items) and 7 (malformed around a break): the same for every layout
    def generic(self, a: bytes, b: bytes, break_item: int):
        f = self.fam
        ia, ib = items(a), items(b)
        for i, kind in enumerate(f.layout):
            for tag, v in other_representations(kind, ia[i]):
                self.add(1, f"rep_{tag}@{i}", put(a, {i: v}), "a decoder that reduces or masks instead of refusing", i, a)
            for tag, v in neighbours(kind, ia[i], f.key):
                self.add(2, f"nbr_{tag}@{i}", put(a, {i: v}), "an equation or compare that does not bind this item exactly", base=a)
            self.add(6, f"transplant_item@{i}", put(a, {i: ib[i]}), "an item checked against another ballot's data", base=a)
        brk = {break_item: sc(num(ia[break_item]) + 1)}
        first_p, last_s = f.layout.index("P"), len(f.layout) - 1
        for tag, i in (("before", first_p), ("after", last_s)):
            if i == break_item:
                continue
            _, v = other_representations(f.layout[i], ia[i])[0]
            self.add(7, f"two_malformed_{tag}_break@{i}", put(a, {**brk, i: v}), "a proof failure reported in place of a malformed item", i, a)
        _, vp = other_representations("P", ia[first_p])[0]
        _, vs = other_representations("S", ia[last_s])[0]
        self.add(7, f"two_malformed_both@{first_p}", put(a, {**brk, first_p: vp, last_s: vs}), "the later malformed item reported", first_p, a)

    def challenge_words(self, base: bytes, challenge_items):
        f = self.fam
        assert f.verify(base) == 0, (f.label, "zero-randomness base")
        f.extra.setdefault("word_bases", []).append(base)
        for i in challenge_items:
            s = num(items(base)[i])
            for w in range(8):
                self.add(8, f"word{w}@{i}", put(base, {i: sc(s + (1 << 32 * w))}), "a challenge compare that skips a word", base=base)


# ------------------------------------------------------------------ choice elections
def _choice(name: str, key_name: str) -> Family:
    single = name.startswith("single")
    n = int(name[6:] if single else name[5:])
    pk = E.key(key_name)
    op = o.ChoiceParams(pk, n, single)
    fam = Family(name, "single" if single else "multi", key_name, pk, n_options=n, oracle_params=op, layout=choice_layout(n, single))
    fam.valid = _split(op.generate_batch(31000 + n, 0, N_VALID[fam.kind], n_selected=0 if single else 3, threads=8), fam.size)
    a, b = fam.valid[0], fam.valid[1]
    ia = items(a)
    bld = _Builder(fam)
    e0 = 2 * n                                           # the ring proof's common challenge; two responses a ring follow
    resp = lambda j, k: e0 + 1 + 2 * j + k               # noqa: E731
    bld.generic(a, b, break_item=resp(n // 2, 0))
    K = pk
    if single:
        for i in range(n):                               # family 3
            j = (i + 1) % n
            for xn, X in (("G", G()), ("K", K)):
                for part, off in (("R", 0), ("B", 1)):
                    bld.add(3, f"pair_{part}{i}+{xn}_{part}{j}-{xn}", put(a, {2 * i + off: add(ia[2 * i + off], X), 2 * j + off: sub(ia[2 * j + off], X)}),
                            "a range proof trusted because the sum proof holds", base=a)
            swap = {2 * i: ia[2 * j], 2 * i + 1: ia[2 * j + 1], 2 * j: ia[2 * i], 2 * j + 1: ia[2 * i + 1]}
            bld.add(3, f"swap_ct{i}_{j}", put(a, swap), "ring transcripts that do not bind the option's position", base=a)
            swap.update({resp(i, k): ia[resp(j, k)] for k in (0, 1)})
            swap.update({resp(j, k): ia[resp(i, k)] for k in (0, 1)})
            bld.add(3, f"swap_ct_and_responses{i}_{j}", put(a, swap), "ring transcripts that do not bind the option's position", base=a)
    for i in range(n):                                   # family 4
        bld.add(4, f"rerandomised_ct{i}", put(a, {2 * i: add(ia[2 * i], G()), 2 * i + 1: add(ia[2 * i + 1], K)}),
                "a proof accepted for another encryption of the same value", base=a)
    other = o.ChoiceParams(E.key(OTHER_KEY if key_name == "golden" else "golden"), n, single)
    bld.add(4, "other_key", other.generate_batch(31000 + n, 0, 1, n_selected=0 if single else 3, threads=1), "the key left out of a transcript")
    if single:                                           # family 5
        lies = {"two_ones": [1, 1] + [0] * (n - 2), "no_one": [0] * n, "all_ones": [1] * n}
        for tag, flags in lies.items():
            bld.add(5, f"lie_{tag}", op.new_ballot(flags, o.rng_from_u64(32000 + n)), "a sum proof that is not checked against the sum")
    bld.add(6, "transplant_whole_proof", a[: 64 * n] + b[64 * n :], "a proof not bound to the ciphertexts")
    bld.add(6, "transplant_ciphertexts", b[: 64 * n] + a[64 * n :], "a proof not bound to the ciphertexts")
    if single:
        bld.add(6, "transplant_sum_proof", a[:-64] + b[-64:], "a sum proof not bound to the ciphertexts")
        bld.add(6, "transplant_ring_proof", a[: 64 * n] + b[64 * n : -64] + a[-64:], "a ring proof not bound to the ciphertexts")
        last = len(fam.layout) - 1                       # family 7: sum and range both broken -> the sum is reported
        for j in (0, n - 1):
            bld.add(7, f"two_sum_and_ring{j}", put(a, {last: sc(num(ia[last]) + 1), resp(j, 1): sc(num(ia[resp(j, 1)]) + 1)}),
                    "the range failure reported in place of the sum failure", base=a)
        bld.add(7, "two_sum_and_common_challenge", put(a, {last - 1: sc(num(ia[last - 1]) + 1), e0: sc(num(ia[e0]) + 1)}),
                "the range failure reported in place of the sum failure", base=a)
        # family 8: r summing to 0 -> the sum proof runs over the identity
        rnd = random.Random(f"forgery/{name}/{key_name}")
        rs = [rnd.randrange(L) for _ in range(n - 1)]
        rs.append(-sum(rs) % L)
        base = E.scripted({("ct_r", 0, j): r for j, r in enumerate(rs)}, lambda: op.new_ballot([0] * (n - 1) + [1], o.rng_from_u64(33000 + n)))
        bld.challenge_words(base, [last - 1])
    else:
        base = _zero_randomness(lambda: op.new_ballot([0] * n, o.rng_from_u64(33000 + n)))
        bld.challenge_words(base, [e0])
    return fam


# ------------------------------------------------------------------ quadratic voting
def _qv(name: str, key_name: str) -> Family:
    n, credits = (int(x) for x in name[2:].split("x"))
    pk = E.key(key_name)
    op = o.QvParams(pk, n, credits)
    fam = Family(name, "qv", key_name, pk, n_options=n, credits=credits, oracle_params=op, layout=qv_layout(n, credits))
    assert fam.size == op.ballot_size
    fam.valid = _split(op.generate_batch(34000, 0, N_VALID["qv"], threads=8), fam.size)
    a, b = fam.valid[0], fam.valid[1]
    ia = items(a)
    vote_items, vote_rings, credit_rings = op.vote_size // 32, len(range_rings(isqrt(credits) + 1)), len(range_rings(credits + 1))
    vstart = lambda i: i * vote_items                    # noqa: E731  vote i; i = n: the credit block
    first_resp = lambda i: vstart(i) + 2 * (vote_rings if i < n else credit_rings) + 1    # noqa: E731
    sumsq0 = len(fam.layout) - (2 * n + 2)               # the sum-of-squares challenge; 2n responses and the sum response follow
    last = len(fam.layout) - 1
    bld = _Builder(fam)
    bld.generic(a, b, break_item=first_resp(n // 2))
    K = pk
    for i in range(n + 1):                               # family 4
        s = vstart(i)
        bld.add(4, f"rerandomised_ct{i}", put(a, {s: add(ia[s], G()), s + 1: add(ia[s + 1], K)}), "a proof accepted for another encryption", base=a)
    other = o.QvParams(E.key(OTHER_KEY), n, credits)
    bld.add(4, "other_key", other.generate_batch(34000, 0, 1, threads=1), "the key left out of a transcript")
    for dn, dc in ((0, -2), (0, -1), (0, 1), (0, 2), (-1, 0), (1, 0)):     # neighbouring elections whose ballots have this size
        try:
            nb = o.QvParams(pk, n + dn, credits + dc)
        except ValueError:
            continue
        if nb.ballot_size == fam.size:
            bld.add(4, f"made_for_qv{n + dn}x{credits + dc}", nb.new_ballot([1] + [0] * (n + dn - 1), o.rng_from_u64(34100)),
                    "the range's name left out of a transcript")
    hi = isqrt(credits) + 1                              # family 5: the first vote value out of range
    spend = _squares(credits + 1, n, hi)
    assert spend is not None, "no vote vector spends credits + 1"
    bld.add(5, "lie_credits_plus_1", op.new_ballot(spend, o.rng_from_u64(34200)), "a credit range proof that is not checked")
    for i in range(n):
        votes = [0] * n
        votes[i] = hi
        bld.add(5, f"lie_vote{i}_above_range", op.new_ballot(votes, o.rng_from_u64(34300 + i)), "a vote range proof that is not checked")
    ct_items = [vstart(i) + k for i in range(n + 1) for k in (0, 1)]        # family 6
    ibb = items(b)
    bld.add(6, "transplant_whole_proof", put(b, {i: ia[i] for i in ct_items}), "proofs not bound to the ciphertexts")
    bld.add(6, "transplant_sumsq_block", a[: 32 * sumsq0] + b[32 * sumsq0 :], "a sum-of-squares proof not bound to the ciphertexts")
    for i in range(n + 1):
        blk = range(vstart(i), vstart(i + 1) if i < n else sumsq0)
        bld.add(6, f"transplant_block{i}", put(a, {k: ibb[k] for k in blk}), "a vote not bound to the sum of squares")
    bump = lambda i: {i: sc(num(ia[i]) + 1)}             # noqa: E731  family 7
    for v1, v2 in ((0, n - 1), (1, 2), (n - 2, n - 1)):
        bld.add(7, f"two_variants{v1}_{v2}", put(a, {**bump(first_resp(v1)), **bump(first_resp(v2))}), "the later vote reported", base=a)
    bld.add(7, "two_variant_and_credit_range", put(a, {**bump(first_resp(n - 1)), **bump(first_resp(n))}), "the credit range reported before a vote", base=a)
    bld.add(7, "two_credit_range_and_sumsq", put(a, {**bump(first_resp(n)), **bump(last)}), "the sum of squares reported before the credit range", base=a)
    bld.add(7, "two_variant_and_sumsq", put(a, {**bump(first_resp(0)), **bump(sumsq0)}), "the sum of squares reported before a vote", base=a)
    base = _zero_randomness(lambda: op.new_ballot([0] * n, o.rng_from_u64(34400)))          # family 8
    bld.challenge_words(base, [first_resp(i) - 1 for i in range(n + 1)] + [sumsq0])
    return fam


def _squares(total: int, n: int, hi: int):
    """n votes below `hi` whose squares sum to `total`, or None."""
    if n == 0:
        return [] if total == 0 else None
    for v in range(min(hi - 1, isqrt(total)), -1, -1):
        rest = _squares(total - v * v, n - 1, hi)
        if rest is not None:
            return [v] + rest
    return None


# ------------------------------------------------------------------ standalone proofs
def _proof(name: str, key_name: str) -> Family:
    pk = E.key(key_name)
    k = o.PublicKey(pk)
    other_pk = E.key(OTHER_KEY if key_name == "golden" else "golden")
    k2 = o.PublicKey(other_pk)
    seeds = range(35000, 35008)
    foreign = []                                         # family 4: (name, blob, why)
    lies = []
    word_base, word_items = None, []
    if name == "zero":
        fam = Family(name, "zero", key_name, pk, oracle_params=k, layout="PPSS")
        make = lambda kk, s: kk.encrypt_zero(o.rng_from_u64(s))                              # noqa: E731
        word_base, word_items = _zero_randomness(lambda: make(k, 35100)), [2]
    elif name == "bool":
        fam = Family(name, "bool", key_name, pk, oracle_params=k, layout="PPSSS")
        make = lambda kk, s: kk.encrypt_bool(bool(s & 1), o.rng_from_u64(s))                 # noqa: E731
        word_base, word_items = _zero_randomness(lambda: k.encrypt_bool(False, o.rng_from_u64(35100))), [2]
    elif name.startswith("range"):
        bound = int(name[5:])
        pr = o.PreparedRange(bound)
        fam = Family(name, "range", key_name, pk, credits=bound, oracle_params=k, extra={"range": pr}, layout=range_layout(bound))
        assert fam.size == 64 + pr.proof_size
        make = lambda kk, s: kk.encrypt_range(pr, (s * 7919) % bound, o.rng_from_u64(s))     # noqa: E731
        for d in (-2, -1, 1, 2):                         # neighbouring bounds whose proofs have this size
            nb = o.PreparedRange(bound + d)
            if nb.proof_size == pr.proof_size:
                foreign.append((f"made_for_bound{bound + d}", k.encrypt_range(nb, 1, o.rng_from_u64(35200 + d)), "the range's name left out of a transcript"))
        lies.append(("lie_value_is_bound", k.encrypt_range(pr, bound, o.rng_from_u64(35300)), "an upper bound that is inclusive"))
        word_base, word_items = _zero_randomness(lambda: k.encrypt_range(pr, 0, o.rng_from_u64(35100))), [2 * len(pr.rings)]
    elif name == "share":
        x = {"shares": 3, "threshold": 2, "index": 1, "participant_key": E.element(777)}
        fam = Family(name, "share", key_name, pk, extra=x, layout="PPSS")
        share = lambda idx, key, s: E.element(98000 + s) + o.decryption_share_new(E.sc(777), E.element(98000 + s), 3, 2, key, idx, o.rng_from_u64(s))   # noqa: E731
        make = lambda kk, s: share(1, kk.bytes, s)                                           # noqa: E731
        foreign += [(f"made_for_index{i}", share(i, pk, 35200 + i), "the participant's index left out of a transcript") for i in (0, 2)]
        foreign.append(("made_for_4_shares", E.element(5) + o.decryption_share_new(E.sc(777), E.element(5), 4, 2, pk, 1, o.rng_from_u64(35210)),
                        "the key set's size left out of a transcript"))
        foreign.append(("other_secret", E.element(6) + o.decryption_share_new(E.sc(778), E.element(6), 3, 2, pk, 1, o.rng_from_u64(35211)),
                        "a share not checked against the participant's key"))
    elif name.startswith("sumsq"):
        n = int(name[5:])
        fam = Family(name, "sumsq", key_name, pk, n_options=n, oracle_params=k, extra={"label": LABEL}, layout="P" * (2 * n + 2) + "S" * (2 * n + 2))

        def make(kk, s, values=None):
            cts, proof = kk.sumsq_snapshot(values if values is not None else [(s + 3 * i) % 5 for i in range(n)], o.rng_from_u64(s))
            return cts[64:] + cts[:64] + proof           # value ciphertexts || sum ciphertext || proof

        word_base, word_items = _zero_randomness(lambda: make(k, 35100, [0] * n)), [2 * n + 2]
    else:
        h = E.element(5)
        fam = Family(name, "commit_equiv", key_name, pk, extra={"h": h, "label": LABEL}, layout="P" * CE.N_POINTS + "S" * (CE.N_ITEMS - CE.N_POINTS))
        make = lambda kk, s, label=LABEL, hh=h: CE.prove(kk.bytes, hh, label, s % 1000, o.rng_from_u64(s))[0]   # noqa: E731
        foreign.append(("other_blinding_base", make(k, 35220, hh=E.element(6)), "the blinding base left out of a transcript"))
        word_base, word_items = CE.prove(pk, h, LABEL, 0, o.rng_from_u64(35100), pins={"r": 0, "r_c": 0})[0], [3]
    fam.valid = [make(k, s) for s in seeds]
    a, b = fam.valid[0], fam.valid[1]
    ia = items(a)
    bld = _Builder(fam)
    bld.generic(a, b, break_item=len(fam.layout) - 2 if fam.kind != "commit_equiv" else 4)
    # family 4
    if fam.kind != "share":                              # a share's first items are no ciphertext
        bld.add(4, "rerandomised_ct", put(a, {0: add(ia[0], G()), 1: add(ia[1], pk)}), "a proof accepted for another encryption", base=a)
    if fam.kind == "sumsq":
        s = 2 * fam.n_options
        bld.add(4, "rerandomised_sum_ct", put(a, {s: add(ia[s], G()), s + 1: add(ia[s + 1], pk)}), "a proof accepted for another encryption", base=a)
    bld.add(4, "other_key", make(k2, 35230), "the key left out of a transcript")
    if fam.kind == "commit_equiv":
        for tag, label in zip(("last_byte", "first_byte"), OTHER_LABELS):
            bld.add(4, f"other_label_{tag}", CE.prove(pk, fam.extra["h"], label, 77, o.rng_from_u64(35250))[0], "the label's bytes not all absorbed")
    for nm, blob, why in foreign:
        bld.add(4, nm, blob, why)
    for nm, blob, why in lies:
        bld.add(5, nm, blob, why)
    half = fam.layout.index("S")                         # family 6: the elements of a with the scalars of b
    bld.add(6, "transplant_whole_proof", a[: 32 * half] + b[32 * half :], "a proof not bound to its elements")
    if word_base is not None:
        bld.challenge_words(word_base, word_items)
    return fam


# ------------------------------------------------------------------ the corpus
@functools.lru_cache(None)
def family(name: str, key_name: str = "golden") -> Family:
    if name.startswith(("single", "multi")):
        return _choice(name, key_name)
    if name.startswith("qv"):
        return _qv(name, key_name)
    return _proof(name, key_name)


@functools.lru_cache(None)
def verdicts(name: str, key_name: str = "golden") -> tuple:
    """The oracle's status word of every forgery of the family, computed once and shared by the tests."""
    fam = family(name, key_name)
    if fam.tallies:
        return tuple(fam.oracle_params.verify_batch(b"".join(f.blob for f in fam.forgeries), threads=8))
    return tuple(fam.verify(f.blob) for f in fam.forgeries)
