"""tests/pyref, the pure-Python verifier written from the reference's Rust source: its own pins (Keccak against hashlib, the upstream
Merlin known answer, RFC 9496, the reference's snapshots from their packed and from their object form, a flipped bit in every item
of every snapshot), and the differential against the C oracle on the corpus of tests/pyref_cases.py: every status word and every
tally of the committed fixture (tests/golden/pyref_verdicts.json) is regenerated here and must equal the oracle's.  The oracle and
pyref read the reference independently; a disagreement is a misreading in one of them (or in everything that shares the oracle's
reading: the HIP verifier, the plan builders, serde.py)."""
import ast
import hashlib
import json
import random
import sys
from pathlib import Path

import pytest

import pyref_cases as PC
from pyref import field as FD
from pyref import keccak, merlin, objects, packed
from pyref import protocol as proto
from pyref import ristretto as R

TESTS = Path(__file__).resolve().parent
L, P = FD.L, FD.P


def le(x: int) -> bytes:
    return x.to_bytes(32, "little")


# ------------------------------------------------------------------ independence
def test_pyref_imports_nothing_but_the_standard_library_and_itself():
    files = sorted((TESTS / "pyref").glob("**/*.py"))
    assert {f.name for f in files} >= {"__init__.py", "field.py", "ristretto.py", "keccak.py", "merlin.py", "protocol.py", "packed.py",
                                       "objects.py"}
    own = {f.stem for f in files}
    forbidden = {"ctypes", "numpy", "torch", "oracle", "elastic_elgamal_amd", "cffi", "subprocess", "importlib"}
    for f in files:
        tree = ast.parse(f.read_text())
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods = [a.name.split(".")[0] for a in node.names]
                level = 0
            elif isinstance(node, ast.ImportFrom):
                mods = [(node.module or "").split(".")[0]]
                level = node.level
            else:
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Name):
                    assert node.func.id not in ("__import__", "exec", "eval", "compile"), (f.name, node.lineno)
                continue
            for m in mods:
                if level:                                # relative: inside the package
                    assert level == 1 and (m in own or m == ""), (f.name, node.lineno, m)
                    if m == "" and isinstance(node, ast.ImportFrom):
                        assert all(a.name in own for a in node.names), (f.name, node.lineno)
                else:
                    assert m in sys.stdlib_module_names and m not in forbidden, (f.name, node.lineno, m)
        # no other test module either (they are importable by bare name from tests/)
        others = {p.stem for p in TESTS.glob("*.py")}
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not {a.name.split(".")[0] for a in node.names} & others, (f.name, node.lineno)
            if isinstance(node, ast.ImportFrom) and not node.level:
                assert (node.module or "").split(".")[0] not in others, (f.name, node.lineno)


def test_pool_workers_import_pyref_alone():
    """tests/pyref_judge.py is what a spawned worker imports: the standard library and pyref, no oracle, no product."""
    tree = ast.parse((TESTS / "pyref_judge.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods = [a.name.split(".")[0] for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0
            mods = [node.module.split(".")[0]]
        else:
            continue
        assert all(m == "pyref" or m in sys.stdlib_module_names and m != "ctypes" for m in mods), (node.lineno, mods)


# ------------------------------------------------------------------ Keccak, Merlin
@pytest.mark.parametrize("n", [0, 1, 135, 136, 137, 167, 168, 169, 1000])
def test_keccak_against_hashlib(n):
    msg = random.Random(n).randbytes(n)
    assert keccak.sha3_256(msg) == hashlib.sha3_256(msg).digest()
    assert keccak.shake128(msg, 400) == hashlib.shake_128(msg).digest(400)      # 400 bytes: more than two blocks squeezed


def test_merlin_upstream_known_answer():
    t = merlin.Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"


def test_merlin_append_u64_is_append_message_of_eight_bytes_and_clones_diverge():
    a, b = merlin.Transcript(b"x"), merlin.Transcript(b"x")
    a.append_u64(b"i", 0x0102030405060708)
    b.append_message(b"i", bytes([8, 7, 6, 5, 4, 3, 2, 1]))
    c = a.clone()
    assert a.challenge_bytes(b"c", 64) == b.challenge_bytes(b"c", 64)
    c.append_u64(b"j", 0)
    assert c.challenge_bytes(b"c", 64) != merlin.Transcript(b"x").challenge_bytes(b"c", 64)
    assert a.challenge_bytes(b"c", 16) == b.challenge_bytes(b"c", 16)           # the original was not disturbed by its clone


# ------------------------------------------------------------------ ristretto255
RFC9496_MULTIPLES = [                                    # RFC 9496 A.1, the multiples tests/test_oracle_golden.py holds
    "0000000000000000000000000000000000000000000000000000000000000000",
    "e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76",
    "6a493210f7499cd17fecb510ae0cea23a110e8d5b901f8acadd3095c73a3b919",
    "94741f5d5d52755ece4f23f044ee27d5d1ea1e2bd196b462166b16152a9d0259",
]


def test_ristretto_rfc9496_multiples():
    acc = R.IDENTITY
    for k, want in enumerate(RFC9496_MULTIPLES):
        assert R.encode(R.mul_generator(k)).hex() == want
        assert R.encode(acc).hex() == want
        assert R.encode(R.decode(bytes.fromhex(want))).hex() == want
        acc = R.add(acc, R.BASEPOINT)


def test_reference_rejections_refused(rejections):
    for k in ("non_element", "element_helper_invalid_element"):
        assert R.decode(bytes.fromhex(rejections[k]["hex"])) is None
    for k in ("non_canonical_scalar", "scalar_helper_invalid_scalar"):
        assert FD.scalar_from_canonical_bytes(bytes.fromhex(rejections[k]["hex"])) is None
    for k, v in rejections.items():                      # every entry: refused by the decoder its error text names
        if k.startswith("_"):
            continue
        raw = bytes.fromhex(v["hex"])
        assert raw == objects.b64url(v["b64"])
        if "group element" in v["error_contains"]:
            assert R.decode(raw) is None, k
        else:
            assert "group scalar" in v["error_contains"] and FD.scalar_from_canonical_bytes(raw) is None, k
    assert FD.scalar_from_canonical_bytes(le(L)) is None and FD.scalar_from_canonical_bytes(le(L - 1)) == L - 1
    for bad in (b"\xff" * 32, le(P), le(1), le(P - 1), le(P + 2)):             # >= p, and negative (odd) field elements
        assert R.decode(bad) is None


def test_order_torsion_scaling_and_roundtrip():
    assert R.is_identity(R.mul_generator(L)) and R.encode(R.mul_generator(L)) == bytes(32)
    assert not R.is_identity(R.mul_generator(L - 1)) and R.equal(R.mul_generator(L - 1), R.neg(R.BASEPOINT))
    rnd = random.Random(9496)
    for i in range(200):
        k = rnd.randrange(L)
        pt = R.mul_generator(k)
        assert R.on_curve(pt)
        enc = R.encode(pt)
        back = R.decode(enc)
        assert back is not None and R.equal(back, pt) and R.encode(back) == enc            # decode . encode = id
        if i < 40:
            for t in R.TORSION4:                         # the whole coset encodes alike
                assert R.encode(R.add(pt, t)) == enc
            f = rnd.randrange(1, P)                      # and every projective representative
            assert R.encode(tuple(c * f % P for c in pt)) == enc
        if i < 20:
            assert R.encode(R.add(pt, R.mul_generator(L - k))) == bytes(32)
            k2 = rnd.randrange(L)
            assert R.encode(R.double_mul_generator(k2, pt, k)) == R.encode(R.mul_generator((k2 * k + k) % L))


# ------------------------------------------------------------------ RangeDecomposition::optimal
@pytest.mark.parametrize("ub,text", [
    (5, "0..5"), (16, "4 * 0..4 + 0..4"), (17, "4 * 0..4 + 0..5"), (42, "6 * 0..7 + 0..6"), (60, "12 * 0..5 + 3 * 0..4 + 0..3"),
    (100, "20 * 0..5 + 4 * 0..5 + 0..4"), (101, "20 * 0..5 + 4 * 0..5 + 0..5"), (1000, "125 * 0..8 + 25 * 0..5 + 5 * 0..5 + 0..5"),
    (12345, "2880 * 0..4 + 720 * 0..5 + 90 * 0..9 + 15 * 0..7 + 3 * 0..5 + 0..3"),
    (777777, "125440 * 0..6 + 25088 * 0..6 + 3136 * 0..8 + 784 * 0..4 + 196 * 0..4 + 49 * 0..5 + 7 * 0..7 + 0..7"),
    (21, "3 * 0..7 + 0..3"),
])
def test_range_decomposition_known_answers_by_pyref(ub, text):
    d = proto.RangeDecomposition.optimal(ub)
    assert str(d) == text and d.upper_bound() == ub


def test_isqrt_by_pyref():
    for s in list(range(300)) + [10**4, 10**4 - 1, 2**64 - 1, 1 << 62, (1 << 62) - 1]:
        r = proto.isqrt(s)
        assert r * r <= s < (r + 1) * (r + 1)


# ------------------------------------------------------------------ the reference's snapshots
@pytest.fixture(scope="module")
def pk(golden):
    return objects.b64url(golden["public_key_b64"])


@pytest.fixture(scope="module")
def serde_snapshots():
    return json.loads((TESTS / "golden" / "snapshots_serde.json").read_text())


@pytest.fixture(scope="module")
def commit_equiv_snapshot():
    return json.loads((TESTS / "golden" / "commitment_equiv_ristretto.json").read_text())


def _snapshot_verifiers(pk, golden, oracle, commit_equiv_snapshot):
    """name -> (verifier, packed bytes, item -> the status kind (with detail) a failed proof over that item gives)."""
    out = {}
    g = lambda n: bytes.fromhex(golden[n]["packed"])     # noqa: E731
    out["encrypted-choice"] = (packed.ChoiceVerifier(pk, 5, True), g("encrypted-choice"),
                               lambda i: packed.RANGE_CHALLENGE if 10 <= i < 21 else packed.SUM_CHALLENGE)
    out["encrypted-multi-choice"] = (packed.ChoiceVerifier(pk, 5, False), g("encrypted-multi-choice"), lambda i: packed.RANGE_CHALLENGE)
    qv = packed.QvVerifier(pk, 5, 15)
    vs, cs = len(qv.vote_layout), len(qv.credit_layout)
    out["qv-ballot"] = (qv, g("qv-ballot"),
                        lambda i: packed.status(packed.QV_VARIANT_CHALLENGE, i // vs) if i < 5 * vs
                        else packed.QV_CREDIT_RANGE_CHALLENGE if i < 5 * vs + cs else packed.QV_CREDIT_EQUIV_CHALLENGE)
    out["range-encryption"] = (packed.RangeVerifier(pk, 100), g("range-encryption"), lambda i: packed.RANGE_CHALLENGE)
    out["zero-encryption"] = (packed.ZeroVerifier(pk), g("zero-encryption"), lambda i: packed.SUM_CHALLENGE)
    out["bool-encryption"] = (packed.BoolVerifier(pk), g("bool-encryption"), lambda i: packed.RANGE_CHALLENGE)
    # the sum-of-squares snapshot holds the proof alone; its ciphertexts are re-made by the oracle's prover (no ChaCha in pyref)
    values = golden["sum-sq-proof"]["params"]["values"]
    cts, proof = oracle.PublicKey(pk).sumsq_snapshot(values, oracle.keypair_from_seed(golden["seed"])[2])
    assert proof == g("sum-sq-proof")
    out["sum-sq-proof"] = (packed.SumOfSquaresVerifier(pk, len(values), b"test"), cts[64:] + cts[:64] + proof,
                           lambda i: packed.QV_CREDIT_EQUIV_CHALLENGE)
    ce = commit_equiv_snapshot
    o_, p_ = ce["object"], ce["object"]["proof"]
    item = b"".join(objects.b64url(s) for s in (o_["ciphertext"]["random_element"], o_["ciphertext"]["blinded_element"], o_["commitment"],
                                                p_["challenge"], p_["randomness_response"], p_["value_response"], p_["commitment_response"]))
    out["commitment-equiv-proof"] = (packed.CommitmentEquivalenceVerifier(pk, bytes(ce["blinding_base"]), ce["label"].encode()), item,
                                     lambda i: packed.SUM_CHALLENGE)
    return out


@pytest.fixture(scope="module")
def snapshot_verifiers(pk, golden, oracle, commit_equiv_snapshot):
    return _snapshot_verifiers(pk, golden, oracle, commit_equiv_snapshot)


SNAPSHOTS = ["encrypted-choice", "encrypted-multi-choice", "qv-ballot", "range-encryption", "zero-encryption", "bool-encryption",
             "sum-sq-proof", "commitment-equiv-proof"]


@pytest.mark.parametrize("name", SNAPSHOTS)
def test_snapshot_accepted_from_its_packed_form(snapshot_verifiers, name):
    v, blob, _ = snapshot_verifiers[name]
    assert len(blob) == v.size
    assert v.verify(blob) == packed.OK


def test_snapshot_plain_ciphertext_decrypts_to_42(golden, oracle, pk):
    sk = int.from_bytes(oracle.keypair_from_seed(golden["seed"])[0], "little")
    assert R.encode(R.mul_generator(sk)) == pk
    raw = bytes.fromhex(golden["ciphertext"]["packed"])
    assert raw == bytes.fromhex(golden["ciphertext-bin"]["packed"])
    r_elem, b_elem = R.decode(raw[:32]), R.decode(raw[32:])
    assert R.encode(R.sub(b_elem, R.mul(sk, r_elem))) == R.encode(R.mul_generator(golden["ciphertext"]["params"]["value"]))
    assert proto.Ciphertext(r_elem, b_elem).to_bytes() == raw


def test_snapshots_accepted_from_the_object_form_and_packed_by_pyref(golden, serde_snapshots, pk):
    s = serde_snapshots
    assert objects.verify_choice(pk, 5, True, s["encrypted-choice"]) == packed.OK
    assert objects.verify_choice(pk, 5, False, s["encrypted-multi-choice"]) == packed.OK
    assert objects.verify_qv(pk, 5, 15, s["qv-ballot"]) == packed.OK
    assert objects.verify_range_encryption(pk, 100, s["range-encryption"]) == packed.OK
    assert objects.pack_choice(s["encrypted-choice"], True).hex() == golden["encrypted-choice"]["packed"]
    assert objects.pack_choice(s["encrypted-multi-choice"], False).hex() == golden["encrypted-multi-choice"]["packed"]
    assert objects.pack_qv(s["qv-ballot"]).hex() == golden["qv-ballot"]["packed"]
    assert objects.pack_range_encryption(s["range-encryption"]).hex() == golden["range-encryption"]["packed"]
    # other parameters than the snapshot's: refused, with the reference's variant
    assert objects.verify_choice(pk, 4, True, s["encrypted-choice"]) == packed.OPTIONS_LEN
    assert objects.verify_qv(pk, 4, 15, s["qv-ballot"]) == packed.OPTIONS_LEN
    assert objects.verify_range_encryption(pk, 101, s["range-encryption"]) == packed.RANGE_LEN
    assert objects.verify_choice(pk, 5, False, s["encrypted-choice"]) == objects.MALFORMED


@pytest.mark.parametrize("name", SNAPSHOTS)
def test_flipped_bit_in_every_item_of_a_snapshot(snapshot_verifiers, name):
    """Two flips an item: bit 255 (no scalar and no element has it: BAD_SCALAR / BAD_POINT with the item's index), and a low bit (a
    scalar stays canonical, so the proof over the item fails with the kind the header gives it; an element either stops decoding, which
    is BAD_POINT at the item, or the proof over it fails)."""
    v, blob, kind_of = snapshot_verifiers[name]
    rnd = random.Random(name)
    for i, k in enumerate(v.layout):
        top = bytearray(blob)
        top[32 * i + 31] ^= 0x80
        assert v.verify(bytes(top)) == packed.status(packed.BAD_POINT if k == "P" else packed.BAD_SCALAR, i), (name, i)
        low = bytearray(blob)
        low[32 * i + rnd.randrange(31)] ^= 1 << rnd.randrange(8)
        item = bytes(low[32 * i : 32 * i + 32])
        if k == "S":
            assert int.from_bytes(item, "little") < L
            want = kind_of(i)
        else:
            want = kind_of(i) if R.decode(item) is not None else packed.status(packed.BAD_POINT, i)
        assert v.verify(bytes(low)) == want, (name, i)


def test_first_malformed_item_in_wire_order_wins(snapshot_verifiers):
    v, blob, _ = snapshot_verifiers["encrypted-choice"]
    bad = bytearray(blob)
    bad[32 * 22 + 31] ^= 0x80                            # the last scalar ...
    bad[32 * 3 + 31] ^= 0x80                             # ... and an element before it
    assert v.verify(bytes(bad)) == packed.status(packed.BAD_POINT, 3)
    bad[32 * 3 + 31] ^= 0x80
    bad[32 * 12] ^= 1                                    # a failing ring proof does not hide the malformed scalar behind it
    assert v.verify(bytes(bad)) == packed.status(packed.BAD_SCALAR, 22)


# ------------------------------------------------------------------ the fixture
def test_fixture_covers_the_corpus_and_every_status_kind():
    fx = PC.load_fixture()["families"]
    ids = [f"{c}:{n}" if c in ("sweep", "objects") else f"{c}:{n}/{k}" for c, n, k in PC.all_ids()]
    assert list(fx) == ids
    kinds = {w & 0xFF for f in fx.values() for w in f["words"]}
    assert kinds >= set(range(0, 13)), sorted(kinds)
    for fid, f in fx.items():
        assert len(PC.fixture_words(fid)) == f["n"] == len(f["words"]), fid      # the lookup keys are unique
    assert PC.FIXTURE.stat().st_size < 96 * 1024


@pytest.mark.parametrize("name,key_name", PC.F.FAMILIES, ids=[f"{n}-{k}" for n, k in PC.F.FAMILIES])
def test_forgery_sample_keeps_every_category_and_kind(name, key_name):
    fam = PC.F.family(name, key_name)
    picked = PC.forgery_sample(name, key_name)           # asserts the coverage itself
    assert (len(picked), len(fam.forgeries)) == PC.FORGERY_COUNTS[(name, key_name)]
    if (name, key_name) == ("single5", "golden"):
        assert len(picked) == len(fam.forgeries)
    k = PC.FORGERY_STRIDE[(name, key_name)]
    assert set(range(0, len(fam.forgeries), k)) <= set(picked)


def _oracle_words(jf):
    if jf.corpus == "objects":
        return [PC.oracle_object_word(jf, c.blob) for c in jf.cases]
    if jf.fam.tallies:
        return jf.fam.oracle_params.verify_batch(b"".join(c.blob for c in jf.cases), threads=8)
    return [jf.fam.verify(c.blob) for c in jf.cases]


@pytest.mark.parametrize("corpus,name,key_name", PC.all_ids(), ids=[f"{c}-{n}{'-' + k if k else ''}" for c, n, k in PC.all_ids()])
def test_pyref_fixture_and_oracle_agree(corpus, name, key_name):
    """The family's verdicts, regenerated by pyref, are the committed fixture's; the oracle's status words and tally equal them."""
    jf = PC.judged(corpus, name, key_name)
    entry = PC.fixture_entry(jf)
    words = entry["words"]
    if corpus != "objects":
        assert PC.pyref_verifier(jf.spec).layout == jf.fam.layout        # pyref's layout == the one derived from the product
    rejected_valid = [c.name for c, w in zip(jf.cases, words) if c.valid and w != 0]
    assert not rejected_valid, f"pyref rejects items the oracle's prover made: {rejected_valid[:10]}"
    if corpus == "sweep":
        assert all(w != 0 for c, w in zip(jf.cases, words) if not c.valid)
    want = _oracle_words(jf)
    wrong = [(c.name, hex(w), hex(x)) for c, w, x in zip(jf.cases, words, want) if w != x]
    assert not wrong, f"pyref against oracle (name, pyref, oracle): {wrong[:10]}"
    if "tally_sha256" in entry:
        blobs = [c.blob for c in jf.cases]
        tally = PC.pyref_tally(jf.spec, blobs, words)
        assert tally == jf.fam.tally(b"".join(blobs), want).hex() != bytes(64 * jf.fam.n_options).hex()
        assert entry["tally_sha256"] == hashlib.sha256(bytes.fromhex(tally)).hexdigest()
    assert entry == PC.load_fixture()["families"][jf.id], "stale fixture: regenerate with tests/golden/make_pyref_verdicts.py"


# ------------------------------------------------------------------ primitives against the oracle
EDGE_SCALARS = [0, 1, L - 1, 2**252]


def test_primitives_against_the_oracle(oracle):
    rnd = random.Random(20250)
    scalars = EDGE_SCALARS + [rnd.randrange(L) for _ in range(200)]
    multiples = [R.mul_generator(k) for k in range(17)]
    for k, pt in enumerate(multiples):                   # the multiples 0 .. 16 of the basepoint
        assert R.encode(pt) == oracle.point_mul_generator(le(k))
    points = [(le(0), R.IDENTITY)] + [(R.encode(m), m) for m in multiples[1:]]
    for i, k in enumerate(scalars):
        enc = R.encode(R.mul_generator(k))
        assert enc == oracle.point_mul_generator(le(k)), k
        assert oracle.point_roundtrip(enc) == enc == R.encode(R.decode(enc))
        points.append((enc, R.decode(enc)))
        wide = rnd.getrandbits(512) if i >= 4 else (2**512 - 1, L, L * L - 1, 2**511)[i]
        assert le(FD.scalar_from_wide(wide.to_bytes(64, "little"))) == oracle.sc_from_wide(wide.to_bytes(64, "little"))
        junk = rnd.randbytes(32)                         # random bytes: both decoders agree on what is an element
        got = R.decode(junk)
        assert oracle.point_roundtrip(junk) == (None if got is None else R.encode(got))
    for i, k in enumerate(scalars):
        (ea, a), (eb, b) = points[(3 * i) % len(points)], points[(7 * i + 1) % len(points)]
        r = scalars[(5 * i + 2) % len(scalars)]
        assert R.encode(R.double_mul_generator(k, a, r)) == oracle.point_double_mul_generator(le(k), ea, le(r)), i
        assert R.encode(R.add(a, b)) == oracle.point_add(ea, eb), i
        assert R.encode(R.sub(a, b)) == oracle.point_add(ea, eb, True), i
        for terms in (1, 2, 3, 7):
            ks = [scalars[(i + 11 * t) % len(scalars)] for t in range(terms)]
            ps = [points[(i + 13 * t) % len(points)] for t in range(terms)]
            got = R.encode(R.multi_mul(ks, [p for _, p in ps]))
            assert got == oracle.point_multi_mul(b"".join(le(x) for x in ks), b"".join(e for e, _ in ps)), (i, terms)
