"""Commitment-equivalence proofs without a GPU: the test-side restatement (tests/commit_equiv_ref.py) against the reference's snapshot
(tests/golden/commitment_equiv_ristretto.json) and the negative cases of its unit test (src/proofs/commitment.rs:298-330), the new
entries of the C ABI, the shape of the verification plan, its index check under ASan + UBSan, and the serde packer."""
import copy
import ctypes as C
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import commit_equiv_ref as R
import elastic_elgamal_amd as eg
from elastic_elgamal_amd import serde

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
NEW_SYMBOLS = ("eg_commit_equiv_params_create", "eg_commit_equiv_prove_batch", "eg_commit_equiv_prove_batch_device")


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def snap(oracle, fx):
    """(pk, H, label, the snapshot's item)."""
    _, pk, _ = oracle.keypair_from_seed(fx["seed"])
    item = b"".join(serde.b64url_decode(s) for s in (
        fx["object"]["ciphertext"]["random_element"], fx["object"]["ciphertext"]["blinded_element"], fx["object"]["commitment"],
        fx["object"]["proof"]["challenge"], fx["object"]["proof"]["randomness_response"], fx["object"]["proof"]["value_response"],
        fx["object"]["proof"]["commitment_response"]))
    return pk, bytes(fx["blinding_base"]), fx["label"].encode(), item


def test_restatement_reproduces_the_snapshot_and_accepts_it(oracle, fx, snap):
    pk, h, label, want = snap
    assert len(want) == R.ITEM == 224 and len(h) == 32
    _, pk2, rng = oracle.keypair_from_seed(fx["seed"])          # rng stands after the keypair draw: rng_skip = 1
    item, r_c = R.prove(pk2, h, label, fx["value"], rng)
    assert pk2 == pk
    for i in range(R.N_ITEMS):
        assert item[32 * i : 32 * i + 32] == want[32 * i : 32 * i + 32], f"item {i}"
    assert R.verify(pk, h, label, want) == R.OK
    # the commitment is [v]G + [r_c]H over the Bulletproofs blinding base
    v = R.sc(fx["value"])
    assert oracle.point_add(oracle.point_mul_generator(v), oracle.point_multi_mul(r_c, h)) == want[64:96]


def test_restatement_rejects_the_reference_negatives(oracle, fx, snap):
    pk, h, label, item = snap
    # another ciphertext under the same key (commitment.rs:298-308: receiver.encrypt(8))
    rng = oracle.rng_from_u64(99)
    r = oracle.sc_from_wide(oracle.rng_fill64(rng))
    other_ct = oracle.point_mul_generator(r) + oracle.point_add(oracle.point_mul_generator(R.sc(8)), oracle.point_multi_mul(r, pk))
    assert R.verify(pk, h, label, other_ct + item[64:]) == R.CHALLENGE
    # C + G (:310-319)
    c_plus_g = oracle.point_add(item[64:96], oracle.point_mul_generator(R.ONE))
    assert R.verify(pk, h, label, item[:64] + c_plus_g + item[96:]) == R.CHALLENGE
    # another transcript label (:321-330)
    assert R.verify(pk, h, b"other_test", item) == R.CHALLENGE
    # a wrong H and a wrong K
    assert R.verify(pk, oracle.point_mul_generator(R.sc(5)), label, item) == R.CHALLENGE
    assert R.verify(pk, pk, label, item) == R.CHALLENGE
    assert R.verify(oracle.point_mul_generator(R.sc(5)), h, label, item) == R.CHALLENGE
    assert R.verify(h, h, label, item) == R.CHALLENGE


def test_restatement_rejects_a_flipped_bit_in_every_item(snap):
    pk, h, label, item = snap
    for i in range(R.N_ITEMS):
        for bit in (0, 77, 250):
            t = bytearray(item)
            t[32 * i + bit // 8] ^= 1 << (bit % 8)
            st = R.verify(pk, h, label, bytes(t))
            assert st != R.OK, (i, bit)
            # a flip either breaks the encoding of THIS item or the challenge; never another item's verdict
            assert st == R.CHALLENGE or (st >> 8 == i and st & 0xFF == (R.BAD_POINT if i < R.N_POINTS else R.BAD_SCALAR)), (i, bit, st)


def test_restatement_precedence_of_malformed_items(snap):
    pk, h, label, item = snap
    bad_scalar, bad_point = b"\xff" * 32, b"\x01" + bytes(31)        # >= l; an odd (negative) field element
    for i in range(R.N_ITEMS):
        t = item[: 32 * i] + (bad_point if i < R.N_POINTS else bad_scalar) + item[32 * i + 32 :]
        kind = R.BAD_POINT if i < R.N_POINTS else R.BAD_SCALAR
        assert R.verify(pk, h, label, t) == kind | (i << 8), i
    both = item[:64] + bad_point + bad_scalar + item[128:]
    assert R.verify(pk, h, label, both) == R.BAD_POINT | (2 << 8)         # the first malformed item wins
    assert R.verify(pk, h, label, item[:96] + bad_scalar + item[128:192] + bad_scalar) == R.BAD_SCALAR | (3 << 8)


def test_identity_commitment_with_a_matching_proof_is_accepted(oracle, fx):
    _, pk, rng = oracle.keypair_from_seed(7)
    h = bytes(fx["blinding_base"])
    item, r_c = R.prove(pk, h, b"zero", 0, rng, pins={"r_c": 0})
    assert item[64:96] == bytes(32) and r_c == bytes(32)
    assert R.verify(pk, h, b"zero", item) == R.OK


def test_library_exports_the_new_entries():
    lib = eg._load()
    for name in NEW_SYMBOLS:
        assert name in eg.exported_symbols(), name
        assert hasattr(lib, name), name
    assert eg.ABI_VERSION == lib.eg_abi_version() == 7
    assert hasattr(eg, "CommitmentEquivalenceVerifier")
    for m in ("verify", "verify_device", "prove", "prove_device"):
        assert callable(getattr(eg.CommitmentEquivalenceVerifier, m)), m


def test_plan_describe_has_the_shape_of_the_proof():
    d = eg.plan_describe("commit_equiv")
    want = {"stride": 224, "wire_points": 3, "wire_scalars": 4, "stages": 1, "jobs": 3, "jobs_per_stage": [3], "direct_terms": 3,
            "combs": 5, "var_terms": 3, "table_terms": 0, "bases": 0, "tables": 0, "deferred": 3, "inversion_groups": 1,
            "hash_programs": 1, "prefixes": 1, "flags": 1, "rules": 1, "tally_slots": 0, "derived_points": 0}
    assert {k: d[k] for k in want} == want
    # the other kinds are described as before (spot check of the counts that the new H term touches)
    assert eg.plan_describe("zero")["combs"] == 2 and eg.plan_describe("sumsq", 3)["combs"] == 11


@pytest.fixture(scope="module")
def checklib():
    so = HERE / "libcequivcheck.so"
    srcs = [HERE / "cequivcheck.cpp", ROOT / "elastic_elgamal_amd" / "csrc" / "host_plan.hpp", ROOT / "elastic_elgamal_amd" / "csrc" / "plan.h"]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", str(so), str(HERE / "cequivcheck.cpp")])
    return so


def _run(lib, body: str) -> str:
    asan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    code = textwrap.dedent(f"""
        import ctypes as C
        L = C.CDLL({str(lib)!r})
        L.ce_stride.restype = C.c_ulonglong
        why = C.create_string_buffer(200)
    """) + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={"LD_PRELOAD": asan, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r.stdout


def test_plan_passes_the_index_check_under_sanitizers(checklib):
    out = _run(checklib, """
        assert L.ce_stride() == 224
        for label in (b"", b"t", b"test", b"other_test", bytes(range(256))[1:], b"x" * 255):
            assert L.ce_plan(label, len(label), why, 200) == 3, (label, why.value)
        assert L.ce_others_have_no_h() == 1
        print("ok")
    """)
    assert "ok" in out


def test_index_check_refuses_an_h_scalar_source_out_of_range(checklib):
    out = _run(checklib, """
        assert L.ce_plan_mutated(0, why, 200) == 0, why.value
        for m in (1, 2, 3, 4, 5):
            assert L.ce_plan_mutated(m, why, 200) == 1, (m, why.value)
            print(m, why.value.decode())
    """)
    lines = dict(l.split(" ", 1) for l in out.strip().splitlines())
    assert lines["1"] == "job H scalar out of range" and lines["4"] == "job H scalar out of range"
    assert lines["2"] == "job H scalar source out of range"
    assert lines["3"] == "job H scalar out of range"
    assert "no table of H" in lines["5"]


def test_packer_turns_the_snapshot_object_into_the_item(fx, snap):
    pk, h, label, item = snap
    packed = serde.pack_commitment_equivalence(fx["object"])
    assert packed == item and len(packed) == eg.CommitmentEquivalenceVerifier.ITEM_SIZE
    assert R.verify(pk, h, label, packed) == R.OK
    # examples/equivalence.rs prints the proof under "equiv"
    alt = copy.deepcopy(fx["object"])
    alt["equiv"] = alt.pop("proof")
    assert serde.pack_commitment_equivalence(alt) == item


def test_packer_refuses_bad_base64_and_wrong_lengths(fx):
    paths = [("ciphertext", "random_element"), ("ciphertext", "blinded_element"), ("commitment",), ("proof", "challenge"),
             ("proof", "randomness_response"), ("proof", "value_response"), ("proof", "commitment_response")]

    def with_value(path, v):
        obj = copy.deepcopy(fx["object"])
        d = obj
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = v
        return obj

    for path in paths:
        d = fx["object"]
        for k in path:
            d = d[k]
        for bad in (d + "=", d[:-1] + "*", d[:-1] + "+", d[:-2], d + "AAAA", "", d[:-1] + "B", 5, None):
            if bad == d:
                continue
            with pytest.raises(serde.SerdeError):
                serde.pack_commitment_equivalence(with_value(path, bad))
    both = copy.deepcopy(fx["object"])
    both["equiv"] = both["proof"]
    with pytest.raises(serde.SerdeError):
        serde.pack_commitment_equivalence(both)
    neither = copy.deepcopy(fx["object"])
    del neither["proof"]
    with pytest.raises(serde.SerdeError):
        serde.pack_commitment_equivalence(neither)
