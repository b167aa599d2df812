"""The provers of the zero, bool, range, sum-of-squares and decryption-share proofs without a GPU: the new entries of the C ABI and
their bindings, the input validator and the workspace counts under ASan + UBSan (tests/hostcheck/provecheck.cpp), and the plans of
every existing kind, which the provers must leave as they were (tests/golden/plan_describe_before_provers.json)."""
import ctypes as C
import json
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
NEW_SYMBOLS = ("eg_proof_prove_input_size", "eg_proof_prove_batch", "eg_proof_prove_batch_device", "eg_share_prove_batch",
               "eg_share_prove_batch_device")
L = 2**252 + 27742317777372353535851937790883648493


def test_library_declares_exports_and_binds_the_new_entries():
    lib = eg._load()
    hdr = (ROOT / "include" / "eg_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert name in eg.exported_symbols(), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name          # the binding gave it a prototype
        assert hdr.count(name + "(") == 1, name
    assert lib.eg_proof_prove_input_size.restype is C.c_size_t
    assert lib.eg_proof_prove_input_size(None) == 0


def test_abi_version_is_still_the_headers():
    hdr = (ROOT / "include" / "eg_hip.h").read_text()
    line = next(l for l in hdr.splitlines() if l.startswith("#define EG_ABI_VERSION"))
    assert eg.ABI_VERSION == eg._load().eg_abi_version() == int(line.split()[2])


def test_python_methods_exist():
    for cls in (eg.PublicKeyVerifier, eg.SumOfSquaresVerifier, eg.DecryptionShareVerifier):
        for m in ("prove", "prove_device", "verify_batch", "verify_device"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert eg.SumOfSquaresVerifier.prove is eg.PublicKeyVerifier.prove
    assert eg.DecryptionShareVerifier.prove is not eg.PublicKeyVerifier.prove            # it takes the secret share
    assert eg.CommitmentEquivalenceVerifier.prove is not eg.PublicKeyVerifier.prove      # it keeps its own entry (blindings)


def test_cpp_mirror_has_the_provers(tmp_path):
    src = tmp_path / "provers.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace elastic_elgamal_hip;
        int main(int argc, char**) {
          if (argc < 100) return 0;            // compiled and linked against the C ABI; running it needs a GPU
          Context ctx(0);
          Element pk{};
          Scalar sk{};
          ZeroEncryption z(ctx, pk);
          BoolEncryption b(ctx, pk);
          RangeEncryption r(ctx, pk, 100);
          SumOfSquares s(ctx, pk, 2, "test");
          DecryptionShares d(ctx, pk, 3, 2, 0, pk);
          Bytes all = z.encrypt_zero(1, 0, 4);
          Bytes bb = b.encrypt_bool(1, 0, {true, false});
          Bytes rr = r.encrypt_range(1, 0, {0, 99}, 1);
          Bytes ss = s.prove(1, 0, {1, 2, 3, 4});
          std::vector<uint8_t> ok;
          Bytes dd = d.decrypt_share(sk, 1, 0, {pk, pk}, &ok);
          return (int)(z.verify_batch(all).size() + b.verify_batch(bb).size() + r.verify_batch(rr).size() + s.verify_batch(ss).size() +
                       d.verify_batch(dd).size() + r.item_size());
        }
    """))
    exe = tmp_path / "provers"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert exe.exists()


# ------------------------------------------------------------------ host logic under sanitizers
@pytest.fixture(scope="module")
def checklib():
    so = HERE / "libprovecheck.so"
    srcs = [HERE / "provecheck.cpp", ROOT / "elastic_elgamal_amd" / "csrc" / "host_plan.hpp", ROOT / "elastic_elgamal_amd" / "csrc" / "plan.h"]
    if not so.exists() or any(s.stat().st_mtime > so.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", str(so), str(HERE / "provecheck.cpp")])
    return so


def _run(lib, body: str) -> str:
    asan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    code = textwrap.dedent(f"""
        import ctypes as C
        L = C.CDLL({str(lib)!r})
        U = C.c_ulonglong
        why = C.create_string_buffer(200)
        def check(kind, bound, n_values, rows):
            flat = [x for r in rows for x in r]
            arr = (U * max(len(flat), 1))(*flat)
            rc = L.pc_check(kind, U(bound), n_values, arr if flat else None, U(len(rows)), why, 200)
            return rc, why.value.decode()
        ZERO, BOOL, RANGE, SHARE, SUMSQ, CEQUIV = 0, 1, 2, 3, 4, 5
    """) + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env={"LD_PRELOAD": asan, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r.stdout


def test_input_validator_under_sanitizers(checklib):
    out = _run(checklib, """
        M = 2**64 - 1
        assert [L.pc_inputs_per_item(k, 7) for k in (ZERO, BOOL, RANGE, SHARE, SUMSQ, CEQUIV, 9)] == [0, 1, 1, -1, 7, -1, -1]
        # the edge values are admissible
        assert check(ZERO, 0, 0, []) == (0, "")
        assert check(BOOL, 0, 0, [[0], [1]]) == (0, "")
        for ub in (2, 5, 100, 10**6):
            assert check(RANGE, ub, 0, [[0], [1], [ub - 1]]) == (0, ""), ub
        assert check(SUMSQ, 0, 1, [[2**32 - 1], [0]]) == (0, "")                         # (2^32 - 1)^2 < 2^64
        assert check(SUMSQ, 0, 2, [[2**32 - 1, 92681]]) == (0, "")                       # 2^64 - 2^33 + 1 + 92681^2 = 2^64 - 166830
        assert check(SUMSQ, 0, 16, [[2**30] * 15 + [2**30 - 1]]) == (0, "")              # 16 * 2^60 - 2^31 + 1 = 2^64 - 2^31 + 1
        assert check(SUMSQ, 0, 3, [[0, 0, 0]]) == (0, "")
        # what the reference panics on (or overflows) is refused, wherever in the batch it sits
        assert check(BOOL, 0, 0, [[0], [1], [2]]) == (1, "a bool is 0 or 1")
        assert check(BOOL, 0, 0, [[M]])[0] == 1
        for ub in (2, 5, 100, 10**6):
            assert check(RANGE, ub, 0, [[0], [ub]]) == (1, "value out of range"), ub
            assert check(RANGE, ub, 0, [[M]])[0] == 1
        assert check(SUMSQ, 0, 1, [[2**32]]) == (1, "the sum of squares does not fit 64 bits")
        assert check(SUMSQ, 0, 2, [[1, 1], [2**32 - 1, 92682]])[0] == 1                  # 92682^2 is 185363 more: 2^64 + 18533
        assert check(SUMSQ, 0, 16, [[2**30] * 16])[0] == 1                               # exactly 2^64
        assert check(SUMSQ, 0, 2, [[M, M]])[0] == 1                                      # needs the 128-bit sum: 2 M^2 mod 2^64 is small
        assert check(SUMSQ, 0, 3, [[2**63, 2**63, 5]])[0] == 1                           # 2^126 + 2^126 + 25: wraps to 25 in 64 bits
        # the kinds that have no value-driven prover, and a missing buffer
        assert check(SHARE, 0, 0, [])[0] == 1 and check(CEQUIV, 0, 0, [])[0] == 1 and check(9, 0, 0, [])[0] == 1
        assert L.pc_check(BOOL, U(0), 0, None, U(3), why, 200) == 1 and why.value == b"inputs missing"
        assert L.pc_check(ZERO, U(0), 0, None, U(3), why, 200) == 0
        print("ok")
    """)
    assert "ok" in out


def test_secret_share_canonicity_under_sanitizers(checklib):
    out = _run(checklib, f"""
        l = {L}
        enc = lambda x: x.to_bytes(32, "little")
        for x in (0, 1, l - 1, 2**252, l // 2):
            assert L.pc_scalar_canonical(enc(x)) == 1, x
        for x in (l, l + 1, 2**253, 2**255, 2**256 - 1, l + 2**128):
            assert L.pc_scalar_canonical(enc(x)) == 0, x
        print("ok")
    """)
    assert "ok" in out


def test_workspace_counts_against_a_python_count(checklib):
    """Words per lane: a range proof keeps, per ring, the value index (1), the ring's randomness, its commitment scalar and the two
    terminal commitments (4 x 8), and 8 per response; a sum of squares the value (1) and r, e_r, e_x (3 x 8) per value; a decryption
    share the eight cached points {1..8}R of 4 field elements of 9 limbs."""
    bounds = [2, 3, 5, 12, 15, 20, 50, 100, 101, 1000, 65536, 777777, 1000000]
    out = _run(checklib, f"""
        import json
        res = {{}}
        for ub in {bounds}:
            nr, resp = C.c_uint(), C.c_uint()
            w = L.pc_range_ws_words(U(ub), C.byref(nr), C.byref(resp))
            res[ub] = [w, nr.value, resp.value]
        print(json.dumps({{"range": res, "sumsq": [L.pc_sumsq_ws_words(n) for n in (1, 2, 5, 16, 1000)], "share": L.pc_share_ws_words(),
                          "prefix": [[L.pc_gen_prefix(k, w) for w in range(4)] for k in range(5)]}}))
    """)
    got = json.loads(out.strip().splitlines()[-1])
    for ub in bounds:
        rings = [part.split("0..")[1] for part in eg.range_decomposition(ub).split(" + ")]
        sizes = [int(x) for x in rings]
        w, nr, resp = got["range"][str(ub)]
        assert (nr, resp) == (len(sizes), sum(sizes)), ub
        assert w == sum(1 + 4 * 8 for _ in sizes) + 8 * sum(sizes), ub
    assert got["sumsq"] == [(1 + 3 * 8) * n for n in (1, 2, 5, 16, 1000)]
    assert got["share"] == 8 * 4 * 9
    # the provers import prefixes that their plans hoist: main/ring for the ring proofs, the log-equality / sum-of-squares one otherwise
    zero, boo, rng, share, sumsq = got["prefix"]
    assert zero == [-1, -1, 0, -1] and share == [-1, -1, 0, -1] and sumsq == [-1, -1, -1, 0]
    assert boo[:2] == [0, 1] and rng[:2] == [0, 1] and boo[2:] == rng[2:] == [-1, -1]


# ------------------------------------------------------------------ the plans are untouched
def test_plan_describe_of_every_existing_kind_is_what_it_was():
    before = json.loads((ROOT / "tests" / "golden" / "plan_describe_before_provers.json").read_text())
    assert {c[0] for c in before} == {"single", "multi", "qv", "zero", "bool", "range", "sumsq", "commit_equiv"}
    for kind, n, c, want in before:
        assert eg.plan_describe(kind, n, c) == want, (kind, n, c)
