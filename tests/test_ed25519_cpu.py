"""Voter signatures (eg_ed25519_*, eg_sha512_*) without a GPU:
* the RFC 8032 model of tests/ed25519_ref.py against the OpenSSL-made fixture tests/golden/ed25519_openssl.json (verifier and signer,
  byte for byte), its refusals and the stated details;
* tests/hostcheck/ed25519check.cpp: sha512.cuh, ed25519.cuh and ed25519_host.hpp under -DEG_BOUNDCHECK with ASan + UBSan, the lane
  functions of the kernels run serially.  Expected values come from hashlib, the fixture and the model;
* every refusal of every new entry that needs no GPU; the new symbols declared, exported, bound and mirrored; ABI version 7; plain C99."""
import ctypes as C
import hashlib
import json
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import ed25519_ref as R
import elastic_elgamal_amd as eg

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
FIXTURE = [{k: bytes.fromhex(v) if k != "source" else v for k, v in e.items()}
           for e in json.loads((ROOT / "tests" / "golden" / "ed25519_openssl.json").read_text())["entries"]]
BAD_ARG = -3
ENTRIES = {  # name: (return type in the header, restype, number of arguments)
    "eg_ed25519_verify_scratch_bytes": ("size_t", C.c_size_t, 2),
    "eg_ed25519_verify_device": ("int", C.c_int, 16),
    "eg_ed25519_verify_batch": ("int", C.c_int, 13),
    "eg_ed25519_keypair_batch": ("int", C.c_int, 4),
    "eg_ed25519_keypair_batch_device": ("int", C.c_int, 5),
    "eg_ed25519_sign_batch": ("int", C.c_int, 9),
    "eg_ed25519_sign_batch_device": ("int", C.c_int, 10),
    "eg_sha512_batch": ("int", C.c_int, 8),
    "eg_sha512_batch_device": ("int", C.c_int, 9),
}


def flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


# ------------------------------------------------------------------ the model against the fixture
def test_fixture_covers_the_lengths_around_the_block_seams():
    lengths = {len(e["message"]) for e in FIXTURE}
    assert {0, 1, 3, 47, 48, 49, 111, 112, 113, 127, 128, 129, 736, 2144} <= lengths and 28 <= len(FIXTURE) <= 36
    assert sum(e["source"] == "openssl" for e in FIXTURE) >= 28


def test_model_accepts_every_entry_and_rejects_a_flipped_bit_anywhere():
    for e in FIXTURE:
        pk, m, s = e["public_key"], e["message"], e["signature"]
        assert R.verify_detail(pk, m, s) == 0
        assert R.verify_detail(pk, m, flip(s, 3)) == R.MISMATCH                    # R
        assert R.verify_detail(pk, m, flip(s, 256 + 17)) == R.MISMATCH             # S, still canonical
        assert R.verify_detail(pk, m, flip(s, 511)) == R.BAD_S                     # S above l
        assert R.verify_detail(flip(pk, 9), m, s) in (R.BAD_KEY, R.MISMATCH)       # A
        assert R.verify_detail(pk, m + b"\0", s) == R.MISMATCH
        if m:
            assert R.verify_detail(pk, flip(m, 0), s) == R.MISMATCH
        for tampered_key in (flip(pk, 9), pk):
            for sig in (flip(s, 3), flip(s, 511)):
                assert R.expected_status(tampered_key, m, sig, True) == R.status_word(R.verify_detail(tampered_key, m, sig))
        assert R.expected_status(pk, m, s, False) == 0 and R.expected_status(pk, m, s, True, index_ok=False) == R.status_word(R.BAD_INDEX)


def test_models_signer_reproduces_keys_and_signatures_byte_for_byte():
    for e in FIXTURE:
        assert R.public_key(e["seed"]) == e["public_key"]
        assert R.sign(e["seed"], e["message"]) == e["signature"]


def test_refused_keys_get_the_stated_detail():
    e = FIXTURE[3]
    m, s = e["message"], e["signature"]
    small = R.small_order_encodings()
    assert len(set(small)) == 8 and (1).to_bytes(32, "little") in small and (R.P - 1).to_bytes(32, "little") in small and bytes(32) in small
    for enc in small:
        assert R.verify_detail(enc, m, s) == R.SMALL_ORDER
    for enc in (R.P.to_bytes(32, "little"), (R.P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little"),
                ((R.P - 1) | 1 << 255).to_bytes(32, "little"), bytes([0xFF] * 32)):
        assert R.verify_detail(enc, m, s) == R.BAD_KEY, enc.hex()
    assert R.status_word(R.BAD_KEY) == 15 | 2 << 8 and R.status_word(0) == 0
    # first failure wins: S >= l in front of a bad key
    assert R.verify_detail(bytes([0xFF] * 32), m, s[:32] + R.L.to_bytes(32, "little")) == R.BAD_S


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_bound_and_mirrored():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for name, (ret, restype, nargs) in ENTRIES.items():
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in eg.exported_symbols()
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    for phrase in ("COFACTORLESS", "TIMING: variable time throughout", "STRICT", "R is never decoded", "not for a voter client"):
        assert phrase in header, phrase
    for m in ("keypairs", "sign", "verify", "verify_device", "sha512", "verify_scratch_bytes"):
        assert callable(getattr(eg.Ed25519, m)), m
    assert "Ed25519" in eg.__all__
    ffi = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    assert int(re.search(r"EG_ST_BAD_SIGNATURE = (\d+)", header).group(1)) == eg.ST_BAD_SIGNATURE == R.ST_BAD_SIGNATURE == 15
    assert eg.STATUS_NAMES[15] == "BadSignature" and eg.STATUS_NAMES[14] == "Duplicate"
    for name, value in (("BAD_S", 1), ("BAD_KEY", 2), ("SMALL_ORDER", 3), ("MISMATCH", 4), ("BAD_INDEX", 5)):
        assert re.search(rf"EG_ED25519_{name} = {value}\b", header) and getattr(eg, "ED25519_" + name) == getattr(R, name) == value
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7
    lanes = (CSRC / "ed25519.cuh").read_text()
    assert "ED_ST_BAD_SIGNATURE = 15" in lanes and "ED_BAD_S = 1, ED_BAD_KEY = 2, ED_SMALL_ORDER = 3, ED_MISMATCH = 4, ED_BAD_INDEX = 5" in lanes
    assert "TIMING" in lanes and "COFACTORLESS" in lanes


def test_cpp_mirror_compiles(tmp_path):
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Ed25519 ed{ctx};
            Bytes seeds(64), msgs(20), prefix(3);
            Bytes keys = ed.keypairs(seeds), sigs = ed.sign(seeds, msgs, 10, prefix);
            std::vector<uint32_t> st = ed.verify(msgs, 10, keys, sigs, prefix, {1, 0}, {0, 0});
            ed.verify_device(0, nullptr, 0, 0, prefix, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, ed.verify_scratch_bytes(0));
            ed.keypairs_device(0, nullptr, nullptr);
            ed.sign_device(0, nullptr, nullptr, 0, 0, nullptr, 0, nullptr);
            ed.sha512_device(0, nullptr, 0, 0, nullptr, 0, nullptr);
            return (int)(st.size() + ed.sha512(2, msgs, 10).size());
          }
          static_assert(EG_ST_BAD_SIGNATURE == 15 && EG_ED25519_MISMATCH == 4 && EG_ED25519_BAD_INDEX == 5, "header constants");
          return 0;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_ST_BAD_SIGNATURE == 15 && EG_ED25519_BAD_S == 1 && eg_ed25519_verify_device && '
                   'eg_ed25519_verify_batch && eg_ed25519_sign_batch && eg_ed25519_keypair_batch_device && eg_sha512_batch ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob():
    for f in ("sha512.cuh", "ed25519.cuh", "ed25519_kernels.cuh", "ed25519_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()


# ------------------------------------------------------------------ refusals that need no GPU
def test_refusals_without_a_gpu():
    """the argument rules come before the context is looked at; what passes them fails on the missing context"""
    lib = eg._load()
    buf = C.create_string_buffer(512)
    base = (C.addressof(buf) + 15) & ~15
    one = (C.c_uint32 * 4)()

    def vdev(n=1, msgs=base, stride=8, length=8, prefix=b"p", plen=1, keys=base, n_keys=1, index=None, sigs=base, out=one, scratch=base, sbytes=1 << 20):
        rc = lib.eg_ed25519_verify_device(None, n, msgs, stride, length, prefix, plen, keys, n_keys, index, sigs, None, out, scratch, sbytes, None)
        return rc, lib.eg_last_error()

    def vhost(n=1, msgs=b"12345678", stride=8, length=8, prefix=b"p", plen=1, keys=bytes(32), n_keys=1, index=None, sigs=bytes(64), out=one, **_):
        rc = lib.eg_ed25519_verify_batch(None, n, msgs, stride, length, prefix, plen, keys, n_keys, index, sigs, None, out)
        return rc, lib.eg_last_error()

    for call in (vdev, vhost):
        for kw, text in (({"n": 1 << 31}, b"n is 2^31 or more"), ({"n": 1 << 40}, b"n is 2^31 or more"), ({"plen": 256}, b"prefix_len is above 255"),
                         ({"prefix": None}, b"null prefix with prefix_len > 0"), ({"stride": 7}, b"msg_stride is below msg_len"),
                         ({"msgs": None}, b"null msgs"), ({"keys": None}, b"null keys, sigs or status_out"), ({"sigs": None}, b"null keys, sigs or status_out"),
                         ({"out": None}, b"null keys, sigs or status_out"), ({"n_keys": 0, "index": one}, b"n_keys is 0"),
                         ({"n_keys": 2}, b"n_keys must equal n"), ({"n": 2, "n_keys": 1}, b"n_keys must equal n")):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and text in msg, (call.__name__, kw, msg)
        # what is within the rules fails on the missing context: the limits themselves are not over the limit
        for kw in ({}, {"plen": 0, "prefix": None}, {"prefix": b"x" * 255, "plen": 255}, {"n": 4, "n_keys": 1, "index": one},
                   {"n": (1 << 31) - 1, "n_keys": (1 << 31) - 1}, {"n": 0, "n_keys": 0, "msgs": None, "keys": None, "sigs": None, "out": None},
                   {"length": 0, "stride": 0, "msgs": None}):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and b"null ctx" in msg, (call.__name__, kw, msg)
    for kw in ({"keys": base + 1}, {"sigs": base + 2}, {"out": C.addressof(one) + 1}, {"n": 4, "index": C.addressof(one) + 2}):
        rc, msg = vdev(**kw)
        assert rc == BAD_ARG and b"4-byte aligned" in msg, kw
    assert lib.eg_ed25519_verify_scratch_bytes(None, 100) == 0

    sig64, dig64 = C.create_string_buffer(64), C.create_string_buffer(64)
    cases = (
        (lambda **k: lib.eg_ed25519_sign_batch(None, k.get("n", 1), k.get("seeds", bytes(32)), k.get("msgs", b"12345678"), k.get("stride", 8), 8,
                                               k.get("prefix", b"p"), k.get("plen", 1), k.get("out", sig64)), b"null seeds or sigs"),
        (lambda **k: lib.eg_ed25519_sign_batch_device(None, k.get("n", 1), k.get("seeds", base), k.get("msgs", base), k.get("stride", 8), 8,
                                                      k.get("prefix", base), k.get("plen", 1), k.get("out", base), None), b"null seeds or sigs"),
        (lambda **k: lib.eg_sha512_batch(None, k.get("n", 1), k.get("msgs", b"12345678"), k.get("stride", 8), 8, k.get("prefix", b"p"), k.get("plen", 1),
                                         k.get("out", dig64)), b"digests null"),
        (lambda **k: lib.eg_sha512_batch_device(None, k.get("n", 1), k.get("msgs", base), k.get("stride", 8), 8, k.get("prefix", base), k.get("plen", 1),
                                                k.get("out", base), None), b"digests null"),
    )
    for call, null_out in cases:
        for kw, text in (({"n": 1 << 31}, b"n is 2^31 or more"), ({"plen": 256}, b"prefix_len is above 255"), ({"prefix": None}, b"null prefix"),
                         ({"stride": 7}, b"msg_stride is below msg_len"), ({"msgs": None}, b"null msgs"), ({"out": None}, null_out[:4])):
            assert call(**kw) == BAD_ARG and text in lib.eg_last_error(), kw
        assert call() == BAD_ARG and b"null ctx" in lib.eg_last_error()
    assert lib.eg_ed25519_sign_batch(None, 1, None, b"12345678", 8, 8, None, 0, sig64) == BAD_ARG and b"null seeds" in lib.eg_last_error()
    for rc in (lib.eg_ed25519_keypair_batch(None, 1 << 31, bytes(32), sig64), lib.eg_ed25519_keypair_batch_device(None, 1 << 31, base, base, None)):
        assert rc == BAD_ARG and b"n is 2^31 or more" in lib.eg_last_error()
    for rc in (lib.eg_ed25519_keypair_batch(None, 1, None, sig64), lib.eg_ed25519_keypair_batch_device(None, 1, base, None, None),
               lib.eg_ed25519_keypair_batch_device(None, 1, base, base + 2, None)):
        assert rc == BAD_ARG and b"null seeds or keys" in lib.eg_last_error()
    for rc in (lib.eg_ed25519_keypair_batch(None, 1, bytes(32), sig64), lib.eg_ed25519_keypair_batch_device(None, 0, None, None, None)):
        assert rc == BAD_ARG and b"null ctx" in lib.eg_last_error()


def test_missing_gpu_is_loud():
    ed = object.__new__(eg.Ed25519)
    ed.ctx = type("NoCtx", (), {"_h": None})()
    with pytest.raises(eg.EgError, match="null ctx"):
        ed.verify(bytes(8), 8, bytes(32), bytes(64))
    with pytest.raises(eg.EgError, match="null ctx"):
        ed.sign(bytes(32), bytes(8), 8)
    with pytest.raises(eg.EgError, match="null ctx"):
        ed.sha512(bytes(8), 8)
    with pytest.raises(eg.EgError, match="n_keys must equal n"):
        ed.verify(bytes(16), 8, bytes(32), bytes(128))
    assert ed.verify_scratch_bytes(10) == 0


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "ed25519check", HERE / "ed25519check.cpp"
    deps = [src, *CSRC.glob("*.cuh"), *CSRC.glob("*.hpp"), CSRC / "plan.h"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args, ok=True):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        if ok:
            assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout if ok else r

    return run


def test_hostcheck_sha512_every_length_every_cut_every_alignment(check, tmp_path):
    """total lengths 0..300 against hashlib, the message cut into four ranges (empty ones included) that start at every offset mod 8"""
    lines = []
    for n in range(0, 301):
        m = (hashlib.sha512(b"m%d" % n).digest() * 5)[:n]
        d = hashlib.sha512(m).hexdigest()
        cuts = {(0, 0, 0), (n, 0, 0), (min(n, 32), min(max(n - 32, 0), 32), min(max(n - 64, 0), n % 7)), (n // 5, n // 3, min(n - n // 5 - n // 3, 7)),
                (min(n, 1), 0, min(max(n - 1, 0), 127)), (0, min(n, 128), 0)}
        for k, (a, b, c) in enumerate(sorted(cuts)):
            lines.append(f"{(n + k) % 8} {a} {b} {c} {hx(m)} {d}")
        if n in (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 300):
            for shift in range(8):
                lines.append(f"{shift} {min(n, 32)} {min(max(n - 32, 0), 32)} {min(max(n - 64, 0), 19)} {hx(m)} {d}")
    path = tmp_path / "sha.txt"
    path.write_text("\n".join(lines) + "\n")
    assert f"SHA {len(lines)}\n" in check("sha", path)


def test_hostcheck_codec_round_trips_and_refusals(check, tmp_path):
    lines = [f"{enc.hex()} 3" for enc in R.small_order_encodings()]
    lines += [f"{e['public_key'].hex()} 0" for e in FIXTURE] + [f"{e['signature'][:32].hex()} 0" for e in FIXTURE[:8]]
    no_root = [y for y in range(2, 60) if R.decode(y.to_bytes(32, "little")) is None]
    roots = [y for y in range(2, 60) if R.decode(y.to_bytes(32, "little")) is not None]
    assert no_root and roots
    lines += [f"{y.to_bytes(32, 'little').hex()} 2" for y in no_root]
    for y in roots:                                        # both signs of x
        for sign in (0, 1):
            enc = (y | sign << 255).to_bytes(32, "little")
            lines.append(f"{enc.hex()} {3 if R.is_small_order(R.decode(enc)) else 0}")
    for v in (R.P, R.P + 1, R.P + 18, (1 << 255) - 1, 1 | 1 << 255, (R.P - 1) | 1 << 255, (1 << 256) - 1, R.P | 1 << 255):
        lines.append(f"{v.to_bytes(32, 'little').hex()} 2")
    path = tmp_path / "codec.txt"
    path.write_text("\n".join(lines) + "\n")
    assert f"CODEC {len(lines)}\n" in check("codec", path)


def test_hostcheck_verify_lane_on_the_fixture_and_its_tampered_twins(check, tmp_path):
    lines, accepted = [], 0
    small = R.small_order_encodings()
    for i, e in enumerate(FIXTURE):
        pk, m, s = e["public_key"], e["message"], e["signature"]
        twins = [(b"", m, pk, s), (b"", m, pk, flip(s, i % 256)), (b"", m, pk, flip(s, 256 + i % 252)), (b"", m, flip(pk, i % 256), s),
                 (b"x", m, pk, s), (b"", m + b"\0", pk, s)]
        if m:
            twins += [(b"", flip(m, (37 * i) % (8 * len(m))), pk, s), (m[:1], m[1:], pk, s), (m, b"", pk, s)]       # the prefix only shifts the cut
        if i < 8:
            twins.append((b"", m, small[i], s))
        for prefix, msg, key, sig in twins:
            want = R.status_word(R.verify_detail(key, prefix + msg, sig))
            accepted += want == 0
            lines.append(f"{hx(prefix)} {hx(msg)} {key.hex()} {sig.hex()} {want}")
    # S in {0, 1, l - 1, l, l + 1, 2^256 - 1}: canonical ones are a mismatch (or whatever the model says), the others detail 1
    e = FIXTURE[5]
    for v in (0, 1, R.L - 1, R.L, R.L + 1, (1 << 256) - 1):
        sig = e["signature"][:32] + v.to_bytes(32, "little")
        want = R.status_word(R.verify_detail(e["public_key"], e["message"], sig))
        assert want == R.status_word(R.BAD_S if v >= R.L else R.MISMATCH)
        lines.append(f"- {hx(e['message'])} {e['public_key'].hex()} {sig.hex()} {want}")
    # first failure wins: S >= l in front of a key that does not decode, a key that does not decode in front of everything else
    bad_key = R.P.to_bytes(32, "little")
    lines.append(f"- {hx(e['message'])} {bad_key.hex()} {(e['signature'][:32] + R.L.to_bytes(32, 'little')).hex()} {R.status_word(R.BAD_S)}")
    lines.append(f"- {hx(e['message'])} {bad_key.hex()} {e['signature'].hex()} {R.status_word(R.BAD_KEY)}")
    path = tmp_path / "verify.txt"
    path.write_text("\n".join(lines) + "\n")
    out = check("verify", path)
    assert f"VERIFY {len(lines)} ACCEPTED {accepted}\n" in out and accepted >= 2 * len(FIXTURE) - 2


def test_hostcheck_sign_lane_reproduces_the_fixture(check, tmp_path):
    lines = [f"{e['seed'].hex()} - {hx(e['message'])} {e['public_key'].hex()} {e['signature'].hex()}" for e in FIXTURE]
    for e in FIXTURE:                                          # with a prefix: the same bytes signed, cut elsewhere
        m = e["message"]
        if len(m) >= 3:
            lines.append(f"{e['seed'].hex()} {m[:3].hex()} {hx(m[3:])} {e['public_key'].hex()} {e['signature'].hex()}")
    path = tmp_path / "sign.txt"
    path.write_text("\n".join(lines) + "\n")
    assert f"SIGN {len(lines)}\n" in check("sign", path)


def test_hostcheck_layout_against_a_direct_count(check):
    def up(x):
        return (x + 255) // 256 * 256

    for n, cus in ((0, 256), (1, 256), (256, 256), (257, 256), (65536, 256), (1 << 20, 256), (1 << 20, 8), ((1 << 31) - 1, 304)):
        blocks = min((n + 255) // 256, 4 * cus)
        prefix = 256 if n else 0
        h, tables = up(32 * n), blocks * 256 * 1152
        out = check("layout", n, cus)
        assert f"LAYOUT blocks {blocks} prefix 0 h {prefix} tables {prefix + h} total {prefix + h + up(tables)}\n" in out, (n, cus, out)


def test_hostcheck_refusal_rules(check):
    def refuse(n=1, have_msgs=1, stride=8, length=8, have_prefix=1, plen=1, n_keys=1, have_index=0):
        return check("refuse", n, have_msgs, stride, length, have_prefix, plen, n_keys, have_index).split("\n")[0]

    assert refuse() == "REFUSE -" and refuse(n=0, n_keys=0, have_msgs=0) == "REFUSE -" and refuse(plen=255) == "REFUSE -"
    assert refuse(n=(1 << 31) - 1, n_keys=(1 << 31) - 1) == "REFUSE -" and refuse(n=5, n_keys=2, have_index=1) == "REFUSE -"
    assert refuse(n=1 << 31) == "REFUSE n is 2^31 or more"
    assert refuse(plen=256) == "REFUSE prefix_len is above 255"
    assert refuse(have_prefix=0) == "REFUSE null prefix with prefix_len > 0" and refuse(have_prefix=0, plen=0) == "REFUSE -"
    assert refuse(stride=7) == "REFUSE msg_stride is below msg_len"
    assert refuse(have_msgs=0) == "REFUSE null msgs" and refuse(have_msgs=0, length=0, stride=0) == "REFUSE -"
    assert refuse(n_keys=0, have_index=1) == "REFUSE n_keys is 0"
    assert refuse(n_keys=2) == "REFUSE no key_index: n_keys must equal n"
