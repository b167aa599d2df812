"""The shuffle verifier (eg_shuffle_*) without a GPU:
* the model tests/shuffle_ref.py checks itself over the oracle backend: completeness for every N = 1 .. 40 and three kinds of
  permutation, blobs of the wrong length, a flipped bit in every section of statement, key, prefix and proof, and the lying provers
  with the bits they must set;
* tests/hostcheck/shufflecheck.cpp: shuffle_kernels.cuh and shuffle_host.hpp under -DEG_BOUNDCHECK with ASan + UBSan, the lane functions
  run serially in the kernels' arrangement (the chain in tiles of 63 rows with the neighbour's point handed over) against the model,
  hashlib and Python integers;
* every refusal of every entry that needs no GPU, the sizes, the symbols, the mirrors, the plain-C header."""
import ctypes as C
import hashlib
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

import shuffle_cases as SC
import shuffle_ref as M

ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "hostcheck"
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
MANY_TRIES_SEED = b"eg-shuffle many tries 0"
NONE4 = [0, 0, M.NONE, M.NONE]


@pytest.fixture(scope="module")
def be(oracle):
    return M.OracleBackend()


@pytest.fixture(scope="module")
def K(be):
    return be.mul_generator([0xC0FFEE])[0]


@pytest.fixture(scope="module")
def key(be):
    return M.derive_key(be, SC.SEED, 70)


_cases = {}


def case_of(be, K, key, n, perm="random"):
    if (n, perm) not in _cases:
        _cases[n, perm] = M.make(be, K, key, SC.PREFIX, n, 1000 * len(perm) + n, perm)
    return _cases[n, perm]


# ------------------------------------------------------------------ the model checks itself
@pytest.mark.parametrize("perm", ["random", "identity", "reverse"])
def test_model_accepts_every_honest_shuffle(be, K, key, perm):
    for n in range(1, 41):
        c = case_of(be, K, key, n, perm)
        assert M.verify(be, c["ins"], c["outs"], K, key, SC.PREFIX, c["proof"]) == (0, [0] * n, NONE4), n


def test_model_key(be):
    key, used = M.derive_key(be, MANY_TRIES_SEED, 8, with_tries=True)
    assert used == [4, 21, 30, 26, 5, 3, 12, 5, 12]                      # the pinned seed: three generators beyond 20 candidates
    assert all(be.decodes(key)) and M.IDENTITY not in key and len(set(key)) == 9
    assert M.derive_key(be, MANY_TRIES_SEED, 3) == key[:4]               # H_j does not depend on cap
    for j, h in enumerate(key):                                           # no earlier candidate was an element
        assert h == M.key_candidate(MANY_TRIES_SEED, j, used[j] - 1)
        assert not any(be.decodes([M.key_candidate(MANY_TRIES_SEED, j, c) for c in range(used[j] - 1)]))
    with pytest.raises(ValueError):
        M.derive_key(be, MANY_TRIES_SEED, 8, tries=29)


def test_model_refuses_wrong_lengths(be, K, key):
    c = case_of(be, K, key, 5)
    for proof in (c["proof"][:-1], c["proof"] + b"\0", c["proof"][:-32], c["proof"] + bytes(160), b""):
        with pytest.raises(ValueError):
            M.verify(be, c["ins"], c["outs"], K, key, SC.PREFIX, proof)
    with pytest.raises(ValueError):
        M.verify(be, c["ins"], c["outs"][:-1], K, key, SC.PREFIX, c["proof"])
    with pytest.raises(ValueError):
        M.verify(be, c["ins"], c["outs"], K, key[:5], SC.PREFIX, c["proof"])
    assert M.verify(be, [], [], K, key, SC.PREFIX, bytes(288)) == (0, [], NONE4)


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_every_tampered_twin_is_rejected(be, K, key, n):
    c = case_of(be, K, key, n)
    seen = 0
    for t in SC.tampered(c, K, key):
        mask, rows, found = SC.judge(be, t)
        assert mask != 0, t["name"]
        assert found == M.found_of(rows)
        if mask & M.BAD_ENCODING:
            assert mask == M.BAD_ENCODING, t["name"]                     # the other bits are masked
        seen |= mask
    assert seen == 127
    # bad scalars and points name their rows
    k = n // 2
    by = {t["name"]: SC.judge(be, t) for t in SC.tampered(c, K, key)}
    assert by["shat_is_l"][1][n - 1] & M.ROW_BAD and by["shat_is_l"][2][2] == n - 1
    assert by["c_not_a_point"][1][0] & M.ROW_BAD and by["c_not_a_point"][2][:3:2] == [1, 0]
    assert by["out_R_not_a_point"][1][k] & M.ROW_BAD          # (c and out are hashed: the rows fail CHAIN as well)
    assert by["K_not_a_point"][0] == M.BAD_ENCODING and by["K_not_a_point"][2][0] == 0      # no row is at fault
    assert by["s4_is_max"] == (M.BAD_ENCODING, [0] * n, NONE4)
    # a flipped bit in t^_k of a finished proof changes the challenge: everything fails, and no encoding is bad
    assert by["that_bit"][0] == 126 and by["t1_not_canonical"][0] == 126


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_lying_provers_set_the_stated_bits(be, K, key, n):
    c = case_of(be, K, key, n)
    for t in SC.lying(be, c, K, key, 4000 + n):
        mask, rows, found = SC.judge(be, t)
        if t["name"] == "that_flip":
            k = t["row"]
            assert (mask, rows, found) == (M.CHAIN, [M.ROW_CHAIN if i == k else 0 for i in range(n)], [0, 1, M.NONE, k])
        elif t["name"] == "other_message":
            assert (mask, rows, found) == (M.T41, [0] * n, NONE4)
        elif t["name"] == "two_on_one_H":
            assert mask and not mask & ~(M.T1 | M.T3) and not any(rows)
        else:
            assert mask != 0 and not mask & M.BAD_ENCODING, t["name"]


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "shufflecheck", HERE / "shufflecheck.cpp"
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


def hx(b: bytes) -> str:
    return b.hex() or "-"


def test_key_lanes(check, be, tmp_path):
    key, used = M.derive_key(be, MANY_TRIES_SEED, 8, with_tries=True)
    key2 = M.derive_key(be, b"", 2)
    long_seed = bytes(range(255))
    key3 = M.derive_key(be, long_seed, 1)
    lines = [f"{hx(MANY_TRIES_SEED)} {j} 4096" for j in range(9)] + [f"- {j} 4096" for j in range(3)] + [f"{hx(long_seed)} {j} 4096" for j in range(2)]
    lines += [f"{hx(MANY_TRIES_SEED)} 2 29", f"{hx(MANY_TRIES_SEED)} 2 30", f"{hx(MANY_TRIES_SEED)} 0 0"]        # the retry bound, lowered
    f = tmp_path / "key.txt"
    f.write_text("\n".join(lines) + "\n")
    got = check("key", f).split("\n")
    want = [f"{u} {k.hex()}" for u, k in zip(used, key)] + [f"{u} {k.hex()}" for u, k in zip(M.derive_key(be, b"", 2, with_tries=True)[1], key2)]
    want += [f"{u} {k.hex()}" for u, k in zip(M.derive_key(be, long_seed, 1, with_tries=True)[1], key3)]
    want += [f"0 {bytes(32).hex()}", f"30 {key[2].hex()}", f"0 {bytes(32).hex()}"]
    assert got[:len(want)] == want


def test_hash_lanes(check, tmp_path):
    rng = random.Random(5)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    lines, want = [], []
    for _ in range(4):
        a, b, c, h = rb(64), rb(64), rb(32), rb(32)
        lines.append(f"1 {a.hex()} {b.hex()} {c.hex()} {h.hex()}")
        want.append(M.H32(b"\x00" + a + b + c + h).hex())
        lines.append(f"2 {c.hex()} {h.hex()}")
        want.append(M.H32(b"\x00" + c + h).hex())
    for plen, n in ((0, 1), (1, 2), (18, 65), (110, 1 << 20), (111, 3), (255, (1 << 23))):
        p, Kb, h0, r1 = rb(plen), rb(32), rb(32), rb(32)
        lines.append(f"seed {hx(p)} {n} {Kb.hex()} {h0.hex()} {r1.hex()}")
        want.append(hashlib.sha512(b"eg-shuffle-v1/seed" + bytes([plen]) + p + M.le64(n) + Kb + h0 + r1).hexdigest())
    for i in (0, 1, 255, 256, (1 << 23) - 1, (1 << 40) + 5):
        s = rb(64)
        lines.append(f"u {s.hex()} {i}")
        want.append(M.sc(M.wide(b"eg-shuffle-v1/u" + s + M.le64(i))).hex())
        r2, head = rb(32), rb(160)
        lines.append(f"x {s.hex()} {r2.hex()} {head.hex()}")
        want.append(M.sc(M.wide(b"eg-shuffle-v1/c" + s + r2 + head)).hex())
    f = tmp_path / "hash.txt"
    f.write_text("\n".join(lines) + "\n")
    assert check("hash", f).split("\n")[:len(want)] == want


def run_verify(check, tmp_path, t, tag=""):
    n = len(t["ins"])
    f = tmp_path / f"verify{tag}.txt"
    f.write_text(f"{n} {hx(t['prefix'])} {t['K'].hex()}\n{b''.join(t['key'][:n + 1]).hex()}\n{b''.join(t['ins']).hex()}\n{b''.join(t['outs']).hex()}\n"
                 f"{t['proof'].hex()}\n")
    out = check("verify", f).split("\n")
    head = list(map(int, out[0].split()))
    return head[0], list(map(int, out[1].split())), head[1:]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_the_whole_pass_lane_by_lane(check, be, K, key, tmp_path, n):
    """accepted shuffles, EVERY tampered twin and the lying provers through the lanes in the kernels' arrangement: mask, rows and found are
    the model's, word for word.  At the tile's edge (63, 64, 65) a wrong t^ with its own challenge is also put at rows 0, 62 and the last,
    and a bad chain element at row 62, whose successor is the first row of the next tile.  A run of the program under the sanitizers takes
    seconds at these sizes, so the twins of a size run as processes side by side."""
    c = case_of(be, K, key, n)
    twins = [SC.base(c, K, key)] + SC.tampered(c, K, key) + SC.lying(be, c, K, key, 5000 + n)
    if n > 2:
        twins += [dict(SC.base(c, K, key), name=f"that_flip_{k}",
                       proof=M.prove(be, c["ins"], c["outs"], K, key, SC.PREFIX, c["src"], c["rho"], random.Random(6000 + k), that_flip=k))
                  for k in sorted({0, 62, n - 1})]
        twins.append(dict(SC.base(c, K, key), name="chat_62_not_a_point", proof=SC.put(c["proof"], n, "chat", 62, SC.NOT_A_POINT)))
    want = [SC.judge(be, t) for t in twins]
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        got = list(pool.map(lambda kt: run_verify(check, tmp_path, kt[1], kt[0]), enumerate(twins)))
    for t, g, w in zip(twins, got, want):
        assert g == w, (n, t["name"])
    assert got[0] == (0, [0] * n, NONE4)
    by = {t["name"]: g for t, g in zip(twins, got)}
    last = n - 1
    assert by["chat_last_not_a_point"][1][last] & M.ROW_BAD and by["shat_is_l"][1][last] & M.ROW_BAD
    if n > 63:                                                            # row 62 is bad; row 63, in the next tile, has no predecessor to evaluate against
        assert by["chat_62_not_a_point"][1][62] & M.ROW_BAD and by["chat_62_not_a_point"][1][63] == 0


@pytest.mark.parametrize("name,value", sorted(SC.SCALARS.items()))
def test_chain_lane_scalar_corners(check, be, K, key, tmp_path, name, value):
    """s^ and s' in {0, 1, l - 1, l, 2^256 - 1}: the rows at fault are flagged, canonical ones fail CHAIN, nothing faults"""
    n = 3
    c = case_of(be, K, key, n)
    raw = value.to_bytes(32, "little")
    for sec in ("shat", "sprime"):
        t = dict(SC.base(c, K, key), name=f"{sec}_{name}", proof=SC.put(c["proof"], n, sec, 1, raw))
        want = SC.judge(be, t)
        assert run_verify(check, tmp_path, t) == want
        assert want[1][1] == (M.ROW_BAD if value >= M.L else M.ROW_CHAIN)


def test_layout_and_refusals(check):
    for n, cus, tree, big, small in ((1, 256, 0, 0, 0), (63, 256, 0, 1024, 0), (1025, 4, 2048, 999_999, 512), (100_000, 256, 4096, 3_000_000, 0)):
        total, grid = map(int, check("layout", n, cus, tree, big, small).split("\n")[0].split())
        up = lambda b: (b + 255) // 256 * 256
        tiles = -(-n // 63)
        want_grid = min(-(-tiles * 64 // 256), cus * 4)
        parts = [256, 512, 32 * n, n, tree, 32 * -(-n // 256), 256 * n, 256 * n, 128, 128, 4, 128, 128, 64, 64, 2, want_grid * 256 * 2 * 1152, max(big, small)]
        assert (total, grid) == (sum(up(p) for p in parts), want_grid)
    ok = [5, 5, 1, 1, 1, 1, 3, 1, 1, 1, 1]
    assert check("refuse", *ok).startswith("ok")
    for at, value, word in ((0, (1 << 23) + 1, "N is above"), (1, (1 << 23) + 1, "key_cap"), (1, 4, "N > key_cap"), (6, 256, "255"), (5, 0, "null prefix"),
                            (9, 0, "verdict"), (10, 0, "found"), (2, 0, "null in"), (3, 0, "null in"), (4, 0, "null in"), (7, 0, "null in"), (8, 0, "null in")):
        args = list(ok)
        args[at] = value
        assert word in check("refuse", *args), (at, value)
    assert check("refuse", 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1).startswith("ok")             # nothing to verify: only the outputs are needed


# ------------------------------------------------------------------ the entries without a GPU
@pytest.fixture(scope="module")
def lib():
    import elastic_elgamal_amd as eg

    return eg._load()


def test_sizes(lib):
    top = 1 << 23
    assert [lib.eg_shuffle_proof_bytes(n) for n in (0, 1, 2, top, top + 1)] == [288, 448, 608, 288 + 160 * top, 0]
    assert [lib.eg_shuffle_key_bytes(n) for n in (0, 1, top, top + 1)] == [32, 64, 32 * (top + 1), 0]
    assert lib.eg_shuffle_verify_scratch_bytes(None, 5) == 0
    assert M.proof_bytes(7) == lib.eg_shuffle_proof_bytes(7)


def test_every_refusal_comes_before_the_context(lib):
    import elastic_elgamal_amd as eg

    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    v, f = C.c_uint32(), (C.c_uint32 * 4)()
    B = C.create_string_buffer(32)

    def dev(n=5, d_in=p, d_out=p, K=B, prefix=b"ab", plen=2, d_key=p, cap=5, d_proof=p, d_v=p, d_rows=p, d_f=p, d_s=p, sb=1 << 40):
        return lib.eg_shuffle_verify_device(None, n, d_in, d_out, K, prefix, plen, d_key, cap, d_proof, d_v, d_rows, d_f, d_s, sb, None)

    def host(n=5, a=buf, b=buf, K=B, prefix=b"ab", plen=2, key=buf, cap=5, proof=buf, vv=C.byref(v), rows=None, ff=f):
        return lib.eg_shuffle_verify(None, n, a, b, K, prefix, plen, key, cap, proof, vv, rows, ff)

    def refused(rc, word):
        assert rc == -3 and word in lib.eg_last_error().decode(), lib.eg_last_error()

    refused(dev(), "null ctx")                                         # everything else is fine: only the context is missing
    refused(host(), "null ctx")
    for fn in (dev, host):
        refused(fn(n=(1 << 23) + 1, cap=(1 << 23) + 1), "N is above")
        refused(fn(cap=(1 << 23) + 1), "key_cap")
        refused(fn(n=6), "N > key_cap")
        refused(fn(plen=256), "255")
        refused(fn(prefix=None), "null prefix")
        refused(fn(K=None), "null in")
    for kw in ("d_in", "d_out", "d_key", "d_proof"):
        refused(dev(**{kw: None}), "null in")
        refused(dev(**{kw: p + 2}), "4-byte aligned")
    for kw in ("a", "b", "key", "proof"):
        refused(host(**{kw: None}), "null in")
    refused(dev(d_v=None), "verdict")
    refused(dev(d_f=None), "found")
    refused(host(vv=None), "verdict")
    refused(host(ff=None), "found")
    for kw in ("d_v", "d_rows", "d_f"):
        refused(dev(**{kw: p + 1}), "4-byte aligned")
    refused(dev(d_s=p + 8), "16-byte aligned")
    refused(dev(n=0, d_in=None, d_out=None, d_key=None, d_proof=None, K=None, prefix=None, plen=0, cap=0, d_s=None, sb=0), "null ctx")   # N == 0 passes the rules
    # the key entries
    e = C.c_uint32()
    refused(lib.eg_shuffle_key_derive(None, b"s", 1, (1 << 23) + 1, buf), "cap is above")
    refused(lib.eg_shuffle_key_derive(None, b"s", 256, 3, buf), "255")
    refused(lib.eg_shuffle_key_derive(None, None, 1, 3, buf), "null seed")
    refused(lib.eg_shuffle_key_derive(None, b"s", 1, 3, None), "null key")
    refused(lib.eg_shuffle_key_derive(None, b"s", 1, 3, buf), "null ctx")
    refused(lib.eg_shuffle_key_derive_device(None, b"s", 1, 3, p, None, None), "exhausted")
    refused(lib.eg_shuffle_key_derive_device(None, b"s", 1, 3, p + 1, C.addressof(e), None), "4-byte aligned")
    refused(lib.eg_shuffle_key_derive_device(None, b"s", 1, 3, p, C.addressof(e), None), "null ctx")
    with pytest.raises(eg.EgError):
        eg.ShuffleVerifier.derive_key(type("X", (), {"_h": None})(), b"s", 3)


def test_symbols_bindings_and_mirrors(lib, tmp_path):
    import elastic_elgamal_amd as eg

    names = ["eg_shuffle_key_bytes", "eg_shuffle_proof_bytes", "eg_shuffle_key_derive_device", "eg_shuffle_key_derive", "eg_shuffle_verify_scratch_bytes",
             "eg_shuffle_verify_device", "eg_shuffle_verify"]
    assert set(names) <= set(eg.exported_symbols())
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    for n in names:
        assert getattr(lib, n).argtypes is not None and n + "(" in hpp, n
    assert (eg.SHUFFLE_BAD_ENCODING, eg.SHUFFLE_T1, eg.SHUFFLE_T2, eg.SHUFFLE_T3, eg.SHUFFLE_T41, eg.SHUFFLE_T42, eg.SHUFFLE_CHAIN) == \
        (M.BAD_ENCODING, M.T1, M.T2, M.T3, M.T41, M.T42, M.CHAIN) == (1, 2, 4, 8, 16, 32, 64)
    assert (eg.SHUFFLE_ROWS_MAX, eg.SHUFFLE_KEY_TRIES, eg.ABI_VERSION) == (M.ROWS_MAX, M.KEY_TRIES, 7)
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_SHUFFLE_BAD_ENCODING == 1 && EG_SHUFFLE_CHAIN == 64 && EG_SHUFFLE_ROW_CHAIN == 2 && '
                   'EG_SHUFFLE_ROWS_MAX == 8388608u && EG_SHUFFLE_KEY_TRIES == 4096 && EG_ABI_VERSION == 7 && eg_shuffle_verify_device && '
                   'eg_shuffle_verify && eg_shuffle_key_derive && eg_shuffle_proof_bytes(1) == 448 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "mirror.cpp"
    cpp.write_text('#include "elastic_elgamal_hip.hpp"\nusing namespace elastic_elgamal_hip;\n'
                   'int main() { ShuffleVerdict v; return v.accepted() && ShuffleVerifier::proof_bytes(2) == 608 && ShuffleVerifier::key_bytes(1) == 64 ? 0 : 1; }\n')
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(cpp), f"-L{ROOT / 'elastic_elgamal_amd'}",
                           "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0
