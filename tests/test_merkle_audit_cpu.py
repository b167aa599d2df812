"""The receipt log's audit entries (eg_merkle_heads / _consistency / _consistency_check, eg_merkle_consistency_len) without a GPU:
* the surface: the symbols declared, exported, bound, mirrored and in INTEGRATION.md; EG_MERKLE_MISMATCH_OLD in the header, the Python
  mirror, merkle_audit_host.hpp and the model; the C++ mirror compiles and instantiates the new methods; plain C99; no environment knob
  and no waiting loop in the device code;
* self-checks of the model tests/merkle_audit_ref.py (written from the text of RFC 9162 2.1.4 with hashlib);
* tests/hostcheck/merkleauditcheck.cpp: merkle_audit_host.hpp and the lane functions of merkle_audit_kernels.cuh under ASan + UBSan, run
  serially for every N = 0 .. 70: heads, proofs and checks, every verdict count against the model's;
* eg_merkle_consistency_len against the model, and every refusal that needs no GPU."""
import ctypes as C
import random
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import merkle_audit_ref as A
import merkle_ref as M

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
BAD_ARG = -3
NMAX = 70
ENTRIES = {  # name: (return type in the header, restype, number of arguments)
    "eg_merkle_consistency_len": ("uint32_t", C.c_uint32, 2),
    "eg_merkle_heads_device": ("int", C.c_int, 9),
    "eg_merkle_heads": ("int", C.c_int, 8),
    "eg_merkle_consistency_device": ("int", C.c_int, 9),
    "eg_merkle_consistency": ("int", C.c_int, 8),
    "eg_merkle_consistency_check_device": ("int", C.c_int, 12),
    "eg_merkle_consistency_check": ("int", C.c_int, 11),
}


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
    # inside the receipt-log section, behind eg_merkle_check and in front of the multi-GPU tier; no section line of their own
    section, nxt = header.index("/* ---- receipt log"), header.index("/* ---- batch tier on several GPUs")
    for name in ENTRIES:
        assert section < header.index("int eg_merkle_check(") < header.index(f" {name}(uint64_t" if name.endswith("_len") else f"int {name}(") < nxt, name
    assert header[section:nxt].count("/* ---- ") == 1
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("int eg_merkle_check("):nxt])
    for phrase in ("PAST HEAD", "CONSISTENCY PROOF", "RFC 9162 2.1.4.1", "RFC 9162 2.1.4.2", "THE SEED", "fold it on the left", "no proof byte is read",
                   "the first failure in this order wins", "(3, 6) -> 4", "take no lock", "never synchronise", "variable time"):
        assert phrase in text, phrase
    for m in ("heads", "consistency", "consistency_check", "heads_device", "consistency_device", "consistency_check_device", "consistency_len"):
        assert callable(getattr(eg.ReceiptLog, m)), m
    ffi = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name
    assert "pub fn eg_merkle_consistency_len(old_size: u64, n_leaves: u64) -> u32;" in ffi
    for doc, words in (("README.md", ("merkle_audit_kernels.cuh", "test_gpu_merkle_audit.py", "r20_log_audit.txt", "first measurement")),
                       ("DESIGN.md", ("consistency proof", "k_merkle_cons_check", "past head")), ("INTEGRATION.md", ("consistency proof",))):
        text = (ROOT / doc).read_text()
        for w in words:
            assert w in text, (doc, w)


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    host = (CSRC / "merkle_audit_host.hpp").read_text()
    value = int(re.search(r"EG_MERKLE_MISMATCH_OLD = (\d+)", header).group(1))
    assert value == eg.MERKLE_MISMATCH_OLD == eg.ReceiptLog.MISMATCH_OLD == A.MISMATCH_OLD == 4
    assert re.search(rf"\bMERKLE_MISMATCH_OLD = {value};", host)
    assert (A.BAD_INDEX, A.BAD_LENGTH, A.MISMATCH) == (eg.MERKLE_BAD_INDEX, eg.MERKLE_BAD_LENGTH, eg.MERKLE_MISMATCH) == (1, 2, 3)
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert max(eg.STATUS_NAMES) == 16                                   # no status word is added


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
            ReceiptLog rl{ctx, {1, 2, 3}};
            Bytes log(6 * 32);
            MerkleTree t = rl.tree(log);
            PastHeads h = rl.heads({0, 3, 6, 7}, log, t.nodes);
            ConsistencyProofs p = rl.consistency({3, 6}, log, t.nodes);
            Bytes old(h.heads.begin() + 32, h.heads.begin() + 96);
            ConsistencyVerdicts v = rl.consistency_check({3, 6}, old, p.proofs, 32 * ((size_t)ReceiptLog::depth(6) + 1), p.proof_len, 6, t.root);
            rl.heads_device(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
            rl.consistency_device(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
            rl.consistency_check_device(0, nullptr, nullptr, nullptr, 32, nullptr, 0, nullptr, nullptr, nullptr);
            return (int)(h.found[0] + v.found[3] + v.verdict.size() + p.proof_len.size());
          }
          static_assert(EG_MERKLE_MISMATCH_OLD == 4 && EG_MERKLE_MISMATCH == 3, "header constants");
          return eg_merkle_consistency_len(3, 6) == 4 && ReceiptLog::consistency_len(6, 6) == 0 && eg_merkle_consistency_len(7, 6) == EG_MERKLE_NO_PATH ? 0 : 1;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    names = " && ".join(ENTRIES)
    src.write_text(f'#include "eg_hip.h"\nint main(void) {{ return EG_MERKLE_MISMATCH_OLD == 4 && {names} ? 0 : 1; }}\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-address", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_no_waiting_between_lanes():
    for f in ("merkle_audit_kernels.cuh", "merkle_audit_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    host = (CSRC / "merkle_audit_host.hpp").read_text()
    assert "#include <hip" not in host and "__global__" not in host and '#include "merkle_host.hpp"' in host        # pure host code
    for name in ("consistency_len", "refuse_heads", "refuse_consistency", "refuse_consistency_check"):
        assert re.search(rf"\b{name}\(", host), name
    kernels = (CSRC / "merkle_audit_kernels.cuh").read_text()
    # bounded for loops only, no fences, no compare-and-swap; the lanes share nothing but the wave tally
    assert not re.search(r"\bwhile\b", kernels) and "__threadfence" not in kernels and "__builtin_amdgcn_fence" not in kernels
    assert "atomic" not in kernels.replace("wave-level atomic", "") and "__syncthreads" not in kernels and "__shared__" not in kernels
    for name in ("k_merkle_heads", "k_merkle_consistency", "k_merkle_cons_check"):
        assert re.search(rf"__global__ void __launch_bounds__\(MERKLE_NT\) {name}\(", kernels), name
    assert kernels.count("merkle_wave_tally(") == 5 and "merkle_empty_root(" in kernels and "merkle_ld8(" in kernels and "merkle_st8(" in kernels
    assert '#include "merkle_audit_kernels.cuh"' in (CSRC / "eg_hip.hip").read_text()


# ------------------------------------------------------------------ the model checks itself
def _leaves(n, seed=1):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(n)]


def test_model_every_proof_proves_and_the_forms_agree():
    """every 1 <= m <= N <= 130: the recursion of the RFC equals the store form, the length the closed form, the fold the prefix's MTH;
    truncated and lengthened proofs fail; a flipped bit anywhere fails with the right one of the two mismatch verdicts"""
    assert A.self_check(_leaves(130), 130) == 130 * 131 // 2
    assert A.consistency_len(3, 6) == 4 == M.depth(6) + 1 and A.consistency_len(6, 6) == 0 and A.consistency_len(4, 6) == 1
    # the proofs of RFC 6962 2.1.3's example tree of seven leaves
    d = _leaves(7, seed=2)
    lv = M.levels(d)
    c, dd, g, h, i, j, k, ll = lv[0][2], lv[0][3], lv[1][0], lv[1][1], lv[1][2], lv[0][6], lv[2][0], lv[2][1]
    assert A.proof(3, d) == [c, dd, g, ll] and A.proof(4, d) == [ll] and A.proof(6, d) == [i, j, k]
    assert dd == d[3] and h == M.node_hash(c, dd)


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "merkleauditcheck", HERE / "merkleauditcheck.cpp"
    deps = [src, CSRC / "merkle_audit_kernels.cuh", CSRC / "merkle_audit_host.hpp", CSRC / "merkle_kernels.cuh", CSRC / "merkle_host.hpp", CSRC / "sha512.cuh",
            CSRC / "fe25519.cuh"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout

    return run


def test_heads_proofs_and_checks_of_every_size(check, tmp_path):
    leaves = _leaves(NMAX, seed=7)
    path = tmp_path / "leaves.txt"
    path.write_text("\n".join(x.hex() for x in leaves) + "\n")
    out = check("audit", path)
    head = {}
    for n in range(NMAX + 1):
        head[n] = M.mth(leaves[:n])
    rows = [line.split(" ") for line in out.splitlines() if line.startswith("HEAD")]
    assert len(rows) == sum(n + 2 for n in range(NMAX + 1))
    for _, n, s, h in rows:
        n, s = int(n), int(s)
        assert h == (head[s].hex() if s <= n else "00" * 32), (n, s)      # every past head is MTH of the prefix; a size above N: zeroed
    rows = [line.split(" ") for line in out.splitlines() if line.startswith("PROOF")]
    assert len(rows) == sum(n + 2 for n in range(NMAX + 1))
    want = [0, 0, 0, 0, 0]                                                # by verdict
    proofs = {}
    for _, n, m, length, row in rows:
        n, m, length = int(n), int(m), int(length)
        d = M.depth(n)
        if m == 0 or m > n:
            assert length == A.NO_PATH and row == "00" * 32 * (d + 1), (n, m)
            want[A.BAD_INDEX] += 4
            continue
        p = proofs[m, n] = A.proof(m, leaves[:n])                          # the recursion of the RFC
        assert length == len(p) and row == (b"".join(p) + bytes(32 * (d + 1 - length))).hex(), (n, m)
        want[A.check(m, n, head[m], p, head[n])] += 1                     # honest
        want[A.BAD_LENGTH] += d + 4                                        # every proof_len of 0 .. depth + 3 but the right one, and NO_PATH
        for k in range(len(p)):
            want[A.check(m, n, head[m], p[:k] + [A.flip(p[k], 9)] + p[k + 1:], head[n])] += 1
        want[A.check(m, n, A.flip(head[m], 3), p, head[n])] += 1
        want[A.check(m, n, head[m], p, A.flip(head[n], 77))] += 1
        if m < n:
            want[A.check(m, n, head[m], proofs[m, n - 1], head[n])] += 1   # the proof of (m, N - 1) offered at N
    got = list(map(int, re.search(r"VERDICTS (\d+) (\d+) (\d+) (\d+) (\d+)", out).groups()))
    assert got == want and want[0] == NMAX * (NMAX + 1) // 2 and want[A.BAD_INDEX] == 4 * 2 * (NMAX + 1) and want[A.MISMATCH_OLD] > 1000


# ------------------------------------------------------------------ the pure host function of the library
def test_consistency_len_against_the_model(check):
    lib = eg._load()
    for n in range(0, 71):
        for m in range(0, n + 3):
            assert lib.eg_merkle_consistency_len(m, n) == A.consistency_len(m, n) == eg.ReceiptLog.consistency_len(m, n), (m, n)
    for n in range(1, 71):
        d = _leaves(n, seed=4)
        assert [lib.eg_merkle_consistency_len(m, n) for m in range(1, n + 1)] == [len(A.proof(m, d)) for m in range(1, n + 1)], n
    sizes = [(1 << 10) + d for d in (-1, 0, 1)] + [(1 << 20) + d for d in (-1, 0, 1, 3)] + [(1 << 31) - 2, (1 << 31) - 1]
    olds = [1, 2, 3, 511, 512, 513, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 2]
    for n in sizes:
        for m in olds + [n - 1, n, n + 1, 0, 1 << 40]:
            got = lib.eg_merkle_consistency_len(m, n)
            assert got == A.consistency_len(m, n), (m, n)
            assert got == A.NO_PATH or got <= M.depth(n) + 1
    assert lib.eg_merkle_consistency_len(3, 6) == 4 and "LEN 4\n" in check("len", 3, 6)


# ------------------------------------------------------------------ refusals of the library that need no GPU
def test_refusals_of_the_six_entries_without_a_gpu():
    """the argument rules come before the context is looked at; what passes them fails on the missing context"""
    lib = eg._load()
    buf = C.create_string_buffer(1 << 12)
    base = (C.addressof(buf) + 15) & ~15
    P = C.c_void_p
    big = 1 << 31

    def err():
        return lib.eg_last_error()

    def chars(p):
        return C.cast(P(p), C.c_char_p)

    # heads
    def heads_dev(m=1, size=base, n=5, log=base, nodes=base, heads=base, found=base):
        return lib.eg_merkle_heads_device(None, m, P(size), n, P(log), P(nodes), P(heads), P(found), None)

    def heads_host(m=1, size=base, n=5, log=base, nodes=base, heads=base, found=base):
        return lib.eg_merkle_heads(None, m, P(size), n, chars(log), chars(nodes), P(heads), P(found))

    for call in (heads_dev, heads_host):
        for kw, text in (({"m": big}, b"m is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"), ({"size": None}, b"null size, heads or found"),
                         ({"heads": None}, b"null size, heads or found"), ({"found": None}, b"null size, heads or found"),
                         ({"log": None}, b"null log or nodes"), ({"nodes": None}, b"null log or nodes"), ({"n": 1, "log": None}, b"null log or nodes")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in ({}, {"m": 0, "size": None, "log": None, "nodes": None, "heads": None, "found": None}, {"n": 1, "nodes": None},
                   {"n": 0, "log": None, "nodes": None}, {"m": big - 1, "n": big - 1}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    assert heads_dev(size=base + 4) == BAD_ARG and b"8-byte aligned" in err()
    for name in ("log", "nodes", "heads", "found"):
        assert heads_dev(**{name: base + 2}) == BAD_ARG and b"4-byte aligned" in err(), name

    # consistency
    def cons_dev(m=1, old=base, n=5, log=base, nodes=base, proofs=base, plen=base):
        return lib.eg_merkle_consistency_device(None, m, P(old), n, P(log), P(nodes), P(proofs), P(plen), None)

    def cons_host(m=1, old=base, n=5, log=base, nodes=base, proofs=base, plen=base):
        return lib.eg_merkle_consistency(None, m, P(old), n, chars(log), chars(nodes), P(proofs), P(plen))

    for call in (cons_dev, cons_host):
        for kw, text in (({"m": big}, b"m is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"), ({"old": None}, b"null old_size, proofs or proof_len"),
                         ({"proofs": None}, b"null old_size, proofs or proof_len"), ({"plen": None}, b"null old_size, proofs or proof_len"),
                         ({"n": 1, "proofs": None}, b"null old_size, proofs or proof_len"), ({"log": None}, b"null log or nodes"),
                         ({"nodes": None}, b"null log or nodes"), ({"n": 1, "log": None}, b"null log or nodes")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in ({}, {"m": 0, "old": None, "log": None, "nodes": None, "proofs": None, "plen": None}, {"n": 1, "nodes": None},
                   {"n": 0, "log": None, "nodes": None}, {"m": big - 1, "n": big - 1}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    assert cons_dev(old=base + 4) == BAD_ARG and b"8-byte aligned" in err()
    for name in ("log", "nodes", "proofs", "plen"):
        assert cons_dev(**{name: base + 2}) == BAD_ARG and b"4-byte aligned" in err(), name

    # the check: depth(5) = 3, a row of four entries
    def check_dev(m=1, old=base, oroot=base, proofs=base, stride=128, plen=base, n=5, root=base, verdict=base, found=base):
        return lib.eg_merkle_consistency_check_device(None, m, P(old), P(oroot), P(proofs), stride, P(plen), n, P(root), P(verdict), P(found), None)

    def check_host(m=1, old=base, oroot=base, proofs=base, stride=128, plen=base, n=5, root=base, verdict=base, found=base):
        return lib.eg_merkle_consistency_check(None, m, P(old), chars(oroot), chars(proofs), stride, P(plen), n, chars(root), P(verdict), P(found))

    for call in (check_dev, check_host):
        for kw, text in (({"m": big}, b"m is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"), ({"stride": 127}, b"proof_stride is below 32 * (depth(N) + 1)"),
                         ({"stride": 96}, b"proof_stride is below 32 * (depth(N) + 1)"), ({"n": 1025, "stride": 352}, b"proof_stride is below 32 * (depth(N) + 1)"),
                         ({"n": 1, "stride": 0}, b"proof_stride is below 32 * (depth(N) + 1)"), ({"stride": 130}, b"proof_stride is no multiple of 4"),
                         ({"proofs": None}, b"null proofs")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for name in ("old", "oroot", "plen", "root", "verdict", "found"):
            assert call(**{name: None}) == BAD_ARG and b"null old_size, old_root, proof_len, root, verdict or found" in err(), (call.__name__, name)
        for kw in ({}, {"stride": 160}, {"n": 1025, "stride": 384}, {"n": 1, "stride": 32, "proofs": None}, {"n": 0, "stride": 32, "proofs": None},
                   {"m": 0, "old": None, "oroot": None, "proofs": None, "plen": None, "root": None, "verdict": None, "found": None}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    assert check_dev(old=base + 4) == BAD_ARG and b"8-byte aligned" in err()
    for name in ("oroot", "proofs", "plen", "root", "verdict", "found"):
        assert check_dev(**{name: base + 2}) == BAD_ARG and b"4-byte aligned" in err(), name


def test_missing_gpu_is_loud():
    log = object.__new__(eg.ReceiptLog)
    log.ctx, log.prefix = type("NoCtx", (), {"_h": None})(), b"election"
    with pytest.raises(eg.EgError, match="null ctx"):
        log.heads([0, 2, 3], bytes(96), bytes(96))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.consistency([1, 2, 3], bytes(96), bytes(96))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.consistency_check([1, 2], [bytes(32), bytes(32)], [bytes(64), bytes(32)], 3, bytes(32))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.consistency_check([2], bytes(32), bytes(96), 3, bytes(32), proof_len=[2], proof_stride=96)
    with pytest.raises(eg.EgError, match="proof_stride is below"):
        log.consistency_check([2], bytes(32), bytes(64), 3, bytes(32), proof_len=[2], proof_stride=64)
