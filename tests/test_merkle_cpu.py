"""The receipt log (eg_merkle_*) without a GPU:
* the surface: the symbols declared, exported, bound, mirrored and in INTEGRATION.md; the constants in the header, the Python mirror,
  merkle_host.hpp and the model; ABI version 7; the header's section order; the C++ mirror; plain C99; no environment knob and no waiting
  loop in the device code;
* self-checks of the model tests/merkle_ref.py (written from the RFC text with hashlib), from which every expected value comes;
* tests/hostcheck/merklecheck.cpp: merkle_host.hpp and the lane functions of merkle_kernels.cuh under ASan + UBSan, run serially: the
  node hash, trees with tiles of 4 and 8 for every N = 0 .. 70, paths and checks for every (i, N), the leaf pass around the block seams;
* eg_merkle_depth / _level / _nodes_bytes against a direct count, and every refusal that needs no GPU."""
import ctypes as C
import hashlib
import random
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import merkle_ref as M

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
BAD_ARG = -3
NMAX = 70
ENTRIES = {  # name: (return type in the header, restype, number of arguments)
    "eg_merkle_depth": ("int", C.c_int, 1),
    "eg_merkle_nodes_bytes": ("size_t", C.c_size_t, 1),
    "eg_merkle_level": ("int", C.c_int, 4),
    "eg_merkle_leaves_scratch_bytes": ("size_t", C.c_size_t, 1),
    "eg_merkle_tree_scratch_bytes": ("size_t", C.c_size_t, 1),
    "eg_merkle_leaves_device": ("int", C.c_int, 21),
    "eg_merkle_leaves": ("int", C.c_int, 18),
    "eg_merkle_tree_device": ("int", C.c_int, 8),
    "eg_merkle_tree": ("int", C.c_int, 5),
    "eg_merkle_paths_device": ("int", C.c_int, 9),
    "eg_merkle_paths": ("int", C.c_int, 8),
    "eg_merkle_check_device": ("int", C.c_int, 12),
    "eg_merkle_check": ("int", C.c_int, 11),
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
    # a section of its own, behind the voter roll and in front of the multi-GPU tier
    at = header.index("int eg_merkle_depth(uint64_t")
    section = header.index("/* ---- receipt log")
    assert header.index("int eg_roll_check(") < section < at < header.index("/* ---- batch tier on several GPUs") < header.index("int eg_verify_choice_batch_multi(")
    sections = [m.start() for m in re.finditer(r"^/\* ---- ", header, re.M)]
    order = [header[s:s + 60] for s in sections]
    names = ("ballot weeding", "voter signatures", "voter roll", "receipt log", "batch tier on several GPUs")
    found = [next(k for k, text in enumerate(order) if name in text) for name in names]
    assert found == sorted(found) and found[3] == found[2] + 1 and found[4] == found[3] + 1, found
    for phrase in ("THE RULE", "ORDER IN THE CHAIN", "signatures -> verify -> weed -> LEAVES -> roll -> tally", "TIMING: variable time", "FULL REBUILD",
                   "no incremental frontier state", "RFC 6962 2.1", "RFC 9162 2.1.3.2", "the first 32 bytes of SHA-512", "promoted unchanged",
                   "no path byte is read", "take no lock", "never synchronise", "MULTI-GPU"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header[section:at]), phrase
    for m in ("leaves", "tree", "paths", "check", "leaves_device", "tree_device", "paths_device", "check_device", "depth", "level", "nodes_bytes"):
        assert callable(getattr(eg.ReceiptLog, m)), m
    assert "ReceiptLog" in eg.__all__
    ffi = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name
    for doc, words in (("README.md", ("Receipt log", "merkle_kernels.cuh", "test_gpu_merkle.py")), ("DESIGN.md", ("receipt log", "status_out", "superseded")),
                       ("INTEGRATION.md", ("receipt",))):
        text = (ROOT / doc).read_text()
        for w in words:
            assert w in text, (doc, w)


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    host = (CSRC / "merkle_host.hpp").read_text()
    for name, model in (("BAD_INDEX", M.BAD_INDEX), ("BAD_LENGTH", M.BAD_LENGTH), ("MISMATCH", M.MISMATCH)):
        value = int(re.search(rf"EG_MERKLE_{name} = (\d+)", header).group(1))
        assert value == getattr(eg, "MERKLE_" + name) == getattr(eg.ReceiptLog, name) == model, name
        assert re.search(rf"\bMERKLE_{name} = {value};", host), name
    assert (M.BAD_INDEX, M.BAD_LENGTH, M.MISMATCH) == (1, 2, 3)
    assert re.search(r"#define EG_LEAF_NONE \(~\(uint64_t\)0\)", header) and eg.LEAF_NONE == eg.ReceiptLog.LEAF_NONE == M.LEAF_NONE == (1 << 64) - 1
    assert "LEAF_NONE = ~0ull;" in host
    assert re.search(r"#define EG_MERKLE_LEAVES_MAX \(1u << 31\)", header) and eg.MERKLE_LEAVES_MAX == eg.ReceiptLog.LEAVES_MAX == M.LEAVES_MAX == 1 << 31
    assert "LEAVES_MAX = 1ull << 31;" in host
    assert re.search(r"#define EG_MERKLE_NO_PATH 0xffffffffu", header) and eg.MERKLE_NO_PATH == eg.ReceiptLog.NO_PATH == M.NO_PATH == 0xFFFFFFFF
    assert re.search(r"#define EG_MERKLE_HASH_BYTES 32", header) and eg.MERKLE_HASH_BYTES == eg.ReceiptLog.HASH_BYTES == 32 and "HASH_BYTES = 32;" in host
    assert int(re.search(r"T_LOG = (\d+);", host).group(1)) == 10
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7
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
            Bytes log, msgs(3 * 40), sigs(3 * 64);
            LeafPass a = rl.leaves(msgs, 40, 3, sigs, {0, 5, 0}, &log);
            MerkleTree t = rl.tree(log);
            Receipts r = rl.paths({0, 1, 7}, log, t.nodes);
            ReceiptVerdicts v = rl.check({0, 1}, log, r.paths, 32 * (size_t)ReceiptLog::depth(2), {1, 1}, 2, t.root);
            rl.leaves_device(0, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                             ReceiptLog::leaves_scratch_bytes(0));
            rl.tree_device(0, nullptr, nullptr, nullptr, nullptr, ReceiptLog::tree_scratch_bytes(0));
            rl.paths_device(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
            rl.check_device(0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr);
            return (int)(a.found[0] + v.found[2] + r.path_len.size() + ReceiptLog::level(5, 1).second + ReceiptLog::nodes_bytes(5));
          }
          static_assert(EG_MERKLE_BAD_INDEX == 1 && EG_MERKLE_BAD_LENGTH == 2 && EG_MERKLE_MISMATCH == 3 && EG_MERKLE_HASH_BYTES == 32 &&
                        EG_LEAF_NONE == 0xffffffffffffffffull && EG_MERKLE_LEAVES_MAX == (1u << 31) && EG_MERKLE_NO_PATH == 0xffffffffu,
                        "header constants");
          return eg_merkle_depth(5) == 3 && eg_merkle_nodes_bytes(5) == 32 * 6 ? 0 : 1;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    names = " && ".join(ENTRIES)
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_MERKLE_MISMATCH == 3 && EG_LEAF_NONE > EG_MERKLE_LEAVES_MAX && EG_MERKLE_NO_PATH && '
                   f'EG_MERKLE_HASH_BYTES == 32 && {names} ? 0 : 1; }}\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-address", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_no_waiting_between_lanes():
    for f in ("merkle_kernels.cuh", "merkle_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    host = (CSRC / "merkle_host.hpp").read_text()
    assert "#include <hip" not in host and "__global__" not in host and "__host__ __device__" in host          # pure host code, shared lanes
    kernels = (CSRC / "merkle_kernels.cuh").read_text()
    device = kernels[kernels.index("#if defined(__HIPCC__)"):]
    # bounded loops only, the kernel boundary is the only synchronisation between workgroups; the tree kernel has no atomics at all
    assert not re.search(r"\bwhile\b", device) and "__threadfence" not in device and "__builtin_amdgcn_fence" not in device and "atomicCAS" not in kernels
    tile = device[device.index("struct MerkleTileArgs"):device.index("__global__ void k_merkle_root")]
    assert "atomic" not in tile and "__syncthreads" in tile and "template <int TL>" in tile
    node = kernels[kernels.index("EG_HD void merkle_node"):kernels.index("// the first 32 digest bytes")]
    assert "eg_funnel" in node and "sha512_compress(s, w)" in node and "w[15] = 520" in node and "unsigned char" not in node
    assert '#include "merkle_kernels.cuh"' in (CSRC / "eg_hip.hip").read_text()


# ------------------------------------------------------------------ the model checks itself
def _leaves(n, seed=1):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(n)]


def test_model_every_receipt_proves_and_the_two_forms_agree():
    leaves = _leaves(130)
    assert M.H(b"") == hashlib.sha512(b"").digest()[:32] == M.mth([])
    assert M.mth(leaves[:1]) == leaves[0] and M.mth(leaves[:2]) == hashlib.sha512(b"\x01" + leaves[0] + leaves[1]).digest()[:32]
    assert M.leaf_hash(b"abc", b"id", b"sig") == hashlib.sha512(b"\x00idabcsig").digest()[:32]
    for n in range(0, 131):
        d = leaves[:n]
        root, lv = M.mth(d), M.levels(d)
        if n:
            assert lv[-1] == [root] and len(lv) == M.depth(n) + 1, n       # the bottom-up levels equal the recursion
        assert [len(x) for x in lv] == [M.level_count(n, k) for k in range(len(lv))]
        assert M.depth(n) == next(k for k in range(64) if (1 << k) >= n) if n > 1 else M.depth(n) == 0
        for i in range(n):
            p = M.path(i, d)
            assert len(p) == M.path_len(i, n) <= M.depth(n), (i, n)         # the closed form
            # PATH by the split is the bottom-up sibling list
            assert p == [lv[k][(i >> k) ^ 1] for k in range(M.depth(n)) if ((i >> k) ^ 1) < len(lv[k])], (i, n)
            assert M.check(i, n, d[i], p, root) == 0 == M.rfc9162_check(i, n, d[i], p, root), (i, n)
            if p:
                assert M.check(i, n, d[i], p[:-1], root) == M.BAD_LENGTH == M.rfc9162_check(i, n, d[i], p[:-1], root)      # truncated
                assert M.check(i, n, d[i], p[1:], root) == M.BAD_LENGTH
            assert M.check(i, n, d[i], p + [bytes(32)], root) == M.BAD_LENGTH == M.rfc9162_check(i, n, d[i], p + [bytes(32)], root)
        for i in (n, n + 1, 1 << 40):
            assert M.check(i, n, bytes(32), [], root) == M.BAD_INDEX
    d, root = leaves[:77], M.mth(leaves[:77])
    p = M.path(50, d)
    assert M.check(50, 77, d[51], p, root) == M.MISMATCH and M.check(50, 77, d[50], p, M.mth(leaves[:78])) == M.MISMATCH
    assert M.check(50, 77, d[50], [p[0]] + [bytes(32)] + p[2:], root) == M.MISMATCH and M.check(51, 77, d[50], p, root) == M.MISMATCH


def test_model_leaf_pass():
    msgs = [bytes([b]) * 5 for b in range(6)]
    res = M.leaves_pass(msgs, b"E", [b"x"] * 6, [0, 3, 0, 0, 9, 0], n_prior=10, log_cap=14)
    assert res["leaf_index"] == [10, M.LEAF_NONE, 11, 12, M.LEAF_NONE, 13] and res["found"] == [4, 0] and res["log_count"] == 14
    assert res["leaves_out"][1] == bytes(32) and res["leaves_out"][2] == hashlib.sha512(b"\x00E" + msgs[2] + b"x").digest()[:32]
    assert res["appended"] == [res["leaves_out"][b] for b in (0, 2, 3, 5)]
    short = M.leaves_pass(msgs, b"E", [b"x"] * 6, [0, 3, 0, 0, 9, 0], n_prior=10, log_cap=13)
    assert short["found"] == [4, 1] and short["appended"] == [] and short["log_count"] == 10 and short["leaf_index"] == res["leaf_index"]


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "merklecheck", HERE / "merklecheck.cpp"
    deps = [src, CSRC / "merkle_kernels.cuh", CSRC / "merkle_host.hpp", CSRC / "sha512.cuh", CSRC / "fe25519.cuh"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args, ok=True):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        if ok:
            assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout if ok else r

    return run


@pytest.fixture(scope="module")
def leaf_file(tmp_path_factory):
    leaves = _leaves(NMAX, seed=7)
    path = tmp_path_factory.mktemp("merkle") / "leaves.txt"
    path.write_text("\n".join(x.hex() for x in leaves) + "\n")
    return path, leaves


def test_node_hash_against_hashlib(check, tmp_path):
    rng = random.Random(3)
    pairs = [(rng.randbytes(32), rng.randbytes(32)) for _ in range(40)]
    pairs += [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32), (bytes(32), b"\xff" * 32), (b"\xff" * 32, bytes(32)), (b"\x80" + bytes(31), bytes(31) + b"\x01")]
    path = tmp_path / "nodes.txt"
    path.write_text("\n".join(a.hex() + " " + b.hex() for a, b in pairs) + "\n")
    got = [line.split()[1] for line in check("node", path).splitlines() if line.startswith("NODE")]
    assert got == [hashlib.sha512(b"\x01" + a + b).digest()[:32].hex() for a, b in pairs]


@pytest.mark.parametrize("t_log", (2, 3))
def test_trees_of_every_size_with_small_tiles(check, leaf_file, t_log):
    path, leaves = leaf_file
    rows = [line.split(" ") for line in check("trees", t_log, path).splitlines() if line.startswith("TREE")]
    assert [int(r[1]) for r in rows] == list(range(NMAX + 1))
    for _, n, root, store in rows:
        n = int(n)
        assert root == M.mth(leaves[:n]).hex(), n
        assert store == M.node_store(leaves[:n]).hex(), n                 # every stored node, level by level


def test_paths_and_checks_of_every_leaf(check, leaf_file):
    path, leaves = leaf_file
    out = check("receipts", path)
    rows = [line.split(" ") for line in out.splitlines() if line.startswith("PATH")]
    assert len(rows) == sum(n + 2 for n in range(NMAX + 1))
    honest = 0
    for _, n, i, length, row in rows:
        n, i, length = int(n), int(i), int(length)
        d = M.depth(n)
        if i >= n:                                                        # index N and N + 1
            assert length == M.NO_PATH and row == "00" * 32 * d, (n, i)
            continue
        want = M.path(i, leaves[:n])
        assert length == len(want) and row == (b"".join(want) + bytes(32 * (d - length))).hex(), (n, i)
        honest += 1
    proven, bad_index, bad_length, mismatch = map(int, re.search(r"VERDICTS (\d+) (\d+) (\d+) (\d+)", out).groups())
    assert proven == honest == NMAX * (NMAX + 1) // 2 and bad_index == 4 * 2 * (NMAX + 1)
    assert bad_length == sum(M.depth(n) + 3 for n in range(NMAX + 1) for _ in range(n))          # every wrong path_len and NO_PATH
    assert mismatch == sum(2 + M.path_len(i, n) for n in range(NMAX + 1) for i in range(n))      # leaf, root, every path entry


MSG_LENS = (110, 111, 112, 127, 128, 239, 240, 736)
PREFIX_LENS = (0, 1, 63, 64, 255)


def _leaf_groups():
    """200 items in groups of one (msg_len, prefix_len, extra): message lengths around the block seams, with and without extras, hand-made
    status words; then the append at the exact fit and one entry short"""
    rng = random.Random(11)
    groups = []
    combos = [(m, p, e) for m in MSG_LENS for p in PREFIX_LENS for e in (0, 64)]
    for k, (m, p, e) in enumerate(combos):
        n = 3 if k < 40 else 2                                            # 40 x 3 + 40 x 2 = 200
        status = [0] * n
        if k % 3 == 0:
            status[k % n] = 6 | (k << 8)
        if k == 5:
            status = [2] * n                                              # nobody participates
        msgs = [rng.randbytes(m) for _ in range(n)]
        extras = [rng.randbytes(e) for _ in range(n)]
        n_prior = (0, 7, 1 << 20)[k % 3]
        groups.append((msgs, extras, status, rng.randbytes(p), n_prior, n_prior + n))
    assert sum(len(g[0]) for g in groups) == 200
    msgs = [rng.randbytes(112) for _ in range(9)]
    status = [0, 0, 4, 0, 0, 0, 1, 0, 0]
    for cap in (12, 11, 5):                                               # seven leaves behind five: the exact fit, one short, no room at all
        groups.append((msgs, [b""] * 9, status, b"id", 5, cap))
    groups.append(([], [], [], b"", 3, 3))                                # n == 0
    return groups


def test_leaf_pass_around_the_block_seams_and_the_append(check, tmp_path):
    groups = _leaf_groups()
    lines = []
    for msgs, extras, status, prefix, n_prior, cap in groups:
        m = len(msgs[0]) if msgs else 0
        e = len(extras[0]) if extras else 0
        lines.append(f"{len(msgs)} {m} {e} {n_prior} {cap} {prefix.hex() or '-'}")
        lines += [f"{s} {a.hex() or '-'} {b.hex() or '-'}" for s, a, b in zip(status, msgs, extras)]
    path = tmp_path / "leaves.txt"
    path.write_text("\n".join(lines) + "\n")
    out = [line for line in check("leaves", path).splitlines() if line.split(" ")[0] in ("INDEX", "LEAVES", "LOG", "FOUND")]
    assert len(out) == 4 * len(groups)
    fits = []
    for k, (msgs, extras, status, prefix, n_prior, cap) in enumerate(groups):
        want = M.leaves_pass(msgs, prefix, extras, status, n_prior, cap)
        index, leaves, log, found = (line.split(" ") for line in out[4 * k:4 * k + 4])
        assert [int(x) for x in index[1:]] == want["leaf_index"], k
        assert leaves[1] == b"".join(want["leaves_out"]).hex(), k
        assert int(log[1]) == want["log_count"] and log[2] == b"".join(want["appended"]).hex(), k
        assert [int(x) for x in found[1:]] == want["found"], k
        fits.append(want["found"][1])
    assert fits[-4:] == [0, 1, 1, 0] and not any(fits[:-4])


def test_hostcheck_layouts_against_a_direct_count(check):
    def up(x):
        return (x + 255) // 256 * 256

    for n in (0, 1, 200, 1024, 1025, 65536, (1 << 20) + 3, 10 ** 7, (1 << 31) - 1):
        tiles = (n + 1023) // 1024
        head, pos, sums, word, rows = (256 if n else 0), up(4 * n), up(4 * tiles), (256 if n else 0), up(32 * n)
        out = check("layout", n)
        assert f"LEAF tiles {tiles} head 0 pos {head} tile_sums {head + pos} total_word {head + pos + sums} leaves {head + pos + sums + word} total {head + pos + sums + word + rows}\n" in out, n
        ping = up(32 * -(-n // 1024)) if n > 1024 else 0
        pong = up(32 * -(-n // (1 << 20))) if n > 1024 else 0
        assert f"TREE ping 0 pong {ping} total {ping + pong}\n" in out, n
        lib = eg._load()
        assert lib.eg_merkle_leaves_scratch_bytes(n) == head + pos + sums + word + rows and lib.eg_merkle_tree_scratch_bytes(n) == ping + pong
    assert eg._load().eg_merkle_leaves_scratch_bytes(1 << 31) == 0 == eg._load().eg_merkle_tree_scratch_bytes(1 << 31)


# ------------------------------------------------------------------ the pure host functions of the library
def test_depth_level_and_nodes_bytes_against_a_direct_count():
    lib = eg._load()
    sizes = list(range(0, 71)) + [(1 << 10) + d for d in (-1, 0, 1)] + [(1 << 20) + d for d in (-1, 0, 1, 3)] + [(1 << 31) - 2, (1 << 31) - 1]
    for n in sizes:
        counts = [n]
        while counts[-1] > 1:
            counts.append((counts[-1] + 1) // 2)                         # the promotion rule, level by level
        depth = len(counts) - 1 if n else 0
        assert lib.eg_merkle_depth(n) == depth == M.depth(n) == eg.ReceiptLog.depth(n), n
        assert lib.eg_merkle_nodes_bytes(n) == 32 * sum(counts[1:]) == eg.ReceiptLog.nodes_bytes(n), n
        off = 0
        for level in range(depth + 1):
            want = (0, n) if level == 0 else (off, counts[level])
            assert eg.ReceiptLog.level(n, level) == want, (n, level)
            if level:
                off += 32 * counts[level]
        a, b = C.c_uint64(5), C.c_uint64(6)
        for level in (-1, depth + 1, 64):
            assert lib.eg_merkle_level(n, level, C.byref(a), C.byref(b)) == BAD_ARG and b"level is not in" in lib.eg_last_error()
        assert (a.value, b.value) == (5, 6)
    a = C.c_uint64(0)
    assert lib.eg_merkle_level(1 << 31, 0, C.byref(a), C.byref(a)) == BAD_ARG and b"N is 2^31 or more" in lib.eg_last_error()
    assert lib.eg_merkle_level(5, 1, None, C.byref(a)) == BAD_ARG and lib.eg_merkle_level(5, 1, C.byref(a), None) == BAD_ARG
    assert lib.eg_merkle_nodes_bytes(1 << 31) == 0 and lib.eg_merkle_depth(1 << 31) == 31 and lib.eg_merkle_depth((1 << 31) + 1) == 32
    with pytest.raises(eg.EgError, match="level is not in"):
        eg.ReceiptLog.level(5, 4)


# ------------------------------------------------------------------ refusals of the library that need no GPU
def test_refusals_of_the_eight_entries_without_a_gpu():
    """the argument rules come before the context is looked at; what passes them fails on the missing context"""
    lib = eg._load()
    buf = C.create_string_buffer(1 << 12)
    base = (C.addressof(buf) + 15) & ~15
    P = C.c_void_p
    big = 1 << 31

    def err():
        return lib.eg_last_error()

    def leaves_dev(n=1, msgs=base, stride=40, mlen=40, prefix=None, plen=0, extra=None, estride=0, elen=0, st=None, n_prior=0, idx=base, out=None,
                   log=None, cap=0, count=None, found=base, scratch=base, sbytes=1 << 20):
        return lib.eg_merkle_leaves_device(None, n, P(msgs), stride, mlen, prefix, plen, P(extra), estride, elen, P(st), n_prior, P(idx), P(out), P(log),
                                           cap, P(count), P(found), P(scratch), sbytes, None)

    def leaves_host(n=1, msgs=base, stride=40, mlen=40, prefix=None, plen=0, extra=None, estride=0, elen=0, st=None, n_prior=0, idx=base, out=None,
                    log=None, cap=0, count=None, found=base, **_):
        return lib.eg_merkle_leaves(None, n, C.cast(P(msgs), C.c_char_p), stride, mlen, prefix, plen, C.cast(P(extra), C.c_char_p), estride, elen, P(st),
                                    n_prior, P(idx), P(out), P(log), cap, P(count), P(found))

    common = (({"n": big}, b"n is 2^31 or more"), ({"n": 1 << 40}, b"n is 2^31 or more"), ({"plen": 256, "prefix": b"x" * 256}, b"prefix_len is above 255"),
              ({"plen": 3}, b"null prefix with a length"), ({"stride": 39}, b"msg_stride is below msg_len"),
              ({"extra": base, "estride": 63, "elen": 64}, b"extra_stride is below extra_len"), ({"msgs": None}, b"null msgs"),
              ({"estride": 64, "elen": 64}, b"null extra with a length"), ({"n_prior": big}, b"n_prior is 2^31 or more"),
              ({"idx": None}, b"null leaf_index or found"), ({"found": None}, b"null leaf_index or found"),
              ({"n_prior": 6, "cap": 5, "log": base, "count": base}, b"n_prior is above log_cap"), ({"cap": 5, "count": base}, b"null log with an append requested"))
    within = ({}, {"n": big - 1, "sbytes": 1 << 50}, {"plen": 255, "prefix": b"x" * 255}, {"extra": base, "estride": 64, "elen": 64}, {"mlen": 0, "stride": 0, "msgs": None},
              {"n": 0, "msgs": None, "idx": None, "found": None, "scratch": None, "sbytes": 0}, {"n_prior": 6, "cap": 5}, {"n_prior": 5, "cap": 5, "log": base, "count": base},
              {"st": base, "out": base, "msgs": base + 1, "extra": base + 3, "estride": 1, "elen": 1})
    for call in (leaves_dev, leaves_host):
        for kw, text in common:
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in within:
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    need = lib.eg_merkle_leaves_scratch_bytes(1)
    assert need == 5 * 256
    for kw in ({"scratch": None}, {"sbytes": 0}, {"sbytes": need - 1}):
        assert leaves_dev(**kw) == BAD_ARG and b"scratch is null or too small" in err(), kw
    assert leaves_dev(sbytes=need) == BAD_ARG and b"null ctx" in err()
    for kw in ({"idx": base + 4}, {"count": base + 4, "log": base, "cap": 9}):
        assert leaves_dev(**kw) == BAD_ARG and b"8-byte aligned" in err(), kw
    for kw in ({"out": base + 2}, {"log": base + 1, "count": base, "cap": 9}, {"st": base + 2}, {"found": base + 2}, {"scratch": base + 1}):
        assert leaves_dev(**kw) == BAD_ARG and b"4-byte aligned" in err(), kw

    # the tree
    def tree_dev(n=5, log=base, root=base, nodes=base, scratch=None, sbytes=0):
        return lib.eg_merkle_tree_device(None, n, P(log), P(root), P(nodes), P(scratch), sbytes, None)

    def tree_host(n=5, log=base, root=base, nodes=base, **_):
        return lib.eg_merkle_tree(None, n, C.cast(P(log), C.c_char_p), P(root), P(nodes))

    for call in (tree_dev, tree_host):
        for kw, text in (({"n": big}, b"N is 2^31 or more"), ({"root": None}, b"null root"), ({"log": None}, b"null log")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in ({}, {"n": 0, "log": None}, {"nodes": None}, {"n": 1024, "nodes": None}, {"n": big - 1}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    need = lib.eg_merkle_tree_scratch_bytes(1025)
    assert need == 512 and lib.eg_merkle_tree_scratch_bytes(1024) == 0
    for kw in ({"scratch": None}, {"scratch": base, "sbytes": need - 1}):
        assert tree_dev(n=1025, nodes=None, **kw) == BAD_ARG and b"scratch is null or too small" in err(), kw
    assert tree_dev(n=1025, nodes=None, scratch=base, sbytes=need) == BAD_ARG and b"null ctx" in err()
    assert tree_dev(n=1025, scratch=None) == BAD_ARG and b"null ctx" in err()          # with a node store no scratch is needed
    for kw in ({"log": base + 2}, {"root": base + 1}, {"nodes": base + 2}, {"scratch": base + 2}):
        assert tree_dev(**kw) == BAD_ARG and b"4-byte aligned" in err(), kw

    # paths
    def paths_dev(m=1, idx=base, n=5, log=base, nodes=base, paths=base, plen=base):
        return lib.eg_merkle_paths_device(None, m, P(idx), n, P(log), P(nodes), P(paths), P(plen), None)

    def paths_host(m=1, idx=base, n=5, log=base, nodes=base, paths=base, plen=base):
        return lib.eg_merkle_paths(None, m, P(idx), n, C.cast(P(log), C.c_char_p), C.cast(P(nodes), C.c_char_p), P(paths), P(plen))

    for call in (paths_dev, paths_host):
        for kw, text in (({"m": big}, b"m is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"), ({"idx": None}, b"null index or path_len"),
                         ({"plen": None}, b"null index or path_len"), ({"log": None}, b"null log, nodes or paths"), ({"nodes": None}, b"null log, nodes or paths"),
                         ({"paths": None}, b"null log, nodes or paths")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in ({}, {"m": 0, "idx": None, "plen": None, "log": None, "nodes": None, "paths": None}, {"n": 1, "log": None, "nodes": None, "paths": None},
                   {"n": 0, "log": None, "nodes": None, "paths": None}, {"m": big - 1, "n": big - 1}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    assert paths_dev(idx=base + 4) == BAD_ARG and b"8-byte aligned" in err()
    for kw in ({"log": base + 2}, {"nodes": base + 1}, {"paths": base + 2}, {"plen": base + 2}):
        assert paths_dev(**kw) == BAD_ARG and b"4-byte aligned" in err(), kw

    # the check
    def check_dev(m=1, idx=base, leaves=base, paths=base, stride=96, plen=base, n=5, root=base, verdict=base, found=base):
        return lib.eg_merkle_check_device(None, m, P(idx), P(leaves), P(paths), stride, P(plen), n, P(root), P(verdict), P(found), None)

    def check_host(m=1, idx=base, leaves=base, paths=base, stride=96, plen=base, n=5, root=base, verdict=base, found=base):
        return lib.eg_merkle_check(None, m, P(idx), C.cast(P(leaves), C.c_char_p), C.cast(P(paths), C.c_char_p), stride, P(plen), n, C.cast(P(root), C.c_char_p),
                                   P(verdict), P(found))

    for call in (check_dev, check_host):
        for kw, text in (({"m": big}, b"m is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"), ({"stride": 95}, b"path_stride is below 32 * depth(N)"),
                         ({"stride": 64}, b"path_stride is below 32 * depth(N)"), ({"n": 1025, "stride": 320}, b"path_stride is below 32 * depth(N)"),
                         ({"stride": 98}, b"path_stride is no multiple of 4"), ({"paths": None}, b"null paths")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for name in ("idx", "leaves", "plen", "root", "verdict", "found"):
            assert call(**{name: None}) == BAD_ARG and b"null index, leaves, path_len, root, verdict or found" in err(), (call.__name__, name)
        for kw in ({}, {"stride": 128}, {"n": 1025, "stride": 352}, {"n": 1, "stride": 0, "paths": None}, {"n": 0, "stride": 0, "paths": None},
                   {"m": 0, "idx": None, "leaves": None, "paths": None, "plen": None, "root": None, "verdict": None, "found": None}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    assert check_dev(idx=base + 4) == BAD_ARG and b"8-byte aligned" in err()
    for name in ("leaves", "paths", "plen", "root", "verdict", "found"):
        assert check_dev(**{name: base + 2}) == BAD_ARG and b"4-byte aligned" in err(), name


def test_missing_gpu_is_loud():
    log = object.__new__(eg.ReceiptLog)
    log.ctx, log.prefix = type("NoCtx", (), {"_h": None})(), b"election"
    with pytest.raises(eg.EgError, match="null ctx"):
        log.leaves(bytes(80), 40, status_in=[0, 5])
    with pytest.raises(eg.EgError, match="null ctx"):
        log.leaves(bytes(80), 40, extra=bytes(128), extra_len=64, log=bytes(64))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.tree(bytes(96))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.paths([0, 2, 9], bytes(96), bytes(96))
    with pytest.raises(eg.EgError, match="null ctx"):
        log.check([0, 2], bytes(64), [bytes(64), bytes(32)], 3, bytes(32))
    log.prefix = bytes(256)
    with pytest.raises(eg.EgError, match="prefix_len is above 255"):
        log.leaves(bytes(80), 40)
