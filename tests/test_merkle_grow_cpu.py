"""The receipt log's grow entry (eg_merkle_grow / eg_merkle_grow_device) without a GPU:
* the surface: the symbols declared, exported, bound, mirrored and in INTEGRATION.md; the header's section behind the audit entries; the
  C++ mirror compiles; plain C99; no environment knob, no waiting loop and k_merkle_tile left as it is;
* tests/hostcheck/merklegrowcheck.cpp: merkle_grow_host.hpp, the lane function of the copy kernel and merkle_tile_step driven from tile0
  under ASan + UBSan, run serially with tiles of 4 and 8 for every 0 <= m <= N <= 70 with everything that must never be read poisoned;
  store and root against the model tests/merkle_ref.py (hashlib only);
* the plan (copy rows, tile0 per launch, copied nodes) against a direct count, T = 2 and 3 for every m <= N <= 70 and T = 10 around 2^10,
  2^20 and 2^31 - 1;
* every refusal that needs no GPU."""
import ctypes as C
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
    "eg_merkle_grow_device": ("int", C.c_int, 8),
    "eg_merkle_grow": ("int", C.c_int, 7),
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
    # inside the receipt-log section, directly behind the audit entries and in front of the multi-GPU tier; no section line of its own
    section, nxt = header.index("/* ---- receipt log"), header.index("/* ---- batch tier on several GPUs")
    last_audit = header.index("int eg_merkle_consistency_check(")
    for name in ENTRIES:
        assert section < last_audit < header.index(f"int {name}(") < nxt, name
    assert header[section:nxt].count("/* ---- ") == 1
    assert "eg_" not in re.sub(r"/\*.*?\*/", "", header[header.index(";", last_audit):header.index("int eg_merkle_grow_device(")], flags=re.S)
    text = re.sub(r"\s*\n \*\s*", " ", header[last_audit:nxt])
    for phrase in ("GROW", "byte for byte what eg_merkle_tree", "(j + 1) 2^L <= m", "tile0 = (m >> L0) >> 10", "COPIED", "NEVER READ", "(m >> 10) << 10",
                   "(j + 1) 2^L > m", "OUT OF PLACE", "left untouched", "not overlap", "m == 0 is a full build", "needs no scratch", "takes no lock",
                   "never synchronises", "before the context is looked at", "variable time"):
        assert phrase in text, phrase
    for m in ("grow", "grow_device"):
        assert callable(getattr(eg.ReceiptLog, m)), m
    ffi = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name
    for doc, words in (("README.md", ("merkle_grow_kernels.cuh", "test_gpu_merkle_grow.py", "eg_merkle_grow")),
                       ("DESIGN.md", ("k_merkle_grow_copy", "k_merkle_grow_tile", "capacity", "compact range")), ("INTEGRATION.md", ("eg_merkle_grow",))):
        text = (ROOT / doc).read_text()
        for w in words:
            assert w in text, (doc, w)
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7


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
            MerkleTree old = rl.tree(Bytes(log.begin(), log.begin() + 4 * 32));
            MerkleTree t = rl.grow(4, old, log);
            rl.grow_device(0, nullptr, 0, nullptr, nullptr, nullptr);
            return (int)(t.root.size() + t.nodes.size());
          }
          return 0;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    names = " && ".join(ENTRIES)
    src.write_text(f'#include "eg_hip.h"\nint main(void) {{ return {names} ? 0 : 1; }}\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-address", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_the_tree_kernel_is_left_alone():
    for f in ("merkle_grow_kernels.cuh", "merkle_grow_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    host = (CSRC / "merkle_grow_host.hpp").read_text()
    assert "#include <hip" not in host and "__global__" not in host and '#include "merkle_host.hpp"' in host        # pure host code
    for name in ("grow_plan", "refuse_grow", "ranges_overlap"):
        assert re.search(rf"\b{name}\(", host), name
    kernels = (CSRC / "merkle_grow_kernels.cuh").read_text()
    # no fences, no atomics, no waiting loops: the kernel boundary on the one stream is the only order between the copy and the tiles
    assert not re.search(r"\bwhile\b", kernels) and "__threadfence" not in kernels and "__builtin_amdgcn" not in kernels and "asm" not in kernels
    assert "atomic" not in kernels and "hipMalloc" not in kernels
    assert re.search(r"__global__ void __launch_bounds__\(MERKLE_NT\) k_merkle_grow_copy\(", kernels)
    assert re.search(r"template <int TL>\s*__global__ void __launch_bounds__\(1 << \(TL - 2\)\) k_merkle_grow_tile\(u32 tile0, MerkleTileArgs a\)", kernels)
    assert "merkle_tile_step<TL>(mem, tile, s, t, a.n_in)" in kernels and "MerkleTileDev<TL> mem{a, odd, even}" in kernels and "uint4" in kernels
    tree = (CSRC / "merkle_kernels.cuh").read_text()
    assert "merkle_tile_step<TL>(mem, blockIdx.x, s, t, a.n_in)" in tree and "grow" not in tree                     # k_merkle_tile as it was
    lib = (CSRC / "eg_hip.hip").read_text()
    assert '#include "merkle_grow_kernels.cuh"' in lib
    body = lib[lib.index("int eg_merkle_grow_device("):lib.index("int eg_merkle_grow(eg_ctx")]
    assert "hipMalloc" not in body and "Synchronize" not in body and "EG_LOCK" not in body and "k_merkle_root" in body
    assert body.index("refuse_grow") < body.index("check_aligned") < body.index("check_ctx") < body.index("hipLaunchKernelGGL")
    assert body.index("k_merkle_grow_copy") < body.index("k_merkle_grow_tile") < body.index("k_merkle_root")           # the order on the stream


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "merklegrowcheck", HERE / "merklegrowcheck.cpp"
    deps = [src, CSRC / "merkle_grow_kernels.cuh", CSRC / "merkle_grow_host.hpp", CSRC / "merkle_kernels.cuh", CSRC / "merkle_host.hpp", CSRC / "sha512.cuh",
            CSRC / "fe25519.cuh"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout

    return run


def _leaves(n, seed=1):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(n)]


@pytest.mark.parametrize("t_log", (2, 3))
def test_grow_of_every_pair_of_sizes_with_small_tiles(check, tmp_path, t_log):
    """every 0 <= m <= N <= 70: the program overwrites and poisons the old store's nodes with (j + 1) 2^L > m and the leaves below
    (m >> T) << T before the pass runs (a pass that rebuilds, or copies a ragged node, aborts under ASan or gives other bytes); the
    expected store and root are the model's over the UNPOISONED leaves"""
    leaves = _leaves(NMAX, seed=7)
    path = tmp_path / "leaves.txt"
    path.write_text("\n".join(x.hex() for x in leaves) + "\n")
    rows = [line.split(" ") for line in check("grow", t_log, path).splitlines() if line.startswith("GROW")]
    assert [(int(r[1]), int(r[2])) for r in rows] == [(m, n) for m in range(NMAX + 1) for n in range(m, NMAX + 1)]
    want = {n: (M.mth(leaves[:n]).hex(), M.node_store(leaves[:n]).hex()) for n in range(NMAX + 1)}
    assert want[0] == (M.H(b"").hex(), "") and want[1] == (leaves[0].hex(), "")
    for _, m, n, root, store in rows:
        assert (root, store) == want[int(n)], (m, n)


# ------------------------------------------------------------------ the plan: arithmetic only
def _level_offset(n, level):
    return sum(M.level_count(n, k) for k in range(1, level))


def _parse_plans(out):
    plans, cur = {}, None
    for line in out.splitlines():
        f = line.split(" ")
        if f[0] == "PLAN":
            cur = plans[int(f[1]), int(f[2])] = {"launch": [], "rows": [], "copied": None}
        elif f[0] == "LAUNCH":
            cur["launch"].append(tuple(map(int, f[1:])))
        elif f[0] == "ROW":
            cur["rows"].append(tuple(map(int, f[1:])))
        elif f[0] == "COPIED":
            cur["copied"] = int(f[1])
    return plans


def _plan_by_formula(m, n, t):
    """launch k reduces input level L0 = k t; its first (m >> L0) >> t tiles lie wholly inside the first m leaves"""
    launch, rows, depth = [], [], M.depth(n)
    for level in range(0, depth, t):
        steps, n_in = min(t, depth - level), M.level_count(n, level)
        tile0 = m >> (level + t)
        launch.append((level, steps, n_in, -(-n_in // (1 << t)), tile0))
        if tile0:
            rows += [(_level_offset(m, level + s), _level_offset(n, level + s), tile0 << (t - s)) for s in range(1, steps + 1)]
    return launch, rows


@pytest.mark.parametrize("t_log", (2, 3))
def test_plan_against_a_direct_count_of_every_node(check, t_log):
    plans = _parse_plans(check("plans", t_log, NMAX))
    assert sorted(plans) == [(m, n) for m in range(NMAX + 1) for n in range(m, NMAX + 1)]
    size = 1 << t_log
    for (m, n), p in plans.items():
        # node by node: (L, j) belongs to tile j >> (t - s) of the launch with input level L0 = t ((L - 1) // t), s = L - L0; that tile is
        # copied iff ALL the leaves it spans are old, (tile + 1) 2^(L0 + t) <= m
        copied = {}
        for level in range(1, M.depth(n) + 1):
            l0 = (level - 1) // t_log * t_log
            s = level - l0
            js = [j for j in range(M.level_count(n, level)) if ((j >> (t_log - s)) + 1) << (l0 + t_log) <= m]
            assert all((j + 1) << level <= m for j in js)                    # only nodes that the append cannot have changed
            assert js == list(range(len(js)))                              # a prefix of the level
            if js:
                copied[level] = len(js)
        rows = [(_level_offset(m, level), _level_offset(n, level), count) for level, count in sorted(copied.items())]
        assert p["rows"] == rows and p["copied"] == sum(copied.values()), (m, n)
        assert (p["launch"], p["rows"]) == _plan_by_formula(m, n, t_log), (m, n)
        for level, steps, n_in, tiles, tile0 in p["launch"]:
            assert tile0 <= tiles and tile0 * size <= m >> level and (tile0 + 1) * size > m >> level, (m, n, level)
        for src, dst, count in p["rows"]:
            assert src + count <= _level_offset(m, M.depth(m) + 1) and dst + count <= _level_offset(n, M.depth(n) + 1), (m, n)
        if m == n and n and n & (n - 1) == 0 and M.depth(n) % t_log == 0:
            assert all(tile0 == tiles for *_, tiles, tile0 in p["launch"]) and p["copied"] == n - 1       # a pure copy
        if m < size:
            assert p["copied"] == 0 and not p["rows"]                       # a full build


def test_plan_of_the_library_tile_around_the_large_seams(check):
    big = (1 << 31) - 1
    sizes = [(1 << 10) + d for d in (-1, 0, 1)] + [(1 << 20) + d for d in (-1, 0, 1, 3, 1030)] + [big - 1, big]
    olds = [0, 1, 1023, 1024, 1025, 2047, 2048, (1 << 20) - 1, 1 << 20, (1 << 20) + 3, (1 << 30) - 1, 1 << 30, (1 << 30) + 1025, big - 1024, big - 1, big]
    for n in sizes:
        for m in sorted({o for o in olds + [n - 1, n] if 0 <= o <= n}):
            p = _parse_plans(check("plan", 10, m, n))[m, n]
            assert (p["launch"], p["rows"]) == _plan_by_formula(m, n, 10), (m, n)
            assert p["copied"] == sum(c for _, _, c in p["rows"]) and len(p["rows"]) <= 31 and len(p["launch"]) <= 4
            total_m, total_n = _level_offset(m, M.depth(m) + 1), _level_offset(n, M.depth(n) + 1)
            for k, (src, dst, count) in enumerate(p["rows"]):
                assert src + count <= total_m and dst + count <= total_n, (m, n, k)
            # the tiles from tile0 on make the nodes from tile0 << (10 - s) on of level L0 + s
            hashed = sum(sum(M.level_count(n, level + s) - (tile0 << (10 - s)) for s in range(1, steps + 1)) for level, steps, _, _, tile0 in p["launch"])
            assert p["copied"] + hashed == total_n, (m, n)                  # every node of the new store exactly once
    p = _parse_plans(check("plan", 10, 1 << 20, 1 << 20))[1 << 20, 1 << 20]
    assert p["copied"] == (1 << 20) - 1 and all(t0 == t for *_, t, t0 in p["launch"])
    p = _parse_plans(check("plan", 10, (1 << 20) - 1, (1 << 20) + 3))[(1 << 20) - 1, (1 << 20) + 3]
    assert [x[4] for x in p["launch"]] == [1023, 0, 0] and [x[1] for x in p["launch"]] == [10, 10, 1] and len(p["rows"]) == 10
    for a, na, b, nb, want in ((100, 10, 110, 5, 0), (100, 10, 109, 5, 1), (110, 5, 100, 10, 0), (109, 5, 100, 10, 1), (100, 10, 100, 0, 0), (100, 0, 100, 10, 0),
                               (100, 50, 120, 1, 1), (120, 1, 100, 50, 1), (big << 32, 1 << 36, (big << 32) + (1 << 36) - 1, 1, 1)):
        assert f"OVERLAP {want}\n" in check("overlap", a, na, b, nb), (a, na, b, nb)


# ------------------------------------------------------------------ refusals of the library that need no GPU
def test_refusals_of_the_two_entries_without_a_gpu():
    """the argument rules come before the context is looked at; what passes them fails on the missing context"""
    lib = eg._load()
    buf = C.create_string_buffer((1 << 14) + 16)
    base = (C.addressof(buf) + 15) & ~15
    P = C.c_void_p
    big = 1 << 31
    at = {"log": base, "old": base + 4096, "nodes": base + 8192, "root": base + 12288}
    old0, new0 = at["old"], at["nodes"]                                     # m = 5: 6 nodes = 192 bytes; N = 9: 11 nodes = 352 bytes
    assert lib.eg_merkle_nodes_bytes(5) == 192 and lib.eg_merkle_nodes_bytes(9) == 352

    def err():
        return lib.eg_last_error()

    def chars(p):
        return C.cast(P(p), C.c_char_p)

    def dev(m=5, old=old0, n=9, log=at["log"], nodes=new0, root=at["root"]):
        return lib.eg_merkle_grow_device(None, m, P(old), n, P(log), P(nodes), P(root), None)

    def host(m=5, old=old0, n=9, log=at["log"], nodes=new0, root=at["root"]):
        return lib.eg_merkle_grow(None, m, chars(old), n, chars(log), P(nodes), P(root))

    for call in (dev, host):
        for kw, text in (({"m": 10}, b"old_size is above N"), ({"m": 1, "n": 0}, b"old_size is above N"), ({"m": big - 1, "n": big - 2}, b"old_size is above N"),
                         ({"m": big, "n": big}, b"old_size is 2^31 or more"), ({"m": big}, b"old_size is 2^31 or more"), ({"n": big}, b"N is 2^31 or more"),
                         ({"root": None}, b"null root"), ({"log": None}, b"null log"), ({"m": 1, "n": 1, "log": None}, b"null log"),
                         ({"nodes": None}, b"null nodes"), ({"m": 0, "n": 2, "nodes": None}, b"null nodes"), ({"old": None}, b"null nodes_old"),
                         ({"m": 2, "old": None}, b"null nodes_old"),
                         # overlap: the same place, from either side, and by one byte
                         ({"nodes": old0}, b"overlap"), ({"nodes": old0 + 188}, b"overlap"), ({"nodes": old0 + 191}, b"overlap"),
                         ({"nodes": old0 - 348}, b"overlap"), ({"nodes": old0 - 351}, b"overlap"), ({"old": new0 + 351}, b"overlap"),
                         ({"old": new0 - 191}, b"overlap"), ({"nodes": old0 + 32, "n": 5}, b"overlap"), ({"m": big - 1, "n": big - 1}, b"overlap")):
            assert call(**kw) == BAD_ARG and text in err(), (call.__name__, kw, err())
        for kw in ({}, {"m": 9}, {"m": 0, "old": None}, {"m": 1, "old": None}, {"m": 0, "n": 0, "old": None, "log": None, "nodes": None},
                   {"m": 1, "n": 1, "old": None, "nodes": None}, {"m": 0, "n": 1, "old": None, "nodes": None},
                   {"m": big - 1, "n": big - 1, "old": 1 << 40, "nodes": 1 << 44},  # addresses are compared, never followed
                   # the stores touch and do not overlap; an empty old store overlaps nothing
                   {"nodes": old0 + 192}, {"nodes": old0 - 352}, {"old": new0 + 352}, {"old": new0 - 192}, {"m": 1, "old": new0 + 8}, {"m": 0, "old": new0}):
            assert call(**kw) == BAD_ARG and b"merkle: null ctx" in err(), (call.__name__, kw, err())
    for name in ("old", "log", "nodes", "root"):
        for off in (1, 2, 3):
            assert dev(**{name: at[name] + off}) == BAD_ARG and b"4-byte aligned" in err(), (name, off)
        assert host(**{name: at[name] + 1}) == BAD_ARG and b"merkle: null ctx" in err(), name                        # host arrays may lie anywhere
    assert dev(**{name: at[name] + 4 for name in ("old", "log", "nodes", "root")}) == BAD_ARG and b"merkle: null ctx" in err()      # 4 bytes are enough


def test_missing_gpu_is_loud():
    log = object.__new__(eg.ReceiptLog)
    log.ctx, log.prefix = type("NoCtx", (), {"_h": None})(), b"election"
    with pytest.raises(eg.EgError, match="null ctx"):
        log.grow(2, bytes(32), bytes(96))
    with pytest.raises(eg.EgError, match="old_size is above N"):
        log.grow(4, bytes(96), bytes(96))
    with pytest.raises(eg.EgError, match="null nodes_old"):
        log.grow(2, b"", bytes(96))
