"""Weeding against a persistent board index (eg_weed_index_*, eg_*_weed_indexed*; csrc/weed_index_kernels.cuh, csrc/weed_index_host.hpp)
without a GPU.

* The seven entry points are declared, exported, bound in Python and mirrored in C++; the header stays plain C; the FFI block of
  INTEGRATION.md names them; there is no new environment knob; weed_kernels.cuh and weed_host.hpp are the files of the round that
  measured them, byte for byte.
* tests/hostcheck/weedindexcheck.cpp: the lane functions under ASan + UBSan, serially.  A sequence of four batches over a growing
  board goes through the indexed lanes and through the stateless lanes over the same board bytes (compared inside the program) and is
  compared here with the model of the rule in tests/weed_ref.py; 20 lane orders, 3 index seeds; find() over the maintained index
  against a freshly built one; indexes of 8 and 16 slots; the append at the exact fit and one entry short; read-only calls; a garbage
  index; poisoned bytes of ballots that do not participate; the layout of the scratch.
* The refusals of every new entry that need no GPU."""
import ctypes as C
import hashlib
import random
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import weed_ref as W

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
SIZES = ("eg_choice_weed_indexed_scratch_bytes", "eg_qv_weed_indexed_scratch_bytes")
DEVICE = ("eg_choice_weed_indexed_device", "eg_qv_weed_indexed_device")
BAD_ARG = -3


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    table = [(("eg_weed_index_bytes",), "size_t", C.c_size_t, 1), (("eg_weed_index_build_device",), "int", C.c_int, 8),
             (("eg_weed_index_find_device",), "int", C.c_int, 10), (SIZES, "size_t", C.c_size_t, 2), (DEVICE, "int", C.c_int, 16)]
    for names, ret, restype, nargs in table:
        for name in names:
            assert re.search(rf"^{ret} {name}\(", header, re.M), name
            assert name in eg.exported_symbols()
            assert hasattr(raw, name), f"{name} is not exported"
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == nargs, name
    # a section of its own, behind weeding's and in front of the ballot audits
    at = header.index("size_t eg_weed_index_bytes(")
    assert header.index("int eg_qv_weed(") < at < header.index("eg_choice_open_check_scratch_bytes(")
    # the header states the contract
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("BYTE FOR BYTE", "One writer at a time per index", "LIFE OF THE INDEX", "neither the board nor a byte of the index changes",
                   "no reference at or above n_prior is ever dereferenced", "a function of n alone"):
        assert phrase in flat, phrase
    # the ABI version is unchanged
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7


def test_index_bytes():
    lib = eg._load()
    for cap in (0, 1, 511, 512, 513, 1000, 5_000_000, 50_000_000, (1 << 31) - 1):
        slots = 1024
        while slots < 2 * cap:
            slots *= 2
        assert lib.eg_weed_index_bytes(cap) == 4 * slots == eg.Context.weed_index_bytes(cap), cap
    assert lib.eg_weed_index_bytes(1 << 31) == 0 == lib.eg_weed_index_bytes(1 << 40)
    assert lib.eg_weed_index_bytes((1 << 31) - 1) == 1 << 34          # 2^32 slots of 4 bytes


def test_python_and_cpp_mirrors_exist(tmp_path):
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        assert callable(cls.weed_indexed_device) and callable(cls.weed_indexed_scratch_bytes)
    for name in ("weed_index_bytes", "weed_index_build_device", "weed_index_find_device"):
        assert callable(getattr(eg.Context, name))
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count("void weed_indexed_device(") == 2 and hpp.count("size_t weed_indexed_scratch_bytes(size_t n) const") == 2
    assert "struct BoardIndex {" in hpp
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        template <class P> void dev(const P& p, const BoardIndex& ix) {
          p.weed_indexed_device(0, nullptr, nullptr, 0, nullptr, ix.board_cap, nullptr, ix.index_seed, 1234567, nullptr, nullptr, nullptr, nullptr,
                                nullptr);
          p.weed_indexed_device(0, nullptr, nullptr, 0, nullptr, ix.board_cap, nullptr, ix.index_seed, 1234567, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr);
          (void)p.weed_indexed_scratch_bytes(3);
        }
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element pk{};
            ChoiceParams c = ChoiceParams::single(ctx, pk, 5);
            QuadraticVotingParams q(ctx, pk, 5, 20);
            const BoardIndex ix{ctx, 1000, 99};
            ix.build_device(0, nullptr, nullptr, nullptr);
            ix.find_device(0, nullptr, 0, nullptr, nullptr, nullptr);
            dev(c, ix); dev(q, ix);
            return (int)ix.bytes();
          }
          return eg_weed_index_bytes(1000) == 4 * 2048 ? 0 : 1;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return eg_weed_index_bytes && eg_weed_index_build_device && eg_weed_index_find_device && '
                   'eg_choice_weed_indexed_device && eg_qv_weed_indexed_device && eg_choice_weed_indexed_scratch_bytes && '
                   'eg_qv_weed_indexed_scratch_bytes ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ffi_block_is_in_step_with_the_header():
    doc = (ROOT / "INTEGRATION.md").read_text()
    block = doc[doc.index("<!-- ffi:begin"):doc.index("<!-- ffi:end -->")]
    assert "pub fn eg_weed_index_bytes(board_cap: usize) -> usize;" in block
    assert re.search(r"pub fn eg_weed_index_find_device\(ctx: \*mut EgCtx, n_q: usize, d_keys: \*const c_void,", block)
    for name in SIZES + DEVICE + ("eg_weed_index_build_device",):
        assert f"pub fn {name}(" in block, name
    n_args = lambda name: re.search(rf"pub fn {name}\(([^)]*)\)", block).group(1).count(":")
    assert n_args("eg_choice_weed_indexed_device") == n_args("eg_qv_weed_indexed_device") == n_args("eg_choice_weed_device") + 2


def test_no_new_environment_knob_and_no_waiting_between_workgroups():
    for f in ("weed_index_kernels.cuh", "weed_index_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    src = (CSRC / "eg_hip.hip").read_text()
    section = src[src.index("// ---- weeding against a persistent board index"):src.index("// builds the wide comb tables now")]
    assert "getenv" not in section and "knobs" not in section
    assert "hipMalloc" not in section and "Synchronize" not in section and "->mu" not in section          # no allocation, no waiting, no lock
    kernels = (CSRC / "weed_index_kernels.cuh").read_text()
    device = kernels[kernels.index("#if defined(__HIPCC__)"):]
    assert not re.search(r"\bwhile\s*\(", device) and "for (;;)" not in device and "__threadfence" not in device and "__builtin_amdgcn_fence" not in device


def test_the_stateless_sources_are_those_of_the_round_that_measured_them():
    """weed_kernels.cuh and weed_host.hpp are included, not edited: the registers and numbers recorded for the stateless pass stand"""
    want = {"weed_kernels.cuh": "95e9580e82b1cb718db016dbc818d2521e474e13821b8bf5efb39fd0ef05b036",
            "weed_host.hpp": "a432d4e035d61ff0238608c2b35c6cd14dd3a9c15cc36883ffd3268515b76323"}
    for name, digest in want.items():
        assert hashlib.sha256((CSRC / name).read_bytes()).hexdigest() == digest, name
    kernels = (CSRC / "weed_index_kernels.cuh").read_text()
    assert '#include "weed_kernels.cuh"' in kernels and "k_weed_insert" not in kernels[kernels.index("#if defined(__HIPCC__)"):]


# ------------------------------------------------------------------ refusals that need no GPU
def _aligned(buf):
    return (C.addressof(buf) + 15) & ~15


def test_refusals_of_build_and_find_without_a_gpu():
    lib = eg._load()
    buf = C.create_string_buffer(512)
    base = _aligned(buf)
    one = (C.c_uint32 * 4)()

    def build(n_prior=0, board=base, cap=8, index=base + 64, found=one):
        return lib.eg_weed_index_build_device(None, n_prior, board, cap, 5, index, found, None), lib.eg_last_error()

    def find(n_q=1, keys=base + 128, n_prior=0, board=base, cap=8, index=base + 64, pos=one):
        return lib.eg_weed_index_find_device(None, n_q, keys, n_prior, board, cap, index, 5, pos, None), lib.eg_last_error()

    for call in (build, find):
        for kw, text in (({"n_prior": 1 << 31, "cap": 1 << 32}, b"n_prior is 2^31 or more"), ({"n_prior": 9}, b"n_prior is above board_cap"),
                         ({"cap": 1 << 31}, b"board_cap is 2^31 or more"), ({"cap": 1 << 40}, b"board_cap is 2^31 or more"),
                         ({"index": None}, b"null index"), ({"n_prior": 3, "board": None}, b"null board with n_prior"),
                         ({"index": base + 68}, b"16-byte aligned"), ({"board": base + 8}, b"16-byte aligned")):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and text in msg, (call.__name__, kw, msg)
        # what is within the limits fails on the missing context
        for kw in ({}, {"n_prior": 8}, {"cap": (1 << 31) - 1}, {"board": None}):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and b"null ctx" in msg, (call.__name__, kw, msg)
    rc, msg = build(found=None)
    assert rc == BAD_ARG and b"null found" in msg
    rc, msg = build(found=C.addressof(one) + 2)
    assert rc == BAD_ARG and b"misaligned" in msg
    for kw, text in (({"n_q": 1 << 31}, b"n_q is 2^31 or more"), ({"keys": None}, b"null keys"), ({"pos": None}, b"null pos"),
                     ({"keys": base + 132}, b"16-byte aligned"), ({"pos": C.addressof(one) + 1}, b"misaligned")):
        rc, msg = find(**kw)
        assert rc == BAD_ARG and text in msg, (kw, msg)
    rc, msg = find(n_q=0, keys=None, pos=None)
    assert rc == BAD_ARG and b"null ctx" in msg


def test_refusals_of_the_indexed_entries_without_a_gpu():
    """those of the stateless entry, a null index, the alignment of the index, board_cap >= 2^31; what passes fails on the missing params
    object; the scratch size of a refused call is 0"""
    lib = eg._load()
    buf = C.create_string_buffer(512)
    base = _aligned(buf)
    one = (C.c_uint32 * 4)()

    def device(fn, n=1, ballots=base, status=None, n_prior=0, board=base, cap=8, index=base + 64, scratch=base + 128, dup=one, out=None, count=None,
               found=one):
        rc = fn(None, n, ballots, status, n_prior, board, cap, index, 7, 99, scratch, dup, out, count, found, None)
        return rc, lib.eg_last_error()

    for name in DEVICE:
        fn = getattr(lib, name)
        for n in (1 << 31, 1 << 40):
            rc, msg = device(fn, n=n)
            assert rc == BAD_ARG and b"n is 2^31 or more" in msg, (name, n)
        for kw, text in (({"n_prior": 1 << 31, "cap": 1 << 32}, b"n_prior is 2^31 or more"), ({"n_prior": 9}, b"n_prior is above board_cap"),
                         ({"cap": 1 << 31}, b"board_cap is 2^31 or more"), ({"index": None}, b"null index"),
                         ({"ballots": None}, b"null ballots"), ({"dup": None}, b"null dup_of"), ({"found": None}, b"null found"),
                         ({"n_prior": 3, "board": None}, b"null board with n_prior"),
                         ({"board": None, "count": one}, b"null board with an append requested"),
                         ({"ballots": base + 8}, b"16-byte aligned"), ({"board": base + 4}, b"16-byte aligned"),
                         ({"scratch": base + 129}, b"16-byte aligned"), ({"index": base + 72}, b"16-byte aligned"),
                         ({"dup": C.addressof(one) + 2}, b"misaligned")):
            rc, msg = device(fn, **kw)
            assert rc == BAD_ARG and text in msg, (name, kw, msg)
        for kw in ({}, {"n": (1 << 31) - 1}, {"n": 0, "ballots": None, "dup": None}, {"n_prior": 5}, {"cap": (1 << 31) - 1}):
            rc, msg = device(fn, **kw)
            assert rc == BAD_ARG and b"null params" in msg, (name, kw, msg)
    for name in SIZES:
        fn = getattr(lib, name)
        for n in (1 << 31, 1, 100, 0):
            assert fn(None, n) == 0, (name, n)


def test_argument_rules(check):
    assert "REFUSE n is 2^31 or more" in check("refuse", 1 << 31, 0, 0, 5)
    assert "REFUSE n_prior is 2^31 or more" in check("refuse", 1, 1 << 31, 1 << 32, 5)
    assert "REFUSE n_prior is above board_cap" in check("refuse", 1, 9, 8, 5)
    assert "REFUSE board_cap is 2^31 or more" in check("refuse", 1, 9, 1 << 31, 5)
    assert "EG_WEED_KEYS_MAX" in check("refuse", (1 << 30) // 5 + 1, 0, 0, 5)
    # the board no longer counts against the limit: the stateless entry refuses (2^30 / 5) ballots beside five entries
    assert "REFUSE -" in check("refuse", (1 << 30) // 5, (1 << 31) - 1, (1 << 31) - 1, 5)
    assert "REFUSE -" in check("refuse", 0, 0, 0, 5)


def test_missing_gpu_is_loud():
    ctx = object.__new__(eg.Context)
    ctx._h = None
    with pytest.raises(eg.EgError, match="null ctx"):
        ctx.weed_index_build_device(0, 0, 8, 5, 16, 16)
    with pytest.raises(eg.EgError, match="null ctx"):
        ctx.weed_index_find_device(1, 16, 0, 0, 8, 16, 5, 16)
    with pytest.raises(eg.EgError, match="null index"):
        ctx.weed_index_build_device(0, 0, 8, 5, 0, 16)
    for cls, prefix in ((eg.ChoiceParams, "choice"), (eg.QuadraticVotingParams, "qv")):
        p = object.__new__(cls)
        p._h, p._prefix, p.ballot_size, p.n_options = None, prefix, 736, 5
        with pytest.raises(eg.EgError, match="null params"):
            p.weed_indexed_device(1, 16, 0, 0, 0, 8, 16, 7, 5, 16, 16, 16)
        with pytest.raises(eg.EgError, match="null index"):
            p.weed_indexed_device(1, 16, 0, 0, 0, 8, 0, 7, 5, 16, 16, 16)
        assert p.weed_indexed_scratch_bytes(100) == 0


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "weedindexcheck", HERE / "weedindexcheck.cpp"
    deps = [src, *CSRC.glob("*.cuh"), *CSRC.glob("*.hpp"), CSRC / "plan.h"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args, ok=True):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        if ok:
            assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout if ok else r

    return run


K = 3
REJECTED = 6 + (2 << 8)


@pytest.fixture(scope="module")
def sequence():
    """four batches of 45 three-key ballots over a board that starts with 6 entries.  Every batch carries the plants of W.planted (whole
    copies, the chain A{x,y} B{y,z} C{z,w}, a key at another option position, a key twice inside one kept ballot, a copy of a copy) with
    its ballot 2 rejected - the original of the whole copy 7, which then owns the keys.  Across batches: whole copies and single keys of
    ballots appended one and two batches back, copies of the start board, a copy of a rejected ballot of the batch before (which never
    reached the board).  -> (start board, [(ballots, status)], [(dup_of, status_out, appended)] by the model, the final board)"""
    rng = random.Random(23)
    board = [bytes(rng.getrandbits(8) for _ in range(64)) for _ in range(6)]
    start, batches, want, kept = list(board), [], [], []
    for t in range(4):
        ballots, _ = W.planted(100 + t, 45, K, 0)
        status = [0] * 45
        status[2] = REJECTED
        status[40] = status[41] = 9
        ballots[3][0] = start[0]                                     # the start board, in every batch
        ballots[35][K - 1] = start[5]
        if t >= 1:
            ballots[12][1] = kept[t - 1][4][0]                       # one batch back, at another option position
            ballots[13] = list(kept[t - 1][9])                       # ... and a whole ballot
            ballots[14] = list(batches[t - 1][0][41])                # a rejected ballot of the batch before: it never reached the board
            ballots[40] = list(kept[t - 1][1])                       # a rejected copy is left alone
        if t >= 2:
            ballots[15] = list(kept[t - 2][6])                       # two batches back
            ballots[16][2] = kept[t - 2][8][1]
            ballots[44] = list(kept[t - 2][0])                       # at the last lane
        dup, out, appended = W.weed(ballots, status, board)
        assert dup[7] == W.DUP_NONE and dup[33] == 7 and dup[3] == dup[35] == W.DUP_PRIOR and dup[30] == W.DUP_NONE
        assert (dup[20], dup[21], dup[22], dup[23]) == (W.DUP_NONE, 20, 21, 22) and dup[11] == 5
        if t >= 1:
            assert dup[12] == dup[13] == W.DUP_PRIOR and dup[14] == W.DUP_NONE and dup[40] == W.DUP_NONE and out[40] == 9
        if t >= 2:
            assert dup[15] == dup[16] == dup[44] == W.DUP_PRIOR
        kept.append([keys for b, keys in enumerate(ballots) if dup[b] == W.DUP_NONE and status[b] == 0])
        assert b"".join(appended) == b"".join(b"".join(k) for k in kept[-1])
        batches.append((ballots, status))
        want.append((dup, out, appended))
        board = board + appended
    assert len(set(board)) < len(board)                              # a kept ballot carried a key twice: two equal board entries
    return start, batches, want, board


def _write_sequence(path, start, batches, board_cap, append=None):
    lines = [f"{len(batches)} {K} {len(start)} {board_cap}"] + [e.hex() for e in start]
    for t, (ballots, status) in enumerate(batches):
        lines.append(f"{len(ballots)} {1 if append is None else append[t]}")
        lines += [f"{status[b]} {b''.join(keys).hex()}" for b, keys in enumerate(ballots)]
    path.write_text("\n".join(lines) + "\n")


def _batches(out):
    got = []
    for m in re.finditer(r"^BATCH (\d+)\nDUP :(.*)\nSTATUS :(.*)\nFOUND (\d+) (\d+) (\d+)\nCOUNT (\d+)\nINDEX changed (\d) used (\d+)$", out, re.M):
        got.append(dict(dup=[int(x) for x in m.group(2).split()], out=[int(x) for x in m.group(3).split()],
                        found=tuple(int(m.group(i)) for i in (4, 5, 6)), count=int(m.group(7)), changed=int(m.group(8)), used=int(m.group(9))))
    final = re.search(r"^FINAL count (\d+) distinct (\d+) equal_entries (\d+)\nBOARD ([0-9a-f]*)$", out, re.M)
    return got, tuple(int(final.group(i)) for i in (1, 2, 3)), bytes.fromhex(final.group(4))


def test_a_sequence_of_batches_equals_the_stateless_lanes_and_the_model(check, sequence, tmp_path):
    """20 shuffled lane orders and 3 index seeds: after every batch dup_of, status_out, found, the count and the board bytes are those of
    the stateless lanes over the same board (checked inside the program, with a read-only pass in front of every appending one whose
    index bytes must not change) and of the model; afterwards find() over the maintained index gives, for every board entry and 100
    absent keys, the answers of a freshly built one - the smallest position"""
    start, batches, want, board = sequence
    _write_sequence(tmp_path / "seq.txt", start, batches, len(board))          # the exact fit of the last batch
    runs = [(0, 0)] + [(0, order) for order in range(1, 21)] + [(seed, 3) for seed in (1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1)]
    for seed, order in runs:
        got, (count, distinct, equal_entries), brd = _batches(check("seq", tmp_path / "seq.txt", seed, order))
        assert len(got) == 4
        n_prior = len(start)
        for t, g in enumerate(got):
            dup, out, appended = want[t]
            n_prior += len(appended)
            assert g["dup"] == dup and g["out"] == out, (seed, order, t)
            assert g["found"] == W.found(dup) + (0,) and g["count"] == n_prior and g["changed"] == 1
        assert brd == b"".join(board) and count == len(board)
        assert distinct == len(set(board)) == got[-1]["used"] and equal_entries == len(board) - len(set(board)) >= 4


def test_append_one_entry_short_leaves_index_and_board_alone(check, sequence, tmp_path):
    start, batches, want, board = sequence
    _write_sequence(tmp_path / "short.txt", start, batches, len(board) - 1)
    got, (count, _, _), brd = _batches(check("seq", tmp_path / "short.txt", 5, 2))
    before = len(board) - len(want[3][2])
    assert [g["found"][2] for g in got] == [0, 0, 0, 1] and got[3]["count"] == before == count
    assert got[3]["changed"] == 0 and got[3]["used"] == got[2]["used"]          # not a byte of the index (compared inside the program)
    assert got[3]["dup"] == want[3][0] and got[3]["found"][:2] == W.found(want[3][0])          # the verdicts do not depend on the board's room
    assert brd == b"".join(board[:before]) + b"\xee" * (64 * (len(board) - 1 - before))


def test_read_only_calls_leave_the_index_alone(check, sequence, tmp_path):
    """without a count pointer nothing is appended: every batch is judged against the start board alone, and the index stays as built"""
    start, batches, _, board = sequence
    _write_sequence(tmp_path / "ro.txt", start, batches, len(board), append=[0, 0, 0, 0])
    got, (count, distinct, _), brd = _batches(check("seq", tmp_path / "ro.txt", 9, 4))
    for t, g in enumerate(got):
        dup, out, _ = W.weed(batches[t][0], batches[t][1], start)
        assert g["dup"] == dup and g["out"] == out and g["found"] == W.found(dup) + (0,)
        assert g["count"] == len(start) and g["changed"] == 0 and g["used"] == len(start)
    assert count == distinct == len(start) and brd == b"".join(start) + b"\xee" * (64 * (len(board) - len(start)))


def test_rejected_ballots_are_never_read(check, tmp_path):
    """the bytes of ballots with a non-zero status word are poisoned in the host build (reading one aborts the program); the sequence
    above carries two poisoned ballots per batch through every run.  With every ballot rejected nothing is entered anywhere"""
    ballots, board = W.planted(3, 40, K, 2)
    _write_sequence(tmp_path / "none.txt", board, [(ballots, [5] * 40)], 2 + 40 * K)
    got, (count, distinct, _), _ = _batches(check("seq", tmp_path / "none.txt", 1, 0))
    assert got[0]["dup"] == [W.DUP_NONE] * 40 and got[0]["out"] == [5] * 40 and got[0]["found"] == (0, 0, 0)
    assert got[0]["count"] == 2 == count == distinct and got[0]["changed"] == 0


@pytest.mark.parametrize("slots", [8, 16])
def test_small_indexes_wrap_around_and_report_overflow(check, slots):
    """filled to exactly half (the library's load) with chains that start in the last two slots and wrap around the end; equal bytes take
    no second slot; filled up; one key more: the lane reports and terminates"""
    for seed in range(6):
        assert f"SMALL slots {slots} half {slots // 2} over 1\n" in check("small", slots, seed)


def test_a_garbage_index_terminates_quietly(check):
    for seed in (1, 2, 3):
        out = check("garbage", seed)
        assert out.count("GARBAGE round") == 4


def test_layout_against_a_direct_count_and_without_the_board(check):
    lib = eg._load()
    assert len(lib.eg_choice_weed_indexed_scratch_bytes.argtypes) == 2          # (params, n): there is no n_prior to depend on
    up = lambda x: -(-x // 256) * 256
    for n, k in ((1, 1), (100, 5), (1024, 5), (1025, 2), (103, 5), (1 << 16, 5), (1 << 20, 5), ((1 << 30) // 150, 150)):
        m = re.search(r"LAYOUT slots (\d+) tiles (\d+) table (\d+) pos (\d+) tile_sums (\d+) total_word (\d+) total (\d+)", check("layout", n, k))
        slots, tiles, table, pos, tile_sums, total_word, total = map(int, m.groups())
        assert slots & (slots - 1) == 0 and slots >= max(1024, 2 * n * k) and (slots == 1024 or slots // 2 < 2 * n * k)
        assert tiles == -(-n // 1024)
        assert (table, pos, tile_sums, total_word, total) == (0, up(8 * slots), up(8 * slots) + up(4 * n), up(8 * slots) + up(4 * n) + up(4 * tiles),
                                                             up(8 * slots) + up(4 * n) + up(4 * tiles) + 256)
    assert "total 0" in check("layout", 0, 5)
    # 2^16 five-option ballots: 8.7 MB beside any board (the stateless pass: 134.5 MB beside 5 x 10^6 entries)
    assert "total 8651264" in check("layout", 1 << 16, 5)
    host = (CSRC / "weed_index_host.hpp").read_text()
    assert "inline Layout layout_indexed(size_t n, uint32_t keys_per_ballot) { return layout(n, 0, keys_per_ballot); }" in host
    for cap in (0, 512, 513, 5_000_000):
        assert f"BYTES {lib.eg_weed_index_bytes(cap)}\n" in check("bytes", cap)
    assert "BYTES 0\n" in check("bytes", 1 << 31)
