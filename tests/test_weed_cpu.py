"""Ballot weeding (eg_*_weed*, csrc/weed_kernels.cuh, csrc/weed_host.hpp) without a GPU.

* The six entry points are declared, exported, bound in Python and mirrored in C++; the constants agree; ABI version 7.
* tests/hostcheck/weedcheck.cpp: weed_host.hpp and the lane functions of the kernels under ASan + UBSan, serially.  Expected values come
  from the model of the rule in tests/weed_ref.py (a dict from key bytes to the earliest owner): planted copies of every kind, 20 lane
  orders and 5 seeds, tables filled to capacity and one slot too small, poisoned bytes of ballots that do not participate, the append
  at the exact fit and one entry short, the layout, 64-bit addresses, the adjacency of R and B items.
* The refusals of both entry forms that need no GPU."""
import ctypes as C
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
SIZES = ("eg_choice_weed_scratch_bytes", "eg_qv_weed_scratch_bytes")
DEVICE = ("eg_choice_weed_device", "eg_qv_weed_device")
HOST = ("eg_choice_weed", "eg_qv_weed")
BAD_ARG = -3


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for names, ret, restype, nargs in ((SIZES, "size_t", C.c_size_t, 3), (DEVICE, "int", C.c_int, 14), (HOST, "int", C.c_int, 10)):
        for name in names:
            assert re.search(rf"^{ret} {name}\(", header, re.M), name
            assert name in eg.exported_symbols()
            assert hasattr(raw, name), f"{name} is not exported"
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == nargs, name
    # a section of its own, behind the weighted tally and in front of the multi-GPU tier
    at = header.index("eg_choice_weed_scratch_bytes(")
    assert header.index("int eg_qv_tally_weighted(") < at < header.index("int eg_verify_choice_batch_multi(")
    # the header documents the rule
    for phrase in ("NOT sequential", "EG_DUP_PRIOR if any key of b is on the", "hash_seed", "found[2]"):
        assert phrase in header, phrase


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    assert int(re.search(r"#define EG_DUP_NONE\s+0x([0-9a-f]+)u", header).group(1), 16) == eg.DUP_NONE == W.DUP_NONE == 0xFFFFFFFF
    assert int(re.search(r"#define EG_DUP_PRIOR\s+0x([0-9a-f]+)u", header).group(1), 16) == eg.DUP_PRIOR == W.DUP_PRIOR == 0xFFFFFFFE
    assert re.search(r"#define EG_WEED_KEYS_MAX\s+\(1u << 30\)", header) and eg.WEED_KEYS_MAX == 1 << 30
    assert int(re.search(r"EG_ST_DUPLICATE = (\d+)", header).group(1)) == eg.ST_DUPLICATE == W.ST_DUPLICATE == 14
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7
    host = (CSRC / "weed_host.hpp").read_text()
    assert "DUP_NONE = 0xffffffffu" in host and "DUP_PRIOR = 0xfffffffeu" in host and "ST_DUPLICATE = 14" in host and "KEYS_MAX = 1ull << 30" in host


def test_python_and_cpp_mirrors_exist(tmp_path):
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        assert callable(cls.weed) and callable(cls.weed_device) and callable(cls.weed_scratch_bytes)
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count("Weeded weed(") == 2 and hpp.count("void weed_device(") == 2
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        template <class P> Weeded host(const P& p) { return p.weed(Bytes(), {}, Bytes(), true); }
        template <class P> void dev(const P& p) {
          p.weed_device(0, nullptr, nullptr, 0, nullptr, 0, 1234567, nullptr, nullptr, nullptr, nullptr, nullptr);
          p.weed_device(0, nullptr, nullptr, 0, nullptr, 0, 1234567, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
          (void)p.weed_scratch_bytes(0, 3);
        }
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element pk{};
            ChoiceParams c = ChoiceParams::single(ctx, pk, 5);
            QuadraticVotingParams q(ctx, pk, 5, 20);
            Weeded a = host(c), b = host(q);
            dev(c); dev(q);
            return (int)(a.dropped() + b.appended.size());
          }
          static_assert(EG_DUP_NONE == 0xffffffffu && EG_DUP_PRIOR == 0xfffffffeu && EG_ST_DUPLICATE == 14 && EG_WEED_KEYS_MAX == (1u << 30),
                        "header constants");
          return 0;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_DUP_PRIOR == 0xfffffffeu && EG_ST_DUPLICATE == 14 && eg_choice_weed && '
                   'eg_qv_weed_device && eg_qv_weed_scratch_bytes ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_no_waiting_between_workgroups():
    for f in ("weed_kernels.cuh", "weed_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    kernels = (CSRC / "weed_kernels.cuh").read_text()
    device = kernels[kernels.index("#if defined(__HIPCC__)"):]
    # bounded loops only, the kernel boundary is the only synchronisation
    assert not re.search(r"\bwhile\b", device) and "__threadfence" not in device and "__builtin_amdgcn_fence" not in device
    assert "__host__ __device__" in (CSRC / "weed_host.hpp").read_text()


# ------------------------------------------------------------------ refusals that need no GPU
def test_refusals_of_the_host_and_device_entries_without_a_gpu():
    """the argument checks come before any device work and before the params object is looked at; what passes them fails on the missing
    params object; the scratch size of a refused call is 0"""
    lib = eg._load()
    buf = C.create_string_buffer(256)            # 16-byte aligned below
    base = (C.addressof(buf) + 15) & ~15
    one = (C.c_uint32 * 4)()

    def device(fn, n=1, ballots=base, status=None, n_prior=0, board=base, cap=8, scratch=base, dup=one, out=None, count=None, found=one):
        rc = fn(None, n, ballots, status, n_prior, board, cap, 99, scratch, dup, out, count, found, None)
        return rc, lib.eg_last_error()

    def host(fn, n=1, ballots=base, status=None, n_prior=0, board=base, dup=one, out=None, appended=None):
        n_app = C.c_size_t(7)
        rc = fn(None, n, ballots, status, n_prior, board, dup, out, appended, C.byref(n_app))
        assert n_app.value == 0
        return rc, lib.eg_last_error()

    for name in DEVICE + HOST:
        fn = getattr(lib, name)
        call = (lambda **kw: device(fn, **kw)) if name in DEVICE else (lambda **kw: host(fn, **kw))
        for n in (1 << 31, 1 << 40):
            rc, msg = call(n=n)
            assert rc == BAD_ARG and b"n is 2^31 or more" in msg, (name, n)
        rc, msg = call(n_prior=1 << 31, **({"cap": 1 << 32} if name in DEVICE else {}))
        assert rc == BAD_ARG and b"n_prior is 2^31 or more" in msg, name
        for kw, text in (({"ballots": None}, b"null ballots"), ({"dup": None}, b"null dup_of"), ({"n_prior": 3, "board": None}, b"null board with n_prior")):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and text in msg, (name, kw, msg)
        # what is within the limits fails on the missing params object: the limits themselves are not over the limit
        for kw in ({}, {"n": (1 << 31) - 1}, {"n": 0, "ballots": None, "dup": None}, {"n_prior": 5}):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and b"null params" in msg, (name, kw, msg)
    for name in DEVICE:
        fn = getattr(lib, name)
        rc, msg = device(fn, n_prior=9, cap=8)
        assert rc == BAD_ARG and b"n_prior is above board_cap" in msg
        rc, msg = device(fn, found=None)
        assert rc == BAD_ARG and b"null found" in msg
        rc, msg = device(fn, board=None, count=one)
        assert rc == BAD_ARG and b"null board with an append requested" in msg
        for kw in ({"ballots": base + 8}, {"board": base + 4}, {"scratch": base + 1}):
            rc, msg = device(fn, **kw)
            assert rc == BAD_ARG and b"16-byte aligned" in msg, kw
        rc, msg = device(fn, dup=C.addressof(one) + 2)
        assert rc == BAD_ARG and b"misaligned" in msg
    for name in SIZES:
        fn = getattr(lib, name)
        for n, n_prior in ((1 << 31, 0), (1, 1 << 31), (100, 7), (0, 0)):
            assert fn(None, n, n_prior) == 0, (name, n, n_prior)


def test_missing_gpu_is_loud():
    for cls, prefix in ((eg.ChoiceParams, "choice"), (eg.QuadraticVotingParams, "qv")):
        p = object.__new__(cls)              # what a caller would hold if a params object could exist without a GPU: no handle
        p._h, p._prefix, p.ballot_size, p.n_options = None, prefix, 736, 5
        with pytest.raises(eg.EgError, match="null params"):
            p.weed(bytes(736))
        with pytest.raises(eg.EgError, match="null params"):
            p.weed(bytes(736), [0], bytes(128), append=True)
        with pytest.raises(eg.EgError, match="null params"):
            p.weed_device(1, 16, 0, 0, 0, 0, 5, 16, 16, 16)
        with pytest.raises(ValueError):
            p.weed(bytes(736), [0, 0])
        with pytest.raises(ValueError):
            p.weed(bytes(736), None, bytes(65))
        assert p.weed_scratch_bytes(100, 3) == 0


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "weedcheck", HERE / "weedcheck.cpp"
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


def _write_case(path, ballots, status, board, board_cap):
    k = len(ballots[0]) if ballots else 1
    lines = [f"{len(ballots)} {k} {len(board)} {board_cap}"] + [e.hex() for e in board]
    for b, keys in enumerate(ballots):
        lines.append(f"{0 if status is None else status[b]} {b''.join(keys).hex()}")
    path.write_text("\n".join(lines) + "\n")


def _report(out):
    dup = [int(x) for x in re.search(r"^DUP :(.*)$", out, re.M).group(1).split()]
    st = [int(x) for x in re.search(r"^STATUS :(.*)$", out, re.M).group(1).split()]
    found = tuple(int(x) for x in re.search(r"^FOUND (\d+) (\d+) (\d+)$", out, re.M).groups())
    count = int(re.search(r"^COUNT (\d+)$", out, re.M).group(1))
    board = bytes.fromhex(re.search(r"^BOARD ([0-9a-f]*)$", out, re.M).group(1))
    slots, used = (int(x) for x in re.search(r"^SLOTS (\d+) USED (\d+)$", out, re.M).groups())
    return dup, st, found, count, board, slots, used


@pytest.fixture(scope="module")
def planted():
    """200 ballots of 3 keys and a board of 9 with every kind of copy planted; six ballots rejected - among them the original of a
    whole copy, so that the copy owns the keys, and one copy, which stays EG_DUP_NONE"""
    ballots, board = W.planted(15, 200, 3, 9)
    status = [0] * 200
    for b in (4, 49, 58, 94, 139, 184):
        status[b] = 6 + 256 * b
    ballots[50] = list(ballots[49])          # 49 is rejected: 50 is not a duplicate ...
    ballots[60] = list(ballots[50])          # ... and owns the keys: 60 is a copy of 50
    ballots[58] = list(ballots[10])          # 58 is rejected: a rejected copy is left alone
    assert status[49] and status[58] and not status[50] and not status[60]
    return ballots, status, board


def test_model_on_the_planted_copies(planted):
    """the model itself, on the cases named by the rule"""
    ballots, status, board = planted
    dup, out, appended = W.weed(ballots, status, board)
    assert dup[7] == 2 and dup[199] == 0 and dup[11] == 5 and dup[33] == 2                    # whole copies, one key, a copy of a copy
    assert (dup[20], dup[21], dup[22], dup[23]) == (W.DUP_NONE, 20, 21, 22)                   # the chain: flagged ballots still own keys
    assert dup[30] == W.DUP_NONE                                                             # a key twice inside one ballot
    assert dup[3] == dup[35] == dup[36] == W.DUP_PRIOR                                       # the board wins over the batch
    assert dup[50] == W.DUP_NONE and dup[60] == 50 and dup[58] == W.DUP_NONE and out[58] == status[58]
    assert out[7] == W.ST_DUPLICATE and W.found(dup) == (3, 8)
    assert len(appended) == 3 * (200 - 6 - 11)
    # without the status words the rejected original owns its keys again
    dup_all, _, _ = W.weed(ballots, None, board)
    assert dup_all[50] == 49 and dup_all[60] == 49 and dup_all[58] == 10


def test_lane_functions_equal_the_model_in_any_order_and_under_any_seed(check, planted, tmp_path):
    """20 shuffled lane orders and 5 seeds (0 included): identical dup_of, status_out, counters and appended bytes every time"""
    ballots, status, board = planted
    want_dup, want_out, want_app = W.weed(ballots, status, board)
    cap = len(board) + len(want_app)
    _write_case(tmp_path / "case.txt", ballots, status, board, cap)
    runs = [(0, 0)] + [(0, order) for order in range(1, 21)] + [(seed, 3) for seed in (1, 2, 0xDEADBEEFCAFEF00D, (1 << 64) - 1)] + [(0, 7)]
    for seed, order in runs:
        dup, out, found, count, brd, slots, used = _report(check("run", tmp_path / "case.txt", 0, seed, order))
        assert dup == want_dup and out == want_out, (seed, order)
        assert found == W.found(want_dup) + (0,) and count == cap
        assert brd == b"".join(board) + b"".join(want_app)
        # 609 keys: the smallest power of two >= 1218
        assert slots == 2048 and used == len(set(board) | {k for b, keys in enumerate(ballots) if not status[b] for k in keys})


def test_rejected_ballots_are_never_read(check, tmp_path):
    """the bytes of ballots with a non-zero status word are poisoned in the host build (reading one aborts the program): with every ballot
    rejected only the board is read; the planted case above carries six poisoned ballots through every run"""
    ballots, board = W.planted(3, 40, 2, 2)
    _write_case(tmp_path / "none.txt", ballots, [5] * 40, board, 2)
    dup, out, found, count, _, _, used = _report(check("run", tmp_path / "none.txt", 0, 1, 0))
    assert dup == [W.DUP_NONE] * 40 and out == [5] * 40 and found == (0, 0, 0) and count == 2 and used == 2


@pytest.mark.parametrize("slots", [8, 16])
def test_tables_filled_to_capacity_wrap_around(check, tmp_path, slots):
    """as many distinct keys as slots (a load of 1.0): chains run over the end of the table and every key still finds its owner"""
    rng = random.Random(slots)
    key = lambda: bytes(rng.getrandbits(8) for _ in range(64))
    board = [key() for _ in range(2)]
    distinct = [key() for _ in range(slots - 2)]
    ballots = [distinct[2 * i:2 * i + 2] for i in range((slots - 2) // 2)]
    ballots += [[distinct[1], distinct[-1]], [board[1], distinct[0]], list(ballots[1])]
    want = W.weed(ballots, None, board)
    _write_case(tmp_path / "full.txt", ballots, None, board, 2 + 2 * len(ballots))
    for seed in range(6):
        dup, out, found, count, brd, got_slots, used = _report(check("run", tmp_path / "full.txt", slots, seed, seed))
        assert got_slots == used == slots
        assert (dup, out) == want[:2] and found[2] == 0 and brd[:64 * count] == b"".join(board) + b"".join(want[2])


def test_a_table_one_slot_too_small_reports_overflow_and_terminates(check, tmp_path):
    rng = random.Random(9)
    ballots = [[bytes(rng.getrandbits(8) for _ in range(64)) for _ in range(3)] for _ in range(3)]          # 9 distinct keys, 8 slots
    _write_case(tmp_path / "over.txt", ballots, None, [], 9)
    for seed in range(4):
        dup, out, found, count, _, slots, used = _report(check("run", tmp_path / "over.txt", 8, seed, 0))
        assert slots == used == 8 and found[2] >= 1


def test_append_at_the_exact_fit_and_one_entry_short(check, planted, tmp_path):
    ballots, status, board = planted
    _, _, want_app = W.weed(ballots, status, board)
    fit = len(board) + len(want_app)
    _write_case(tmp_path / "short.txt", ballots, status, board, fit - 1)
    dup, out, found, count, brd, _, _ = _report(check("run", tmp_path / "short.txt", 0, 5, 2))
    assert found[2] == 1 and count == len(board)
    assert brd == b"".join(board) + b"\xee" * (64 * (fit - 1 - len(board)))          # nothing was appended
    assert dup == W.weed(ballots, status, board)[0]                                    # the verdicts do not depend on the board's room


def test_layout_against_a_direct_count(check):
    for n, n_prior, k in ((1, 0, 1), (100, 7, 5), (1024, 0, 5), (1025, 3000, 2), (103, 0, 5), (1 << 20, 5_000_000, 5), ((1 << 30) // 150, 0, 150)):
        m = re.search(r"LAYOUT slots (\d+) tiles (\d+) table (\d+) pos (\d+) tile_sums (\d+) total_word (\d+) total (\d+)", check("layout", n, n_prior, k))
        slots, tiles, table, pos, tile_sums, total_word, total = map(int, m.groups())
        keys = n * k + n_prior
        assert slots & (slots - 1) == 0 and slots >= max(1024, 2 * keys) and (slots == 1024 or slots // 2 < 2 * keys)
        assert tiles == -(-n // 1024)
        up = lambda x: -(-x // 256) * 256
        assert (table, pos, tile_sums, total_word, total) == (0, up(8 * slots), up(8 * slots) + up(4 * n), up(8 * slots) + up(4 * n) + up(4 * tiles),
                                                             up(8 * slots) + up(4 * n) + up(4 * tiles) + 256)
    assert "total 0" in check("layout", 0, 77, 5)                                      # n == 0 needs no scratch


def test_addresses_are_64_bit(check):
    b, stride = (1 << 31) - 2, 256 * 1024
    assert f"ADDR {b * stride + 32 * 7}\n" in check("addr", b, stride, 7)
    assert b * stride > 1 << 48
    kernels = (CSRC / "weed_kernels.cuh").read_text()
    assert "egw::key_offset(b, stride," in kernels and "uint64_t stride, n, n_prior;" in kernels


def test_argument_rules(check):
    assert "REFUSE n is 2^31 or more" in check("refuse", 1 << 31, 0, 0, 5)
    assert "REFUSE n_prior is 2^31 or more" in check("refuse", 1, 1 << 31, 1 << 32, 5)
    assert "REFUSE n_prior is above board_cap" in check("refuse", 1, 9, 8, 5)
    assert "EG_WEED_KEYS_MAX" in check("refuse", (1 << 30) // 5 + 1, 0, 0, 5)
    assert "EG_WEED_KEYS_MAX" in check("refuse", (1 << 30) // 5, 5, 5, 5)
    assert "REFUSE -" in check("refuse", (1 << 30) // 5, 4, 4, 5)
    assert "REFUSE -" in check("refuse", 0, 0, 0, 5)


def test_r_and_b_items_are_adjacent_in_six_election_shapes(check, oracle):
    """the 64 bytes from the R item of every tally ciphertext are the oracle's tally of one accepted ballot"""
    pk = oracle.keypair_from_seed(12345)[1]
    shapes = {"single2": oracle.ChoiceParams(pk, 2, True), "single5": oracle.ChoiceParams(pk, 5, True),
              "single150": oracle.ChoiceParams(pk, 150, True), "multi16": oracle.ChoiceParams(pk, 16, False),
              "qv5_20": oracle.QvParams(pk, 5, 20), "qv3_10000": oracle.QvParams(pk, 3, 10000)}
    seen = set()
    for line in check("items").splitlines():
        if not line.startswith("ITEMS"):
            continue
        name, stride, adjacent = line.split()[1], int(line.split()[3]), int(line.split()[5])
        r_items = [int(x) for x in line.split(":")[1].split()]
        op = shapes[name]
        assert adjacent == 1 and stride == op.ballot_size and stride % 16 == 0 and len(r_items) == op.n_options
        ballot = op.generate_batch(777, 0, 1, 3) if name == "multi16" else op.generate_batch(777, 0, 1)
        assert b"".join(W.keys_of(ballot, stride, r_items)[0]) == op.tally(ballot, [0]), name
        seen.add(name)
    assert seen == set(shapes)
