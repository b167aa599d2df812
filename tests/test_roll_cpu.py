"""The voter-roll pass (eg_roll_*) without a GPU:
* the surface: the five symbols declared, exported, bound and in INTEGRATION.md; the constants in the header, the Python mirror,
  roll_host.hpp and the model; ABI version 7; the C++ mirror; plain C99; no environment knob and no waiting loop in the device code;
* self-checks of the model tests/roll_ref.py (the words, commutativity, idempotence), from which every expected value comes;
* tests/hostcheck/rollcheck.cpp: roll_host.hpp and the lane functions of roll_kernels.cuh under ASan + UBSan, run serially in shuffled
  lane orders over a batch with re-votes of every kind, poisoned inputs of ballots that do not participate, aliased status words;
* every refusal of the four entries that needs no GPU, and merge_rolls over gloo at world size 2."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import roll_ref as R

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
BAD_ARG = -3
POLICIES = (R.ROLL_LAST, R.ROLL_FIRST)
ENTRIES = {  # name: (return type in the header, restype, number of arguments)
    "eg_roll_cast_scratch_bytes": ("size_t", C.c_size_t, 3),
    "eg_roll_cast_device": ("int", C.c_int, 20),
    "eg_roll_cast": ("int", C.c_int, 17),
    "eg_roll_check_device": ("int", C.c_int, 16),
    "eg_roll_check": ("int", C.c_int, 15),
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
    # a section of its own, behind the voter signatures and in front of the multi-GPU tier
    at = header.index("eg_roll_cast_scratch_bytes(const")
    assert header.index("int eg_sha512_batch_device(") < at < header.index("int eg_verify_choice_batch_multi(")
    for phrase in ("THE LARGER WORD WINS", "ORDER IN THE CHAIN", "signatures -> verify -> weed -> roll -> tally", "MERGE by the element-wise maximum",
                   "MULTI-GPU RECIPE", "commutative and idempotent", "never used as an index", "EG_ROLL_WORD(seq, policy)"):
        assert phrase in header, phrase
    for m in ("cast", "check", "cast_device", "check_device", "cast_scratch_bytes", "word", "seq"):
        assert callable(getattr(eg.VoterRoll, m)), m
    assert "VoterRoll" in eg.__all__
    ffi = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name
    from elastic_elgamal_amd import distributed as egd
    assert callable(egd.merge_rolls)


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    host = (CSRC / "roll_host.hpp").read_text()
    assert int(re.search(r"EG_ST_SUPERSEDED = (\d+)", header).group(1)) == eg.ST_SUPERSEDED == eg.VoterRoll.ST_SUPERSEDED == R.ST_SUPERSEDED == 16
    assert "ST_SUPERSEDED = 16;" in host
    assert eg.STATUS_NAMES[16] == "Superseded" and eg.STATUS_NAMES[15] == "BadSignature" and eg.STATUS_NAMES[14] == "Duplicate"
    for name, model in (("FIRST", R.ROLL_FIRST), ("LAST", R.ROLL_LAST), ("SUPERSEDED", R.SUPERSEDED), ("OFF_ROLL", R.OFF_ROLL), ("NOT_CAST", R.NOT_CAST)):
        value = int(re.search(rf"EG_ROLL_{name} = (\d+)", header).group(1))
        assert value == getattr(eg, "ROLL_" + name) == getattr(eg.VoterRoll, "ROLL_" + name) == model, name
        assert re.search(rf"\bROLL_{name} = {value};", host), name
    assert R.ROLL_FIRST != R.ROLL_LAST and 0 not in POLICIES
    assert re.search(r"#define EG_SEQ_NONE \(~\(uint64_t\)0\)", header) and eg.SEQ_NONE == eg.VoterRoll.SEQ_NONE == R.SEQ_NONE == (1 << 64) - 1
    assert "SEQ_NONE = ~0ull;" in host
    assert re.search(r"#define EG_ROLL_KEYS_MAX \(1u << 31\)", header) and eg.ROLL_KEYS_MAX == eg.VoterRoll.ROLL_KEYS_MAX == R.KEYS_MAX == 1 << 31
    assert "KEYS_MAX = 1ull << 31;" in host and "GROUP_NONE = 0xffffffffu;" in host and eg.GROUP_NONE == R.GROUP_NONE
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7


def test_cpp_mirror_compiles_and_the_macros_agree_with_the_model(tmp_path):
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    top = (1 << 63) - 2
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            VoterRoll roll{ctx, EG_ROLL_LAST};
            std::vector<uint64_t> words(4);
            RollVerdicts a = roll.cast({1, 0, 1}, words, 7, {0, 0, 0}, {5, 6, 7, 8}, {1, 1, 2, 2});
            RollVerdicts b = roll.check({1, 0, 1}, words, 7);
            roll.cast_device(0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, roll.cast_scratch_bytes(0, 4));
            roll.check_device(0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            return (int)(a.displaced.size() + b.superseded_by.size() + a.found[0] + roll.word(3) + roll.seq(4));
          }
          static_assert(EG_ST_SUPERSEDED == 16 && EG_ROLL_FIRST == FIRST_V && EG_ROLL_LAST == LAST_V && EG_ROLL_SUPERSEDED == 1 &&
                        EG_ROLL_OFF_ROLL == 2 && EG_ROLL_NOT_CAST == 3 && EG_SEQ_NONE == 0xffffffffffffffffull && EG_ROLL_KEYS_MAX == (1u << 31),
                        "header constants");
          static_assert(EG_ROLL_WORD(0, EG_ROLL_LAST) == 1 && EG_ROLL_WORD(0, EG_ROLL_FIRST) == 0x7fffffffffffffffull &&
                        EG_ROLL_WORD(TOPull, EG_ROLL_LAST) == 0x7fffffffffffffffull && EG_ROLL_WORD(TOPull, EG_ROLL_FIRST) == 1 &&
                        EG_ROLL_SEQ(EG_ROLL_WORD(1, EG_ROLL_FIRST), EG_ROLL_FIRST) == 1 && EG_ROLL_SEQ(EG_ROLL_WORD(TOPull, EG_ROLL_LAST), EG_ROLL_LAST) == TOPull,
                        "the words");
          return 0;
        }
        """).replace("NS;", ns + ";").replace("FIRST_V", str(R.ROLL_FIRST)).replace("LAST_V", str(R.ROLL_LAST)).replace("TOP", str(top)))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_ST_SUPERSEDED == 16 && EG_ROLL_NOT_CAST == 3 && EG_ROLL_WORD(5, EG_ROLL_LAST) == 6 && '
                   'EG_ROLL_SEQ(6, EG_ROLL_LAST) == 5 && EG_SEQ_NONE > EG_ROLL_KEYS_MAX && eg_roll_cast_scratch_bytes && eg_roll_cast_device && '
                   'eg_roll_cast && eg_roll_check_device && eg_roll_check ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-address", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_no_waiting_between_lanes():
    for f in ("roll_kernels.cuh", "roll_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()
    kernels = (CSRC / "roll_kernels.cuh").read_text()
    device = kernels[kernels.index("#if defined(__HIPCC__)"):]
    # bounded loops only, the kernel boundary is the only synchronisation between workgroups, no compare-and-swap
    assert not re.search(r"\bwhile\b", device) and "__threadfence" not in device and "__builtin_amdgcn_fence" not in device
    assert "atomicCAS" not in kernels and "atomicMax" in device
    assert "__host__ __device__" in (CSRC / "roll_host.hpp").read_text()
    lib_src = (CSRC / "eg_hip.hip").read_text()
    assert '#include "roll_kernels.cuh"' in lib_src


# ------------------------------------------------------------------ the model checks itself
def test_model_words_round_trip_at_the_ends():
    for policy in POLICIES:
        for s in (0, 1, (1 << 63) - 2):
            w = R.word(s, policy)
            assert 1 <= w <= (1 << 63) - 1 and R.seq(w, policy) == s
    assert R.word(0, R.ROLL_LAST) == 1 and R.word(0, R.ROLL_FIRST) == (1 << 63) - 1 and R.word((1 << 63) - 2, R.ROLL_FIRST) == 1
    assert R.word(8, R.ROLL_LAST) > R.word(7, R.ROLL_LAST) and R.word(7, R.ROLL_FIRST) > R.word(8, R.ROLL_FIRST)
    lib = object.__new__(eg.VoterRoll)
    for policy in POLICIES:
        lib.policy = policy
        for s in (0, 1, 12345, (1 << 63) - 2):
            assert lib.word(s) == R.word(s, policy) and lib.seq(lib.word(s)) == s


def _three_batches():
    rng = random.Random(5)
    return [(base, [rng.randrange(12) for _ in range(n)], [0 if rng.random() < 0.8 else 6 for _ in range(n)]) for base, n in ((0, 30), (30, 25), (55, 40))]


def test_model_is_commutative_and_idempotent():
    batches = _three_batches()
    for policy in POLICIES:
        rolls = []
        for order in itertools.permutations(range(3)):
            roll = R.Roll(12, policy)
            for k in order:
                base, idx, st = batches[k]
                roll.cast(idx, base, st)
            rolls.append(roll.words())
        assert all(r == rolls[0] for r in rolls) and sum(w != 0 for w in rolls[0]) >= 10
        final = R.Roll(12, policy, rolls[0])
        kept = sum((final.kept(idx, base, st) != [] for base, idx, st in batches))
        assert kept >= 1
        for base, idx, st in batches:                                     # idempotence: nothing moves, nothing is displaced
            res = final.cast(idx, base, st)
            assert final.words() == rolls[0] and res["displaced"] == [] and res["found"][1] == 0
        # every voter with a counted ballot has exactly one kept ballot over all batches
        total = sum(len(final.kept(idx, base, st)) for base, idx, st in batches)
        assert total == sum(w != 0 for w in rolls[0])
        # merging the rolls of the single batches is casting them all
        parts = []
        for base, idx, st in batches:
            roll = R.Roll(12, policy)
            roll.cast(idx, base, st)
            parts.append(roll.words())
        assert R.merge(R.merge(parts[0], parts[1]), parts[2]) == rolls[0]


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "rollcheck", HERE / "rollcheck.cpp"
    deps = [src, CSRC / "roll_kernels.cuh", CSRC / "roll_host.hpp"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args, ok=True):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        if ok:
            assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout if ok else r

    return run


def write_case(path, key_index, status, roll, seq_base, policy, groups=None, weights=None, displaced=True):
    n_keys = len(roll)
    lines = [f"{len(key_index)} {n_keys} {seq_base} {policy} {int(groups is not None)} {int(weights is not None)} {int(displaced)}"]
    lines += [f"{roll[v]} {groups[v] if groups else 0} {weights[v] if weights else 0}" for v in range(n_keys)]
    lines += [f"{s} {v}" for s, v in zip(status, key_index)]
    path.write_text("\n".join(lines) + "\n")
    return path


def parse(out):
    rows = {}
    for line in out.splitlines():
        name, _, rest = line.partition(" ")
        rows[name] = [int(x) for x in rest.replace(":", " ").split()] if name in ("BY", "STATUS", "GROUPS", "WEIGHTS", "FOUND", "ROLL", "DISPLACED") else rest
    if "DISPLACED" in rows:
        d = rows["DISPLACED"]
        rows["DISPLACED"] = list(zip(d[0::2], d[1::2]))
    return rows


def planted(policy, n_keys=40, n=200, seq_base=1000):
    """200 ballots over 40 keys with re-votes of every kind.  Voters 0-3 are kept out of the random draw: 1 gets exactly two ballots, 2 five,
    3 one and 0 none.  Prior words: voter 5 at sequence 10 (below the batch: it wins under FIRST and loses under LAST), voter 6 at 5000
    (above the batch, a batch cast "out of order": the reverse), voter 7 at 3 and voter 0 at 77 (0 has no ballot here: untouched), voter 3
    at 20.  Status words: every ninth ballot is rejected and its key_index poisoned; off-roll indices n_keys, n_keys + 1 and 0xffffffff on
    accepted ballots and, behind the poison, on rejected ones."""
    rng = random.Random(1234 + policy)
    idx = [rng.randrange(4, n_keys) for _ in range(n)]
    for b in (17, 150):
        idx[b] = 1
    for b in (0, 63, 64, 128, 199):
        idx[b] = 2
    idx[100] = 3
    status = [0] * n
    for b in range(4, n, 9):
        status[b] = 6 | (b << 8)
        idx[b] = (n_keys + 5, 0xFFFFFFFF, 2, 1)[b % 4]                    # never read
    for b, v in ((33, n_keys), (34, n_keys + 1), (35, 0xFFFFFFFF)):
        assert status[b] == 0
        idx[b] = v
    roll = [0] * n_keys
    for v, s in ((5, 10), (6, 5000), (7, 3), (0, 77), (3, 20)):
        roll[v] = R.word(s, policy)
    assert {5, 6, 7} <= {v for b, v in enumerate(idx) if status[b] == 0}
    groups = [100 + v % 7 for v in range(n_keys)]
    weights = [(1 << 40) * (v % 3) + v for v in range(n_keys)]
    return idx, status, roll, seq_base, groups, weights


@pytest.mark.parametrize("policy", POLICIES)
def test_lane_functions_equal_the_model_in_any_order(check, tmp_path, policy):
    idx, status, roll, seq_base, groups, weights = planted(policy)
    model = R.Roll(len(roll), policy, roll)
    want = model.cast(idx, seq_base, status, groups, weights)
    # the planted re-votes did what they were planted for
    last = policy == R.ROLL_LAST
    assert want["status_out"][17] == (R.status_word(R.SUPERSEDED) if last else 0) and want["status_out"][150] == (0 if last else R.status_word(R.SUPERSEDED))
    assert [want["status_out"][b] == 0 for b in (0, 63, 64, 128, 199)] == ([False] * 4 + [True] if last else [True] + [False] * 4)
    assert want["superseded_by"][63] == seq_base + (199 if last else 0)
    assert (model.best[5][1] == 10) == (not last) and (model.best[6][1] == 5000) == last and model.best[0][1] == 77
    assert (want["status_out"][100] == 0) == last and want["superseded_by"][100] == (R.SEQ_NONE if last else 20)
    assert [want["status_out"][b] for b in (33, 34, 35)] == [R.status_word(R.OFF_ROLL)] * 3 and want["found"][2] == 3
    assert want["found"][0] > 50 and len(want["displaced"]) == (3 if last else 1) and ((20, seq_base + 100) in want["displaced"]) == last
    path = write_case(tmp_path / "case.txt", idx, status, roll, seq_base, policy, groups, weights)
    for order, alias in [(0, 0), (0, 1)] + [(o, o % 2) for o in range(1, 21)]:
        got = parse(check("cast", path, order, alias))
        assert got["BY"] == want["superseded_by"] and got["STATUS"] == want["status_out"], (order, alias)
        assert got["GROUPS"] == want["groups_out"] and got["WEIGHTS"] == want["weights_out"], (order, alias)
        assert got["FOUND"] == want["found"] and got["ROLL"] == model.words() and got["DISPLACED"] == want["displaced"], (order, alias)
    # cast again over the new roll: nothing moves; the check entry says the same as the cast
    again = write_case(tmp_path / "again.txt", idx, status, model.words(), seq_base, policy, groups, weights)
    got = parse(check("cast", again, 3, 1))
    assert got["ROLL"] == model.words() and got["DISPLACED"] == [] and got["FOUND"][1] == 0 and got["STATUS"] == want["status_out"]
    verdicts = model.check(idx, seq_base, status, groups, weights)
    for order, alias in ((0, 0), (5, 1)):
        got = parse(check("check", again, order, alias))
        assert got["BY"] == verdicts["superseded_by"] == want["superseded_by"] and got["STATUS"] == verdicts["status_out"]
        assert got["GROUPS"] == verdicts["groups_out"] and got["WEIGHTS"] == verdicts["weights_out"] and got["FOUND"] == verdicts["found"]
        assert got["ROLL"] == model.words()
    # the check against an empty roll and against another batch's roll: NOT_CAST, and nobody is kept
    empty = write_case(tmp_path / "empty.txt", idx, status, [0] * len(roll), seq_base, policy)
    got, none = parse(check("check", empty, 0, 0)), R.Roll(len(roll), policy).check(idx, seq_base, status)
    assert got["STATUS"] == none["status_out"] and got["FOUND"] == none["found"] and none["found"][1] == sum(s == 0 for s in status) - 3
    assert "GROUPS" not in got and "WEIGHTS" not in got


@pytest.mark.parametrize("policy", POLICIES)
def test_lane_functions_without_optional_arrays_one_key_and_the_sequence_limit(check, tmp_path, policy):
    # no roster arrays, no displaced: the roll and the verdicts are the same
    idx, status, roll, seq_base, _, _ = planted(policy)
    model = R.Roll(len(roll), policy, roll)
    want = model.cast(idx, seq_base, status)
    got = parse(check("cast", write_case(tmp_path / "bare.txt", idx, status, roll, seq_base, policy, displaced=False), 9, 0))
    assert got["STATUS"] == want["status_out"] and got["BY"] == want["superseded_by"] and got["ROLL"] == model.words() and got["FOUND"] == want["found"]
    assert "DISPLACED" not in got and "GROUPS" not in got
    # n_keys == 1: 70 ballots of one voter and two off the roll
    idx = [0] * 70
    idx[11], idx[12] = 1, 0xFFFFFFFF
    for prior in (0, R.word(5, policy), R.word(10 ** 6, policy)):
        model = R.Roll(1, policy, [prior])
        want = model.cast(idx, 100, None, [9], [3])
        got = parse(check("cast", write_case(tmp_path / "one.txt", idx, [0] * 70, [prior], 100, policy, [9], [3]), 4, 1))
        assert got["STATUS"] == want["status_out"] and got["BY"] == want["superseded_by"] and got["ROLL"] == model.words()
        assert got["FOUND"] == want["found"] and got["DISPLACED"] == want["displaced"] and got["WEIGHTS"] == want["weights_out"]
        assert sum(s == 0 for s in got["STATUS"]) == (1 if model.best[0][1] >= 100 and model.best[0][1] < 170 else 0)
    # seq_base + n at the limit: the last sequence number is 2^63 - 2
    n, top = 9, (1 << 63) - 1
    idx = [b % 3 for b in range(n)]
    model = R.Roll(3, policy, [0, R.word(4, policy), 0])
    want = model.cast(idx, top - n)
    got = parse(check("cast", write_case(tmp_path / "top.txt", idx, [0] * n, [0, R.word(4, policy), 0], top - n, policy), 2, 0))
    assert got["STATUS"] == want["status_out"] and got["BY"] == want["superseded_by"] and got["ROLL"] == model.words() and got["DISPLACED"] == want["displaced"]
    assert max(model.words()) == (top if policy == R.ROLL_LAST else R.word(4, policy))
    assert "REFUSED seq_base + n is above 2^63 - 1" in check("cast", write_case(tmp_path / "over.txt", idx, [0] * n, [0, 0, 0], top - n + 1, policy), 0, 0)


def test_hostcheck_layout_against_a_direct_count(check):
    def up(x):
        return (x + 255) // 256 * 256

    for n, n_keys in ((0, 0), (0, 40), (1, 1), (200, 40), (1024, 300), (1025, 300), (65536, 1 << 20), (1 << 20, 10 ** 7), ((1 << 31) - 1, 1 << 31)):
        tiles = (n + 1023) // 1024
        best, flag, sums = (up(4 * n_keys) if n else 0), up(4 * n), up(4 * tiles)
        assert f"LAYOUT tiles {tiles} best 0 flag {best} tile_sums {best + flag} total {best + flag + sums}\n" in check("layout", n, n_keys), (n, n_keys)


ALL = 0b1111111111   # key_index, roll, superseded_by, found, roster_groups, roster_weights, groups_out, weights_out, displaced, displaced_count


def test_hostcheck_refusal_rules(check):
    def refuse(n=1, n_keys=1, seq_base=0, policy=R.ROLL_LAST, mask=ALL):
        return check("refuse", n, n_keys, seq_base, policy, mask).split("\n")[0]

    top = (1 << 63) - 1
    assert refuse() == "REFUSE -" and refuse(policy=R.ROLL_FIRST) == "REFUSE -" and refuse(n=0, n_keys=0, mask=0) == "REFUSE -"
    assert refuse(n=(1 << 31) - 1, n_keys=1 << 31) == "REFUSE -" and refuse(n=5, seq_base=top - 5) == "REFUSE -" and refuse(mask=0b1111) == "REFUSE -"
    assert refuse(n=1 << 31) == "REFUSE n is 2^31 or more"
    assert refuse(n_keys=0) == "REFUSE n_keys is 0" and refuse(n_keys=(1 << 31) + 1) == "REFUSE n_keys is above EG_ROLL_KEYS_MAX"
    assert refuse(n=0, n_keys=(1 << 31) + 1, mask=0) == "REFUSE n_keys is above EG_ROLL_KEYS_MAX"
    for n, base in ((5, top - 4), (1, top), (0, top + 1), (1, (1 << 64) - 1)):
        assert refuse(n=n, seq_base=base) == "REFUSE seq_base + n is above 2^63 - 1", (n, base)
    for policy in (0, 3, -1):
        assert refuse(policy=policy) == "REFUSE policy is neither EG_ROLL_FIRST nor EG_ROLL_LAST"
    for k in range(4):
        assert refuse(mask=ALL & ~(1 << k)) == "REFUSE null key_index, roll, superseded_by or found", k
    assert refuse(mask=ALL & ~(1 << 4)) == "REFUSE groups_out without roster_groups" and refuse(mask=ALL & ~(1 << 6)) == "REFUSE -"
    assert refuse(mask=ALL & ~(1 << 5)) == "REFUSE weights_out without roster_weights" and refuse(mask=ALL & ~(1 << 7)) == "REFUSE -"
    for k in (8, 9):
        assert refuse(mask=ALL & ~(1 << k)) == "REFUSE displaced and displaced_count come together"


# ------------------------------------------------------------------ refusals of the library that need no GPU
def test_refusals_of_the_four_entries_without_a_gpu():
    """the argument rules come before the context is looked at; what passes them fails on the missing context; the scratch size of a
    refused call is 0"""
    lib = eg._load()
    buf = C.create_string_buffer(512)
    base = (C.addressof(buf) + 15) & ~15
    top = (1 << 63) - 1
    P = C.c_void_p

    def cast_dev(n=1, idx=base, st=None, seq_base=0, policy=R.ROLL_LAST, roll=base, n_keys=1, rg=None, rw=None, by=base, out=None, go=None, wo=None,
                 disp=None, count=None, found=base, scratch=base, sbytes=1 << 20):
        return lib.eg_roll_cast_device(None, n, P(idx), P(st), seq_base, policy, P(roll), n_keys, P(rg), P(rw), P(by), P(out), P(go), P(wo), P(disp),
                                       P(count), P(found), P(scratch), sbytes, None)

    def check_dev(n=1, idx=base, st=None, seq_base=0, policy=R.ROLL_LAST, roll=base, n_keys=1, rg=None, rw=None, by=base, out=None, go=None, wo=None,
                  found=base, **_):
        return lib.eg_roll_check_device(None, n, P(idx), P(st), seq_base, policy, P(roll), n_keys, P(rg), P(rw), P(by), P(out), P(go), P(wo), P(found), None)

    def cast_host(n=1, idx=base, st=None, seq_base=0, policy=R.ROLL_LAST, roll=base, n_keys=1, rg=None, rw=None, by=base, out=None, go=None, wo=None,
                  disp=None, count=None, found=base, **_):
        return lib.eg_roll_cast(None, n, P(idx), P(st), seq_base, policy, P(roll), n_keys, P(rg), P(rw), P(by), P(out), P(go), P(wo), P(disp), P(count),
                                P(found))

    def check_host(n=1, idx=base, st=None, seq_base=0, policy=R.ROLL_LAST, roll=base, n_keys=1, rg=None, rw=None, by=base, out=None, go=None, wo=None,
                   found=base, **_):
        return lib.eg_roll_check(None, n, P(idx), P(st), seq_base, policy, P(roll), n_keys, P(rg), P(rw), P(by), P(out), P(go), P(wo), P(found))

    common = (({"n": 1 << 31}, b"n is 2^31 or more"), ({"n": 1 << 40}, b"n is 2^31 or more"), ({"n_keys": 0}, b"n_keys is 0"),
              ({"n_keys": (1 << 31) + 1}, b"n_keys is above EG_ROLL_KEYS_MAX"), ({"n": 0, "n_keys": (1 << 31) + 1}, b"n_keys is above EG_ROLL_KEYS_MAX"),
              ({"seq_base": top}, b"seq_base + n is above 2^63 - 1"), ({"n": 3, "seq_base": top - 2}, b"seq_base + n is above 2^63 - 1"),
              ({"n": 0, "seq_base": 1 << 63}, b"seq_base + n is above 2^63 - 1"), ({"policy": 0}, b"policy is neither"), ({"policy": 3}, b"policy is neither"),
              ({"idx": None}, b"null key_index, roll, superseded_by or found"), ({"roll": None}, b"null key_index, roll, superseded_by or found"),
              ({"by": None}, b"null key_index, roll, superseded_by or found"), ({"found": None}, b"null key_index, roll, superseded_by or found"),
              ({"go": base}, b"groups_out without roster_groups"), ({"wo": base}, b"weights_out without roster_weights"))
    within = ({}, {"policy": R.ROLL_FIRST}, {"n": 3, "seq_base": top - 3}, {"n": (1 << 31) - 1, "n_keys": 1 << 31, "sbytes": 1 << 40},
              {"n": 0, "n_keys": 0, "idx": None, "roll": None, "by": None, "found": None, "scratch": None, "sbytes": 0},
              {"st": base, "out": base, "rg": base, "rw": base, "go": base, "wo": base}, {"rg": base, "rw": base})
    for call in (cast_dev, check_dev, cast_host, check_host):
        for kw, text in common:
            assert call(**kw) == BAD_ARG and text in lib.eg_last_error(), (call.__name__, kw, lib.eg_last_error())
        for kw in within:
            assert call(**kw) == BAD_ARG and b"roll: null ctx" in lib.eg_last_error(), (call.__name__, kw, lib.eg_last_error())
    for call in (cast_dev, cast_host):
        for kw in ({"disp": base}, {"count": base}):
            assert call(**kw) == BAD_ARG and b"displaced and displaced_count come together" in lib.eg_last_error(), (call.__name__, kw)
        assert call(disp=base, count=base) == BAD_ARG and b"null ctx" in lib.eg_last_error()
    # the scratch: null or too small (one ballot, one key: three parts of 256 bytes)
    for kw in ({"scratch": None}, {"sbytes": 0}, {"sbytes": 767}):
        assert cast_dev(**kw) == BAD_ARG and b"scratch is null or too small" in lib.eg_last_error(), kw
    assert cast_dev(sbytes=768) == BAD_ARG and b"null ctx" in lib.eg_last_error()
    # alignment, device forms: 64-bit arrays on 8 bytes, 32-bit arrays on 4
    for call in (cast_dev, check_dev):
        for kw in ({"roll": base + 4}, {"by": base + 4}, {"rw": base + 4}, {"rw": base, "wo": base + 4}):
            assert call(**kw) == BAD_ARG and b"8-byte aligned" in lib.eg_last_error(), (call.__name__, kw)
        for kw in ({"idx": base + 2}, {"st": base + 1}, {"out": base + 2}, {"rg": base + 2}, {"rg": base, "go": base + 3}, {"found": base + 2}):
            assert call(**kw) == BAD_ARG and b"4-byte aligned" in lib.eg_last_error(), (call.__name__, kw)
        assert call(idx=base + 4, st=base + 4, out=base + 4, rg=base + 4, go=base + 4, found=base + 4) == BAD_ARG and b"null ctx" in lib.eg_last_error()
    for kw in ({"disp": base + 4, "count": base}, {"disp": base, "count": base + 4}):
        assert cast_dev(**kw) == BAD_ARG and b"8-byte aligned" in lib.eg_last_error(), kw
    assert cast_dev(scratch=base + 2) == BAD_ARG and b"4-byte aligned" in lib.eg_last_error()
    for n, n_keys in ((1, 1), (100, 40), (1 << 31, 1), (1, 0), (1, (1 << 31) + 1), (0, 5)):
        assert lib.eg_roll_cast_scratch_bytes(None, n, n_keys) == 0


def test_missing_gpu_is_loud():
    roll = object.__new__(eg.VoterRoll)
    roll.ctx, roll.policy = type("NoCtx", (), {"_h": None})(), eg.ROLL_LAST
    with pytest.raises(eg.EgError, match="null ctx"):
        roll.cast([0, 1, 0], [0, 0])
    with pytest.raises(eg.EgError, match="null ctx"):
        roll.check([0, 1, 0], [0, 0], seq_base=7, status_in=[0, 0, 5], roster_groups=[1, 2], roster_weights=[3, 4])
    with pytest.raises(eg.EgError, match="n_keys is 0"):
        roll.cast([0], [])
    roll.policy = 0
    with pytest.raises(eg.EgError, match="policy is neither"):
        roll.check([0], [0])
    assert roll.cast_scratch_bytes(10, 10) == 0


# ------------------------------------------------------------------ merge_rolls over gloo
def _merge_worker(rank, world, port, policy, exe, tmp, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from elastic_elgamal_amd import distributed as egd

    idx, status, n_keys = _shared_voters()
    lo, hi = egd.shard_range(len(idx), rank, world)

    def run(cmd, roll):
        path = write_case(Path(tmp) / f"{cmd}{rank}.txt", idx[lo:hi], status[lo:hi], roll, lo, policy, displaced=False)
        r = subprocess.run([exe, cmd, str(path), str(rank + 1), "0"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-500:] + r.stderr[-3000:]
        return parse(r.stdout)

    local = run("cast", [0] * n_keys)["ROLL"]
    merged = egd.merge_rolls(torch.tensor(local, dtype=torch.int64)).tolist()
    as_u64 = egd.merge_rolls(torch.tensor(local, dtype=torch.int64).view(torch.uint64)).view(torch.int64).tolist()
    kept = [lo + b for b, s in enumerate(run("check", merged)["STATUS"]) if s == 0]
    q.put((rank, local, merged, as_u64, kept))
    dist.destroy_process_group()


def _shared_voters():
    rng = random.Random(77)
    n, n_keys = 90, 25
    idx = [rng.randrange(n_keys) for _ in range(n)]
    status = [0 if rng.random() < 0.85 else 4 for _ in range(n)]
    return idx, status, n_keys


@pytest.mark.parametrize("policy", POLICIES)
def test_merge_rolls_over_gloo_at_world_size_two(check, tmp_path, policy):
    """two ranks cast disjoint slabs that share voters into rolls of their own (the lane functions of the host check program), merge them
    with ONE all-reduce and check their slabs against the merged roll: the kept set is the model's over the concatenation"""
    import torch
    import torch.multiprocessing as mp
    from elastic_elgamal_amd import distributed as egd

    single = torch.tensor([5, 0, 9], dtype=torch.int64)
    assert egd.merge_rolls(single) is single                          # a single process returns its input
    idx, status, n_keys = _shared_voters()
    model = R.Roll(n_keys, policy)
    model.cast(idx, 0, status)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() + policy) % 2000
    procs = [ctx.Process(target=_merge_worker, args=(r, world, port, policy, str(HERE / "rollcheck"), str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] != res[1][1] and sum(a != 0 and b != 0 for a, b in zip(res[0][1], res[1][1])) >= 10         # the slabs share voters
    assert res[0][2] == res[1][2] == res[0][3] == res[1][3] == model.words() == R.merge(res[0][1], res[1][1])
    assert res[0][4] + res[1][4] == model.kept(idx, 0, status) and len(res[0][4] + res[1][4]) == sum(w != 0 for w in model.words())
