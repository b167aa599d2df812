"""The weighted per-group tally (eg_*_tally_weighted*, csrc/group_tally_kernels.cuh, csrc/group_tally_host.hpp) without a GPU.

* The six entry points are declared, exported, bound in Python and mirrored in C++; ABI version 7; the header stays plain C; no new knob.
* The refusals that need no GPU, and a loud failure without one.
* tests/hostcheck/weightedtallycheck.cpp: ge_mul_u64 and the lane functions of the weighted pass, -DEG_BOUNDCHECK under ASan + UBSan.
  (a) ge_mul_u64 over corner and random weights of every width against oracle.point_multi_mul; (b) the whole pipeline, serially, with
  piece sizes 2 / 2 and 3 / 2 against the oracle's weighted sum of every group and slot, the weight sums against Python integers;
  (c) the scratch layout against a direct count.
Every expected value comes from the CPU oracle."""
import ctypes as C
import random
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import group_tally_cases as G
import weighted_tally_cases as W

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
SIZES = ("eg_choice_tally_weighted_scratch_bytes", "eg_qv_tally_weighted_scratch_bytes")
DEVICE = ("eg_choice_tally_weighted_device", "eg_qv_tally_weighted_device")
HOST = ("eg_choice_tally_weighted", "eg_qv_tally_weighted")
BAD_ARG = -3
M64 = W.M64


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for names, ret, restype, nargs in ((SIZES, "size_t", C.c_size_t, 3), (DEVICE, "int", C.c_int, 14), (HOST, "int", C.c_int, 11)):
        for name in names:
            assert re.search(rf"^{ret} {name}\(", header, re.M), name
            assert name in eg.exported_symbols()
            assert hasattr(raw, name), f"{name} is not exported"
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == nargs, name
    # a section of its own, directly behind the per-group tally and in front of the multi-GPU one
    at = header.index("eg_choice_tally_weighted_scratch_bytes(")
    assert header.index("int eg_qv_tally_grouped(") < at < header.index("int eg_verify_choice_batch_multi(")
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert lib.eg_abi_version() == 7


def test_python_and_cpp_mirrors_exist(tmp_path):
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        assert callable(cls.tally_weighted) and callable(cls.tally_weighted_device) and callable(cls.tally_weighted_scratch_bytes)
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count("WeightedTally tally_weighted(") == 2 and hpp.count("void tally_weighted_device(") == 2
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        template <class P> WeightedTally host(const P& p) {
          WeightedTally one = p.tally_weighted(Bytes(), {}, {}, 16);
          WeightedTally many = p.tally_weighted(Bytes(), {}, {}, 64, {}, 3);
          return one.totals.size() ? one : many;
        }
        template <class P> void dev(const P& p) {
          p.tally_weighted_device(0, nullptr, nullptr, nullptr, 16, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
          p.tally_weighted_device(0, nullptr, nullptr, nullptr, 16, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
          (void)p.tally_weighted_scratch_bytes(0, 3);
        }
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element pk{};
            ChoiceParams c = ChoiceParams::single(ctx, pk, 5);
            QuadraticVotingParams q(ctx, pk, 5, 20);
            WeightedTally a = host(c), b = host(q);
            dev(c); dev(q);
            return (int)(a.totals.size() + b.accepted.size() + a.weight_sums.size() + b.weight_sums[0].high);
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
    src.write_text('#include "eg_hip.h"\nint main(void) { return eg_choice_tally_weighted && eg_qv_tally_weighted_device && '
                   'eg_qv_tally_weighted_scratch_bytes ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob():
    src = (CSRC / "eg_hip.hip").read_text()
    a, b = src.index("static Knobs read_knobs()"), src.index("// Fault points:")
    assert len(set(re.findall(r'"(EG_[A-Z_]+)"', src[a:b]))) == 16
    a, b = src.index("static size_t weighted_scratch_bytes("), src.index("// builds the wide comb tables now")
    assert "getenv" not in src[a:b] and "EG_LOCK" not in src[a:b] and "ws_acquire" not in src[a:b]      # stateless: no knob, no lock, no workspace
    for f in ("group_tally_kernels.cuh", "group_tally_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()


# ------------------------------------------------------------------ refusals that need no GPU
def test_refusals_of_the_host_and_device_entries_without_a_gpu():
    """argument checks come before any device work and before the params object is looked at: what the grouped entry refuses, then
    weight_bits outside 1..64, NULL weights with n > 0, NULL groups with n_groups != 1; arguments that pass them fail on the missing
    params object; the scratch size of a refused call is 0"""
    lib = eg._load()
    one = (C.c_uint32 * 1)()
    w = (C.c_uint64 * 1)()
    for name in HOST + DEVICE:
        fn = getattr(lib, name)

        def call(n, n_groups, bits=64, weights=w, groups=one):
            if name in HOST:
                rc = fn(None, n, None, one, weights, bits, groups, n_groups, None, None, None)
            else:
                rc = fn(None, n, None, one, weights, bits, groups, n_groups, None, None, None, None, None, None)
            return rc, lib.eg_last_error()

        assert call(1, 0) == (BAD_ARG, b"weighted tally: n_groups is 0"), name
        for ng in ((1 << 24) + 1, 0xFFFFFFFF):
            rc, msg = call(1, ng)
            assert rc == BAD_ARG and b"EG_TALLY_GROUPS_MAX" in msg, (name, ng)
        for n in (1 << 31, 1 << 40):
            rc, msg = call(n, 7)
            assert rc == BAD_ARG and b"2^31" in msg, (name, n)
        for bits in (0, -1, 65, 1 << 20):
            rc, msg = call(1, 7, bits=bits)
            assert rc == BAD_ARG and b"weight_bits" in msg, (name, bits)
        assert call(1, 7, weights=None) == (BAD_ARG, b"weighted tally: null weights"), name
        for ng in (2, 7):
            rc, msg = call(1, ng, groups=None)
            assert rc == BAD_ARG and b"n_groups must be 1" in msg, (name, ng)
        for kw in (dict(n=1, n_groups=1), dict(n=1, n_groups=1, groups=None), dict(n=(1 << 31) - 1, n_groups=1 << 24), dict(n=0, n_groups=7),
                   dict(n=0, n_groups=1, weights=None, groups=None), dict(n=1, n_groups=3, bits=1), dict(n=1, n_groups=3, bits=64)):
            rc, msg = call(**kw)
            assert rc == BAD_ARG and b"null params" in msg, (name, kw)
    for name in SIZES:
        fn = getattr(lib, name)
        for n, ng in ((1, 0), (1, (1 << 24) + 1), (1 << 31, 7), (100, 7)):
            assert fn(None, n, ng) == 0, (name, n, ng)


def test_missing_gpu_is_loud():
    for cls, prefix in ((eg.ChoiceParams, "choice"), (eg.QuadraticVotingParams, "qv")):
        p = object.__new__(cls)              # what a caller would hold if a params object could exist without a GPU: no handle
        p._h, p._prefix, p.ballot_size, p.n_options = None, prefix, 736, 5
        with pytest.raises(eg.EgError, match="null params"):
            p.tally_weighted(bytes(736), [0], [5], [0], 3)
        with pytest.raises(eg.EgError, match="null params"):
            p.tally_weighted(bytes(736), [0], [5])
        with pytest.raises(eg.EgError, match="n_groups is 0"):
            p.tally_weighted(bytes(736), [0], [5], [0], 0)
        with pytest.raises(eg.EgError, match="weight_bits"):
            p.tally_weighted(bytes(736), [0], [5], [0], 3, weight_bits=0)
        with pytest.raises(eg.EgError, match="n_groups must be 1"):
            p.tally_weighted(bytes(736), [0], [5], None, 3)
        with pytest.raises(eg.EgError, match="null params"):
            p.tally_weighted_device(1, 0, 0, 8, 16, 0, 1, 0, 0, 0)
        with pytest.raises(ValueError):
            p.tally_weighted(bytes(736), [0], [5, 6], [0], 3)
        with pytest.raises(ValueError):
            p.tally_weighted(bytes(736), [0], [1 << 64], [0], 3)
        assert p.tally_weighted_scratch_bytes(100, 3) == 0


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "weightedtallycheck", HERE / "weightedtallycheck.cpp"
    deps = [src, *CSRC.glob("*.cuh"), *CSRC.glob("*.hpp"), CSRC / "plan.h"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout

    return run


@pytest.fixture(scope="module")
def pk(oracle):
    return oracle.keypair_from_seed(12345)[1]


@pytest.fixture(scope="module")
def points(oracle, pk):
    """the identity, the generator, and points the oracle made: the public key and the ciphertext points of two ballots"""
    ballots = oracle.ChoiceParams(pk, 2, True).generate_batch(31, 0, 2, threads=1)
    size = len(ballots) // 2
    made = [ballots[b * size + 32 * i:b * size + 32 * i + 32] for b in range(2) for i in range(4)]
    return [bytes(32), oracle.point_mul_generator((1).to_bytes(32, "little")), pk] + made


def _products(check, tmp_path, lines):
    (tmp_path / "mul.txt").write_text("".join(f"{bits} {w} {p.hex()}\n" for bits, w, p in lines))
    got = [bytes.fromhex(x) for x in re.findall(r"^MUL ([0-9a-f]{64})$", check("mul", tmp_path / "mul.txt"), re.M)]
    assert len(got) == len(lines)
    return got


def test_ge_mul_u64_against_the_oracle_at_every_width(check, oracle, points, tmp_path):
    """(a) corner weights and random ones at every width, times the identity, the generator and oracle-made points: ge_mul_u64's
    encoding equals oracle.point_multi_mul's, with every limb-class assertion of the bound-check build live"""
    lines = []
    for bits in W.WIDTHS:
        ws = W.corner_weights(bits) + W.random_weights(1000 + bits, 3, bits)
        for k, w in enumerate(ws):
            for p in (points[:3] if k % 2 else points[:2] + [points[3 + (k + bits) % 8]]):
                lines.append((bits, w, p))
    assert {w for b, w, _ in lines if b == 64} >= {0, 1, 2, 3, 1 << 63, M64, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555}
    got = _products(check, tmp_path, lines)
    for (bits, w, p), enc in zip(lines, got):
        assert enc == W.weighted_sum(oracle, [w], [p]), (bits, w, p.hex())
        if p == bytes(32) or w == 0:
            assert enc == bytes(32)


def test_a_weight_longer_than_the_width_gives_another_product(check, oracle, points, tmp_path):
    """ge_mul_u64 reads `bits` bits and no more: a weight of W + 1 bits under W comes out as [w mod 2^W] P, not [w] P - so the range check
    of the count and fill kernels, not the ladder, is the guard a caller sees (bad[2])"""
    g = points[1]
    lines = [(bits, w, g) for bits in (1, 2, 8, 31, 32, 33, 63) for w in ((1 << bits) | 1, (1 << (bits + 1)) - 1, 1 << bits)]
    got = _products(check, tmp_path, lines)
    for (bits, w, p), enc in zip(lines, got):
        assert enc == W.weighted_sum(oracle, [w & ((1 << bits) - 1)], [p])
        assert enc != W.weighted_sum(oracle, [w], [p])


# ------------------------------------------------------------------ the whole pipeline, serially
def _write_case(path, op, ballots, status, weights, groups, n_groups, bits):
    n = len(status)
    lines = [f"{n} {n_groups} {op.n_options} {int(op.single)} {bits} {int(groups is not None)}"]
    for b in range(n):
        lines.append(f"{status[b]} {0 if groups is None else groups[b]} {weights[b]} {ballots[b * op.ballot_size:(b + 1) * op.ballot_size].hex()}")
    path.write_text("\n".join(lines) + "\n")


def _report(out):
    bad = tuple(int(x) for x in re.search(r"^BAD (\d+) (\d+) (\d+)$", out, re.M).groups())
    counts = [int(x) for x in re.search(r"^COUNTS :(.*)$", out, re.M).group(1).split()]
    words = [int(x) for x in re.search(r"^SUMS :(.*)$", out, re.M).group(1).split()]
    sums = [words[2 * g] | (words[2 * g + 1] << 64) for g in range(len(words) // 2)]
    tallies = b"".join(bytes.fromhex(m.group(1)) for m in re.finditer(r"^TALLY \d+ ([0-9a-f]+)$", out, re.M))
    return bad, counts, sums, tallies, int(re.search(r"^LEVELS (\d+)$", out, re.M).group(1))


@pytest.fixture(scope="module")
def corpus(oracle, pk):
    """62 oracle-made 2-option ballots: every fifth tampered, 7 groups of which group 4 is empty, four ballots in no group, shuffled;
    64-bit weights with the corner set, two of 2^64 - 1 in group 1"""
    op = oracle.ChoiceParams(pk, 2, True)
    n, n_groups = 62, 7
    raw = bytearray(op.generate_batch(2025, 0, n, threads=2))
    for b in range(0, n, 5):
        raw[b * op.ballot_size + 32 * (b % 9) + 5] ^= 0x40
    rng = random.Random(63)
    order = list(range(n))
    rng.shuffle(order)
    ballots = b"".join(bytes(raw[b * op.ballot_size:(b + 1) * op.ballot_size]) for b in order)
    status = op.verify_batch(ballots, threads=2)
    live = [0, 1, 2, 3, 5, 6]
    groups = [live[rng.randrange(6)] if rng.random() < 0.7 else 1 for _ in range(n)]          # group 1 holds about a third
    for b in rng.sample(range(n), 4):
        groups[b] = G.GROUP_NONE
    weights = (W.corner_weights(64) + W.random_weights(5, n, 64))[:n]
    in_one = [b for b in range(n) if status[b] == 0 and groups[b] == 1]
    weights[in_one[0]] = weights[in_one[-1]] = M64
    assert 0 < sum(1 for s in status if s) < n and 4 not in groups and len(in_one) >= 3
    return op, ballots, status, weights, groups, n_groups


@pytest.mark.parametrize("s1,s2", [(2, 2), (3, 2)])
def test_pipeline_on_the_host_equals_the_oracle_per_group(check, oracle, corpus, tmp_path, s1, s2):
    """(b) count, scan, fill, weighted sum from the wire, sums of partial sums and of weight sums, encode - the lane functions of the
    kernels, serially - give the oracle's weighted sum of every group and slot byte for byte, exact counts, and weight sums equal to
    Python's integers (two weights of 2^64 - 1 in one group carry into the high word)"""
    op, ballots, status, weights, groups, n_groups = corpus
    _write_case(tmp_path / "case.txt", op, ballots, status, weights, groups, n_groups, 64)
    bad, counts, sums, tallies, levels = _report(check("run", tmp_path / "case.txt", s1, s2))
    want, want_sums, want_counts, bad2 = W.expected(oracle, op, ballots, status, weights, groups, n_groups, 64)
    assert bad == (0, 0, 0) and bad2 == 0 and counts == want_counts and counts[4] == 0
    assert sums == want_sums and sums[4] == 0 and sums[1] >> 64 >= 1
    assert tallies == want
    assert tallies[4 * 128:5 * 128] == bytes(128)
    assert levels == G.depth(len(status), s1, s2) >= 5


def test_pipeline_with_all_weights_one_is_the_unweighted_tally(check, oracle, corpus, tmp_path):
    """every weight 1, at weight_bits 1 and 64: the oracle's own per-group tally (ChoiceParams.tally), byte for byte; weight sums =
    counts; and with groups == NULL the tally of the whole batch"""
    op, ballots, status, _, groups, n_groups = corpus
    ones = [1] * len(status)
    want, want_counts = G.expected(op, ballots, status, groups, n_groups)
    for bits in (1, 64):
        _write_case(tmp_path / "ones.txt", op, ballots, status, ones, groups, n_groups, bits)
        bad, counts, sums, tallies, _ = _report(check("run", tmp_path / "ones.txt", 3, 2))
        assert bad == (0, 0, 0) and counts == want_counts == sums and tallies == want
    _write_case(tmp_path / "whole.txt", op, ballots, status, ones, None, 1, 1)
    bad, counts, sums, tallies, _ = _report(check("run", tmp_path / "whole.txt", 2, 2))
    assert bad == (0, 0, 0) and counts == sums == [status.count(0)] and tallies == op.tally(ballots, status)


def test_pipeline_on_the_host_counts_weights_out_of_range(check, oracle, corpus, tmp_path):
    """weight_bits 8: accepted ballots with weights 2^8 and 2^64 - 1 count in bad[2] and are left out of tallies, counts and sums; the
    same weights on rejected ballots are never read (the check program fails if they are); a weight of 0 counts and adds nothing"""
    op, ballots, status, _, groups, n_groups = corpus
    n = len(status)
    weights = W.random_weights(8, n, 8)
    accepted = [b for b in range(n) if status[b] == 0 and groups[b] != G.GROUP_NONE]
    rejected = [b for b in range(n) if status[b] != 0]
    weights[accepted[0]], weights[accepted[1]], weights[accepted[2]] = 1 << 8, M64, 0
    weights[rejected[0]], weights[rejected[1]] = 1 << 8, M64
    _write_case(tmp_path / "range.txt", op, ballots, status, weights, groups, n_groups, 8)
    bad, counts, sums, tallies, _ = _report(check("run", tmp_path / "range.txt", 2, 2))
    want, want_sums, want_counts, bad2 = W.expected(oracle, op, ballots, status, weights, groups, n_groups, 8)
    assert bad == (0, 0, 2) and bad2 == 2
    assert counts == want_counts and sum(counts) == len(accepted) - 2 and sums == want_sums and tallies == want


def test_pipeline_on_the_host_counts_hostile_inputs(check, oracle, corpus, tmp_path, rejections):
    """an accepted ballot with the id n_groups and a forged status 0 over the reference's rejecting encoding give bad = (1, 1, 0); the same
    two things on REJECTED ballots are never looked at"""
    op, ballots, status, weights, groups, n_groups = corpus
    non_element = bytes.fromhex(rejections["non_element"]["hex"])
    accepted = [b for b, s in enumerate(status) if s == 0 and groups[b] != G.GROUP_NONE]
    rejected = [b for b, s in enumerate(status) if s != 0]
    st, gr, by = list(status), list(groups), bytearray(ballots)
    gr[accepted[0]] = n_groups
    by[accepted[1] * op.ballot_size + 32:accepted[1] * op.ballot_size + 64] = non_element          # tally item 1, status left at 0
    assert op.verify_batch(bytes(by))[accepted[1]] != 0                                             # forged: no verifier accepts it
    _write_case(tmp_path / "hostile.txt", op, bytes(by), st, weights, gr, n_groups, 64)
    bad, counts, _, _, _ = _report(check("run", tmp_path / "hostile.txt", 2, 2))
    assert bad == (1, 1, 0) and sum(counts) == len(accepted) - 1
    st, gr, by = list(status), list(groups), bytearray(ballots)
    gr[rejected[0]] = n_groups
    gr[rejected[2]] = 0xFFFFFFFE
    by[rejected[1] * op.ballot_size + 32:rejected[1] * op.ballot_size + 64] = non_element
    _write_case(tmp_path / "ignored.txt", op, bytes(by), st, weights, gr, n_groups, 64)
    bad, counts, sums, tallies, _ = _report(check("run", tmp_path / "ignored.txt", 2, 2))
    want, want_sums, want_counts, _ = W.expected(oracle, op, ballots, status, weights, groups, n_groups, 64)
    assert bad == (0, 0, 0) and counts == want_counts and sums == want_sums and tallies == want


# ------------------------------------------------------------------ scratch layout
@pytest.mark.parametrize("n,n_groups,n_slots,s1,s2", [(0, 1, 10, 32, 32), (1, 1, 4, 32, 32), (1000, 7, 10, 32, 32), (62, 7, 4, 2, 2),
                                                       (32 * 32 * 32 + 1, 3, 4, 32, 32), (5000, 100000, 32, 32, 32)])
def test_scratch_layout_against_a_direct_count(check, n, n_groups, n_slots, s1, s2):
    """(c) the weighted layout is the grouped layout and, behind it, 16 bytes per piece for each of the two alternating levels (pieces
    counted directly: whole pieces plus one ragged piece per non-empty group), every part 256-byte aligned"""
    row = check("layout", n, n_groups, n_slots, s1, s2)
    v = dict(zip(*[iter(re.search(r"^LAYOUT (.*)$", row, re.M).group(1).split())] * 2))
    v = {k: int(x) for k, x in v.items()}
    up = lambda x: -(-x // 256) * 256
    levels = G.depth(n, s1, s2) if n else 1
    pieces0 = n // s1 + min(n, n_groups)
    pieces1 = pieces0 // s2 + min(n, n_groups) if levels > 1 else 0
    assert (v["levels"], v["pieces0"], v["pieces1"]) == (levels, pieces0, pieces1)
    assert v["grouped"] % 256 == 0 and v["wsum0"] == v["grouped"]
    assert v["wsum1"] == v["wsum0"] + up(16 * pieces0) and v["total"] == v["wsum1"] + up(16 * pieces1)
    # the worst case really fits: one ragged piece per group and whole pieces for the rest
    assert pieces0 >= sum(-(-c // s1) for c in ([n - min(n, n_groups) + 1] + [1] * (min(n, n_groups) - 1) if n else []))
