"""The per-group tally (eg_*_tally_grouped*, csrc/group_tally_kernels.cuh, csrc/group_tally_host.hpp) without a GPU.

* The six entry points are declared, exported, bound in Python and mirrored in C++; the two constants agree; ABI version 7.
* tests/hostcheck/grouptallycheck.cpp: host_plan.hpp, group_tally_host.hpp and the lane functions of the kernels, -DEG_BOUNDCHECK under
  ASan + UBSan.  (a) the wire items behind the tally slots against the oracle's tally of one ballot; (b) the piece / level arithmetic
  against a direct count; (c) the whole pipeline, serially, with piece sizes 2 / 2 and 3 / 2 against the oracle's tally of every group.
* The refusals of the host entries that need no GPU; a grouped tally through distributed.gather_tallies on two gloo ranks."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import group_tally_cases as G

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
SIZES = ("eg_choice_tally_grouped_scratch_bytes", "eg_qv_tally_grouped_scratch_bytes")
DEVICE = ("eg_choice_tally_grouped_device", "eg_qv_tally_grouped_device")
HOST = ("eg_choice_tally_grouped", "eg_qv_tally_grouped")
BAD_ARG = -3


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for names, ret, restype, nargs in ((SIZES, "size_t", C.c_size_t, 3), (DEVICE, "int", C.c_int, 11), (HOST, "int", C.c_int, 8)):
        for name in names:
            assert re.search(rf"^{ret} {name}\(", header, re.M), name
            assert name in eg.exported_symbols()
            assert hasattr(raw, name), f"{name} is not exported"
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == nargs, name
    # a section of its own, behind the small-batch tier and in front of the multi-GPU one
    at = header.index("eg_choice_tally_grouped_scratch_bytes(")
    assert header.index("int eg_verify_qv_small_device(") < at < header.index("int eg_verify_choice_batch_multi(")


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    assert int(re.search(r"#define EG_GROUP_NONE\s+0x([0-9a-f]+)u", header).group(1), 16) == eg.GROUP_NONE == 0xFFFFFFFF == G.GROUP_NONE
    assert re.search(r"#define EG_TALLY_GROUPS_MAX\s+\(1u << 24\)", header) and eg.TALLY_GROUPS_MAX == 1 << 24
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7
    host = (CSRC / "group_tally_host.hpp").read_text()
    assert "GROUP_NONE = 0xffffffffu" in host and "GROUPS_MAX = 1u << 24" in host
    s1, s2 = G.piece_sizes()
    assert s1 >= 2 and s2 >= 2 and s1 * s2 * s2 <= 1 << 16          # a test below 10^5 ballots reaches the fourth level


def test_python_and_cpp_mirrors_exist(tmp_path):
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        assert callable(cls.tally_grouped) and callable(cls.tally_grouped_device) and callable(cls.tally_grouped_scratch_bytes)
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count("GroupedTally tally_grouped(") == 2 and hpp.count("void tally_grouped_device(") == 2
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        template <class P> GroupedTally host(const P& p) { return p.tally_grouped(Bytes(), {}, {}, 3); }
        template <class P> void dev(const P& p) {
          p.tally_grouped_device(0, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr, nullptr);
          p.tally_grouped_device(0, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr);
          (void)p.tally_grouped_scratch_bytes(0, 3);
        }
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element pk{};
            ChoiceParams c = ChoiceParams::single(ctx, pk, 5);
            QuadraticVotingParams q(ctx, pk, 5, 20);
            GroupedTally a = host(c), b = host(q);
            dev(c); dev(q);
            return (int)(a.totals.size() + b.accepted.size());
          }
          static_assert(EG_GROUP_NONE == 0xffffffffu && EG_TALLY_GROUPS_MAX == (1u << 24), "header constants");
          return 0;
        }
        """).replace("NS;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_GROUP_NONE == 0xffffffffu && eg_choice_tally_grouped && eg_qv_tally_grouped_device ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob():
    src = (ROOT / "elastic_elgamal_amd" / "csrc" / "eg_hip.hip").read_text()
    a, b = src.index("static Knobs read_knobs()"), src.index("// Fault points:")
    assert len(set(re.findall(r'"(EG_[A-Z_]+)"', src[a:b]))) == 16
    for f in ("group_tally_kernels.cuh", "group_tally_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()


# ------------------------------------------------------------------ refusals that need no GPU
def test_refusals_of_the_host_and_device_entries_without_a_gpu():
    """argument checks come before any device work and before the params object is looked at: n_groups == 0, n_groups above
    EG_TALLY_GROUPS_MAX and n >= 2^31 are refused as such; the limits themselves are not over the limit (the call then fails on the
    missing params object); the scratch size of a refused call is 0"""
    lib = eg._load()
    one = (C.c_uint32 * 1)()
    for name in HOST + DEVICE:
        fn = getattr(lib, name)
        tail = (None, None) if name in HOST else (None, None, None, None, None)

        def call(n, n_groups):
            rc = fn(None, n, None, one, one, n_groups, *tail)
            return rc, lib.eg_last_error()

        assert call(1, 0) == (BAD_ARG, b"grouped tally: n_groups is 0"), name
        for ng in ((1 << 24) + 1, 0xFFFFFFFF):
            rc, msg = call(1, ng)
            assert rc == BAD_ARG and b"EG_TALLY_GROUPS_MAX" in msg, (name, ng)
        for n in (1 << 31, 1 << 40):
            rc, msg = call(n, 7)
            assert rc == BAD_ARG and b"2^31" in msg, (name, n)
        for n, ng in ((1, 1), ((1 << 31) - 1, 1 << 24), (0, 7)):
            rc, msg = call(n, ng)
            assert rc == BAD_ARG and b"null params" in msg, (name, n, ng)
    for name in SIZES:
        fn = getattr(lib, name)
        for n, ng in ((1, 0), (1, (1 << 24) + 1), (1 << 31, 7), (100, 7)):
            assert fn(None, n, ng) == 0, (name, n, ng)


def test_missing_gpu_is_loud():
    for cls, prefix in ((eg.ChoiceParams, "choice"), (eg.QuadraticVotingParams, "qv")):
        p = object.__new__(cls)              # what a caller would hold if a params object could exist without a GPU: no handle
        p._h, p._prefix, p.ballot_size, p.n_options = None, prefix, 736, 5
        with pytest.raises(eg.EgError, match="null params"):
            p.tally_grouped(bytes(736), [0], [0], 3)
        with pytest.raises(eg.EgError, match="n_groups is 0"):
            p.tally_grouped(bytes(736), [0], [0], 0)
        with pytest.raises(eg.EgError, match="EG_TALLY_GROUPS_MAX"):
            p.tally_grouped(bytes(736), [0], [0], (1 << 24) + 1)
        with pytest.raises(eg.EgError, match="null params"):
            p.tally_grouped_device(1, 0, 0, 0, 3, 0, 0, 0)
        with pytest.raises(ValueError):
            p.tally_grouped(bytes(736), [0, 0], [0], 3)
        assert p.tally_grouped_scratch_bytes(100, 3) == 0


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "grouptallycheck", HERE / "grouptallycheck.cpp"
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


def test_tally_items_are_the_ciphertext_points_of_the_ballot(check, oracle, pk):
    """(a) for single choice 2 / 5 / 150, multi choice 16 and quadratic voting (5, 20) / (3, 10^4): the 32-byte wire items that the
    plan's tally slots stand for, concatenated from one accepted ballot, are the oracle's tally of that ballot"""
    shapes = {"single2": oracle.ChoiceParams(pk, 2, True), "single5": oracle.ChoiceParams(pk, 5, True),
              "single150": oracle.ChoiceParams(pk, 150, True), "multi16": oracle.ChoiceParams(pk, 16, False),
              "qv5_20": oracle.QvParams(pk, 5, 20), "qv3_10000": oracle.QvParams(pk, 3, 10000)}
    seen = set()
    for line in check("items").splitlines():
        if not line.startswith("ITEMS"):
            continue
        name, stride = line.split()[1], int(line.split()[3])
        items = [int(x) for x in line.split(":")[1].split()]
        op = shapes[name]
        assert stride == op.ballot_size and len(items) == 2 * op.n_options and len(set(items)) == len(items)
        ballot = op.generate_batch(777, 0, 1, 3) if name == "multi16" else op.generate_batch(777, 0, 1)
        assert op.verify_batch(ballot) == [0]
        assert b"".join(ballot[32 * i:32 * i + 32] for i in items) == op.tally(ballot, [0]), name
        if name.startswith("qv3"):
            assert items[2] - items[1] > 3          # partial ciphertexts lie between two tally items
        seen.add(name)
    assert seen == set(shapes)


@pytest.mark.parametrize("s", [2, 3])
def test_piece_and_level_arithmetic_against_a_direct_count(check, s):
    """(b) offsets, pieces and first pieces of every level, the group of every piece (gt_bucket_of), a last level with at most one entry
    per group, and a depth that depends on n alone, in closed form"""
    for counts in G.count_vectors(s):
        out = check("scan", s, s, *counts)
        levels, offsets, per_level = G.scan_reference(counts, s, s)
        assert levels == G.depth(sum(counts), s, s)
        assert f"LEVELS {levels}\n" in out, counts
        rows = {" ".join(l.split(":")[0].split()[:2]): [int(x) for x in l.split(":")[1].split()] for l in out.splitlines() if ":" in l}
        assert rows["OFFSETS"] == offsets, counts
        for l, (pieces, piece0, buckets) in enumerate(per_level):
            assert rows[f"PIECES {l}"] == pieces and rows[f"PIECE0 {l}"] == piece0 and rows[f"BUCKETS {l}"] == buckets, (counts, l)
            assert f"PIECES {l} total {sum(pieces)} :" in out
        assert max(per_level[-1][0]) <= 1
    # the depth is that of the worst case, one group with everything, whatever the groups are
    n = s * s * s + 1
    assert G.depth(n, s, s) == 4 == G.scan_reference([1] * n, s, s)[0] == G.scan_reference([n], s, s)[0]
    # the production sizes: the seventh level is the last one below 2^31 ballots
    s1, s2 = G.piece_sizes()
    assert G.depth((1 << 31) - 1, s1, s2) <= 7 and G.depth(s1 * s2 * s2 + 1, s1, s2) == 4


def _write_case(path, op, ballots, status, groups, n_groups):
    n = len(status)
    lines = [f"{n} {n_groups} {op.n_options} {int(op.single)}"]
    for b in range(n):
        lines.append(f"{status[b]} {groups[b]} {ballots[b * op.ballot_size:(b + 1) * op.ballot_size].hex()}")
    path.write_text("\n".join(lines) + "\n")


def _report(out):
    bad = tuple(int(x) for x in re.search(r"^BAD (\d+) (\d+)$", out, re.M).groups())
    counts = [int(x) for x in re.search(r"^COUNTS :(.*)$", out, re.M).group(1).split()]
    tallies = b"".join(bytes.fromhex(m.group(1)) for m in re.finditer(r"^TALLY \d+ ([0-9a-f]+)$", out, re.M))
    return bad, counts, tallies, int(re.search(r"^LEVELS (\d+)$", out, re.M).group(1))


@pytest.fixture(scope="module")
def corpus(oracle, pk):
    """62 oracle-made 2-option ballots: every fifth tampered, 7 groups of which group 4 is empty, four ballots in no group, shuffled"""
    op = oracle.ChoiceParams(pk, 2, True)
    n, n_groups = 62, 7
    raw = bytearray(op.generate_batch(2024, 0, n, threads=2))
    for b in range(0, n, 5):
        raw[b * op.ballot_size + 32 * (b % 9) + 5] ^= 0x40
    rng = random.Random(62)
    order = list(range(n))
    rng.shuffle(order)
    ballots = b"".join(bytes(raw[b * op.ballot_size:(b + 1) * op.ballot_size]) for b in order)
    status = op.verify_batch(ballots, threads=2)
    live = [0, 1, 2, 3, 5, 6]
    groups = [live[rng.randrange(6)] if rng.random() < 0.7 else 1 for _ in range(n)]          # group 1 holds about a third
    for b in rng.sample(range(n), 4):
        groups[b] = G.GROUP_NONE
    assert 0 < sum(1 for s in status if s) < n and 4 not in groups
    return op, ballots, status, groups, n_groups


@pytest.mark.parametrize("s1,s2", [(2, 2), (3, 2)])
def test_pipeline_on_the_host_equals_the_oracle_per_group(check, corpus, tmp_path, s1, s2):
    """(c) count, scan, fill, sum from the wire, sum of partial sums, encode - the lane functions of the kernels, serially - give the
    oracle's tally of every group's subset byte for byte, and exact counts; six levels deep with pieces of two"""
    op, ballots, status, groups, n_groups = corpus
    _write_case(tmp_path / "case.txt", op, ballots, status, groups, n_groups)
    bad, counts, tallies, levels = _report(check("run", tmp_path / "case.txt", s1, s2))
    want, want_counts = G.expected(op, ballots, status, groups, n_groups)
    assert bad == (0, 0) and counts == want_counts and counts[4] == 0
    assert tallies == want
    assert tallies[4 * 128:5 * 128] == bytes(128)              # Ciphertext::zero() for the empty group
    assert levels == G.depth(len(status), s1, s2) >= 5


def test_pipeline_on_the_host_counts_hostile_inputs(check, corpus, tmp_path, rejections):
    """an accepted ballot with the id n_groups and a forged status 0 over the reference's rejecting encoding give bad = (1, 1); the same
    two things on REJECTED ballots are never looked at: bad = (0, 0) and the tallies of the rest are the oracle's"""
    op, ballots, status, groups, n_groups = corpus
    non_element = bytes.fromhex(rejections["non_element"]["hex"])
    accepted = [b for b, s in enumerate(status) if s == 0 and groups[b] != G.GROUP_NONE]
    rejected = [b for b, s in enumerate(status) if s != 0]
    # on accepted ballots
    st, gr, by = list(status), list(groups), bytearray(ballots)
    gr[accepted[0]] = n_groups
    by[accepted[1] * op.ballot_size + 32:accepted[1] * op.ballot_size + 64] = non_element          # tally item 1, status left at 0
    assert op.verify_batch(bytes(by))[accepted[1]] != 0                                             # forged: no verifier accepts it
    _write_case(tmp_path / "hostile.txt", op, bytes(by), st, gr, n_groups)
    bad, counts, _, _ = _report(check("run", tmp_path / "hostile.txt", 2, 2))
    assert bad == (1, 1)
    assert sum(counts) == len(accepted) - 1
    # on rejected ballots
    st, gr, by = list(status), list(groups), bytearray(ballots)
    gr[rejected[0]] = n_groups
    gr[rejected[2]] = 0xFFFFFFFE
    by[rejected[1] * op.ballot_size + 32:rejected[1] * op.ballot_size + 64] = non_element
    _write_case(tmp_path / "ignored.txt", op, bytes(by), st, gr, n_groups)
    bad, counts, tallies, _ = _report(check("run", tmp_path / "ignored.txt", 2, 2))
    want, want_counts = G.expected(op, ballots, status, groups, n_groups)
    assert bad == (0, 0) and counts == want_counts and tallies == want


# ------------------------------------------------------------------ merging grouped tallies of two ranks
def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from elastic_elgamal_amd import distributed as egd
    from oracle import oracle as o
    import group_tally_cases as cases

    _, pk, _ = o.keypair_from_seed(12345)
    op = o.ChoiceParams(pk, 2, True)
    total, n_groups = 23, 3
    lo, hi = egd.shard_range(total, rank, world)
    ballots = op.generate_batch(909, lo, hi - lo, threads=2)
    st = op.verify_batch(ballots, threads=2)
    groups = [(lo + i) % n_groups for i in range(hi - lo)]
    local, _ = cases.expected(op, ballots, st, groups, n_groups)               # this rank's grouped tally: n_groups x n_options x 64
    gathered = egd.gather_tallies(torch.frombuffer(bytearray(local), dtype=torch.uint8))
    assert gathered.shape == (world, n_groups * 128)
    merged = []
    for k in range(n_groups * 4):                                              # what eg_points_sum_device(ctx, world, n_groups * 2 * n_options) does
        acc = b"\0" * 32
        for r in range(world):
            acc = o.point_add(acc, bytes(gathered[r, 32 * k:32 * k + 32].numpy()))
        merged.append(acc)
    q.put((rank, b"".join(merged)))
    dist.destroy_process_group()


def test_grouped_tallies_of_two_ranks_merge_through_gather_tallies(oracle, pk):
    """distributed.gather_tallies takes a grouped tally unchanged (it gathers any flat byte tensor): two gloo ranks exchange their grouped
    tallies, and the point-wise sum is the grouped tally of the whole batch"""
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    op = oracle.ChoiceParams(pk, 2, True)
    whole = op.generate_batch(909, 0, 23, threads=2)
    want, _ = G.expected(op, whole, op.verify_batch(whole, threads=2), [i % 3 for i in range(23)], 3)
    assert res[0][1] == res[1][1] == want
