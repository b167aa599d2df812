"""The ballot-audit pass (eg_*_open_check, eg_*_open_batch) without a GPU:
* the surface: the ten symbols declared, exported, bound, mirrored and in INTEGRATION.md; the constants in the header, the Python mirror,
  open_host.hpp and the model; ABI version 7; plain C99; no environment knob and no waiting loop in the device code;
* the model tests/open_ref.py over the oracle's primitives, and a handful of cases a second time over tests/pyref's group;
* the positions at which the generators draw the encryption randomness: the oracle's own draw trace against open_host.hpp's functions
  (through the host check binary), and the scalar at that position of the untouched stream opening the ballot under the model.  The GPU
  provers are byte-identical to the oracle's (existing tests), so this pins the opener's positions;
* tests/hostcheck/opencheck.cpp: open_host.hpp and the lane functions of open_kernels.cuh under ASan + UBSan over true openings, pinned
  edge scalars, every forgery, poisoned inputs of ballots that do not participate, aliased status words, with check 1 compiled out, and
  the halved-scalar encoder against a plain one on every point;
* every refusal of the new entries that needs no GPU."""
import ctypes as C
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import open_cases as K
import open_ref as R

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
BAD_ARG = -3
L = R.L
ENTRIES = {  # name: (return type in the header, restype, number of arguments)
    "eg_choice_open_check_scratch_bytes": ("size_t", C.c_size_t, 2),
    "eg_choice_open_check_device": ("int", C.c_int, 10),
    "eg_choice_open_check": ("int", C.c_int, 8),
    "eg_qv_open_check_scratch_bytes": ("size_t", C.c_size_t, 2),
    "eg_qv_open_check_device": ("int", C.c_int, 10),
    "eg_qv_open_check": ("int", C.c_int, 8),
    "eg_choice_open_batch_device": ("int", C.c_int, 10),
    "eg_choice_open_batch": ("int", C.c_int, 9),
    "eg_qv_open_batch_device": ("int", C.c_int, 9),
    "eg_qv_open_batch": ("int", C.c_int, 8),
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
    for phrase in ("THE RULE", "SPOILING", "EG_DUP_PRIOR", "The FIRST failure wins", "Nothing of the ballot is decoded", "STATELESS as weeding",
                   "VARIABLE TIME like the generators", "EG_OPEN_DETAIL(slot, check)"):
        assert phrase in header, phrase
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        for m in ("open_check", "open_check_device", "open_check_scratch_bytes", "open_batch", "open_batch_device"):
            assert callable(getattr(cls, m)), m
    ffi = (ROOT / "INTEGRATION.md").read_text()
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    for name in ENTRIES:
        assert f"pub fn {name}(" in ffi, name
        if not name.endswith("open_batch_device"):
            assert f"{name}(" in hpp, name


def test_constants_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    host = (CSRC / "open_host.hpp").read_text()
    assert int(re.search(r"EG_ST_BAD_OPENING = (\d+)", header).group(1)) == eg.ST_BAD_OPENING == R.ST_BAD_OPENING == 17
    assert "ST_BAD_OPENING = 17;" in host
    for name, model in (("BAD_SCALAR", R.OPEN_BAD_SCALAR), ("R", R.OPEN_R), ("B", R.OPEN_B)):
        value = int(re.search(rf"EG_OPEN_{name} = (\d+)", header).group(1))
        assert value == getattr(eg, "OPEN_" + name) == model, name
        assert re.search(rf"\bOPEN_{name} = {value};", host), name
    assert (R.OPEN_BAD_SCALAR, R.OPEN_R, R.OPEN_B) == (1, 2, 3)
    assert re.search(r"#define EG_OPEN_ITEMS_MAX \(1u << 31\)", header) and eg.OPEN_ITEMS_MAX == R.ITEMS_MAX == 1 << 31 and "ITEMS_MAX = 1ull << 31;" in host
    for slot, check in ((0, 1), (3, 3), (3999, 2)):
        assert R.status_word(slot, check) == eg.ST_BAD_OPENING | eg.open_detail(slot, check) << 8 and R.detail(R.status_word(slot, check)) == (slot, check)
        assert eg.status_kind(R.status_word(slot, check)) == 17 and eg.status_detail(R.status_word(slot, check)) == slot * 4 + check
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7


def test_cpp_mirror_compiles_and_the_macros_agree_with_the_model(tmp_path):
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace %s;
        int main() {
          Opening o; Audited a;
          (void)&ChoiceParams::open_check; (void)&ChoiceParams::open_batch; (void)&ChoiceParams::open_check_device; (void)&ChoiceParams::open_check_scratch_bytes;
          (void)&QuadraticVotingParams::open_check; (void)&QuadraticVotingParams::open_batch; (void)&QuadraticVotingParams::open_check_device;
          const uint32_t w = EG_ST_BAD_OPENING | EG_OPEN_DETAIL(7, EG_OPEN_B) << 8;
          return o.values.empty() && a.failed == 0 && w == %du && EG_STATUS_KIND(w) == 17 && EG_OPEN_DETAIL_SLOT(EG_STATUS_DETAIL(w)) == 7 &&
                 EG_OPEN_DETAIL_CHECK(EG_STATUS_DETAIL(w)) == EG_OPEN_B ? 0 : 1;
        }
        """ % (ns, R.status_word(7, R.OPEN_B))))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_ST_BAD_OPENING == 17 && EG_OPEN_B == 3 && EG_OPEN_DETAIL(2, EG_OPEN_R) == 10 && '
                   'EG_OPEN_ITEMS_MAX > 5 && eg_choice_open_check_scratch_bytes && eg_choice_open_check_device && eg_choice_open_check && '
                   'eg_qv_open_check_scratch_bytes && eg_qv_open_check_device && eg_qv_open_check && eg_choice_open_batch && '
                   'eg_choice_open_batch_device && eg_qv_open_batch && eg_qv_open_batch_device ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-address", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob_and_no_waiting_between_lanes():
    for f in ("open_kernels.cuh", "open_host.hpp", "open_gen_kernels.cuh"):
        assert "getenv" not in (CSRC / f).read_text()
    kernels = (CSRC / "open_kernels.cuh").read_text()
    device = kernels[kernels.index("#if defined(__HIPCC__)"):]
    # the kernel boundary is the only synchronisation: no loop that waits, no fence, no atomic in the check kernel
    assert not re.search(r"\bwhile\b", device) and "__threadfence" not in device and "__builtin_amdgcn_fence" not in device and "atomicCAS" not in device
    check = device[device.index("k_open_check("):device.index("k_open_resolve(")]
    assert not re.search(r"\batomic\w+\(", check)
    src = (CSRC / "eg_hip.hip").read_text()
    body = src[src.index("static uint32_t open_slots("):src.index("// CommitmentEquivalenceProof::new per item")]
    assert "EG_LOCK" not in body and "ws_acquire" not in body and "gen_workspace" not in body       # stateless: no lock, no workspace


# ------------------------------------------------------------------ the model, twice
@pytest.fixture(scope="module")
def keys(oracle):
    sk, pk, _ = oracle.keypair_from_seed(12345)
    return sk, pk


@pytest.fixture(scope="module")
def group(oracle, keys):
    return R.oracle_group(oracle, keys[1])


EDGE_PAIRS = [(0, 0), (1, 0), ((1 << 64) - 1, 0), (0, 1), (1, 1), ((1 << 64) - 1, 1), (0, L - 1), (1, L - 1), ((1 << 64) - 1, L - 1)]


def test_model_agrees_over_two_groups_and_knows_the_identity(oracle, keys, group):
    second = R.pyref_group(keys[1])
    for v, r in [(0, 0), (1, 1), ((1 << 64) - 1, L - 1), (3, 0x1234567890ABCDEF << 100)]:
        assert group.encrypt(v, r) == second.encrypt(v, r), (v, r)
    assert group.encrypt(0, 0) == (bytes(32), bytes(32))              # the identity encodes as 32 zero bytes
    c = K.bare_choice(oracle, keys[1], 128, [(5, 77), (0, 0)])
    for g in (group, second):
        assert R.check_ballot(g, c.ballot, [0, 64], c.values, c.rands) == 0
        assert R.check_ballot(g, c.ballot, [0, 64], [5, 1], c.rands) == R.status_word(1, R.OPEN_B)
        assert R.check_ballot(g, c.ballot, [0, 64], c.values, [c.rands[1], c.rands[1]]) == R.status_word(0, R.OPEN_R)
        assert R.check_ballot(g, c.ballot, [0, 64], c.values, [(77 + L).to_bytes(32, "little"), c.rands[1]]) == R.status_word(0, R.OPEN_BAD_SCALAR)


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("opencheck") / "opencheck"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), str(HERE / "opencheck.cpp")])

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout

    return run


def parse(out):
    got = {}
    for line in out.splitlines():
        if " :" in line:
            name, _, rest = line.partition(" :")
            got[name] = [int(x) for x in rest.split()]
        elif line.startswith("ENCODED"):
            got["ENCODED"] = int(line.split()[1])
    return got


CHOICE_SHAPES = [  # (single, n_options, chosen)
    (True, 2, [0, 1]), (True, 5, [0, 0, 1, 0, 0]), (True, 33, [0] * 32 + [1]),
    (False, 16, [1 if k in (0, 7, 15) else 0 for k in range(16)]), (False, 4, [0, 0, 0, 0]),
]
QV_SHAPES = [(2, 7, [[0, 0], [1, 0], [0, 2], [2, 1]]), (5, 20, [[0, 0, 0, 0, 0], [1, 0, 1, 0, 1], [0, 4, 0, 0, 0], [2, 2, 2, 2, 2]])]


@pytest.fixture(scope="module")
def oracle_piles(oracle, keys):
    """per shape: (name, stride, slots, [Opened], [trace positions], [(kind, rng_skip, what the positions depend on)])"""
    piles = []
    for single, no, chosen in CHOICE_SHAPES:
        op = oracle.ChoiceParams(keys[1], no, single)
        cases, pos, how = [], [], []
        for j, skip in enumerate((0, 1, 5)):
            c, p = K.oracle_choice(oracle, op, 1000 + 17 * no + j, chosen, skip)
            cases.append(c), pos.append(p), how.append(("choice", skip, chosen))
        piles.append((f"{'single' if single else 'multi'}{no}", op.ballot_size, R.choice_slots(no), cases, pos, how))
    for no, credits, votes in QV_SHAPES:
        op = oracle.QvParams(keys[1], no, credits)
        cases, pos, how = [], [], []
        for j, v in enumerate(votes):
            c, p = K.oracle_qv(oracle, op, 2000 + 31 * no + j, v, j)
            cases.append(c), pos.append(p), how.append(("qv", j, op.vote_range.rings))
        piles.append((f"qv{no}", op.ballot_size, R.qv_slots(no, op.vote_size), cases, pos, how))
    return piles


def test_draw_positions_against_the_oracle_trace(oracle_piles, check, group):
    for name, stride, slots, cases, positions, how in oracle_piles:
        for c, pos, (kind, skip, arg) in zip(cases, positions, how):
            if kind == "choice":
                want = R.choice_r_draws(skip, arg)
                got = parse(check("draws", "choice", skip, "".join(str(int(x)) for x in arg)))["DRAWS"]
            else:
                want = R.qv_r_draws(skip, len(slots), arg)
                got = parse(check("draws", "qv", skip, len(slots), len(arg), sum(size for size, _ in arg)))["DRAWS"]
            assert pos == want == got, (name, skip)
            # the scalar at that position of the untouched stream opens the ballot
            assert R.check_ballot(group, c.ballot, slots, c.values, c.rands) == 0, name
    assert R.qv_r_draws(0, 2, [(3, 1)]) == [0, 4] and R.choice_r_draws(1, [0, 1, 0]) == [1, 4, 6]


def test_lane_functions_accept_true_openings_of_every_shape(oracle_piles, check, keys, tmp_path):
    for name, stride, slots, cases, _, _ in oracle_piles:
        got = parse(check("run", K.write_case(tmp_path / f"{name}.txt", keys[1], stride, slots, cases)))
        assert got["STATUS"] == got["NOGUARD"] == [0] * len(cases) and got["FOUND"] == [len(cases), 0], name
        assert got["ENCODED"] == 2 * len(cases) * len(slots)


def test_lane_functions_at_the_edge_scalars(oracle, keys, group, check, tmp_path):
    size = 64 * 3 + 96
    cases = [K.bare_choice(oracle, keys[1], size, EDGE_PAIRS[i:i + 3]) for i in (0, 3, 6)]
    slots = R.choice_slots(3)
    assert cases[0].ballot[:64] == bytes(64) and cases[0].rands[0] == bytes(32)          # r = v = 0: the identity, twice
    want, found = K.model(group, cases, slots)
    assert want == [0, 0, 0]
    got = parse(check("run", K.write_case(tmp_path / "edge.txt", keys[1], size, slots, cases)))
    assert got["STATUS"] == want and got["FOUND"] == found


def planted(oracle, keys):
    """a pile of single-choice ballots of five options: every forgery at a slot of its own, two failures in one ballot, another ballot's
    opening, and ballots that do not participate"""
    op = oracle.ChoiceParams(keys[1], 5, True)
    slots = R.choice_slots(5)
    true = [K.oracle_choice(oracle, op, 3000 + i, [int(k == i % 5) for k in range(5)], i % 3)[0] for i in range(len(K.FORGERIES) + 6)]
    cases = [c.copy() for c in true]
    names = {}
    for i, f in enumerate(K.FORGERIES):
        f(cases[i], (2 * i) % 5, slots)
        names[i] = f.__name__
    k = len(K.FORGERIES)
    K.forge_v_plus_1(cases[k], 3, slots), K.forge_r_plus_1(cases[k], 1, slots)              # the lower slot wins
    K.forge_flip_wire_b(cases[k + 1], 2, slots), K.forge_flip_wire_r(cases[k + 1], 2, slots)  # R wins over B
    K.forge_flip_wire_r(cases[k + 2], 4, slots), K.forge_r_all_ones(cases[k + 2], 4, slots)   # the scalar wins over R
    K.forge_other_opening(cases[k + 3], true[k + 4])
    return op, slots, true, cases, names, k


def test_lane_functions_reject_every_forgery_with_the_model_s_word(oracle, keys, group, check, tmp_path):
    op, slots, true, cases, names, k = planted(oracle, keys)
    want, found = K.model(group, cases, slots)
    by_name = {names[i]: want[i] for i in names}
    assert by_name["forge_r_plus_1"] == R.status_word(0, R.OPEN_R) and by_name["forge_v_plus_1"] == R.status_word(2, R.OPEN_B)
    assert by_name["forge_v_minus_1"] == R.status_word(4, R.OPEN_B) and by_name["forge_r_plus_l"] == R.status_word(1, R.OPEN_BAD_SCALAR)
    assert by_name["forge_r_all_ones"] == R.status_word(3, R.OPEN_BAD_SCALAR) and by_name["forge_flip_wire_r"] == R.status_word(2, R.OPEN_R)
    assert by_name["forge_flip_wire_b"] == R.status_word(4, R.OPEN_B) and R.detail(by_name["forge_swap_slots"])[1] == R.OPEN_R
    assert want[k] == R.status_word(1, R.OPEN_R) and want[k + 1] == R.status_word(2, R.OPEN_R) and want[k + 2] == R.status_word(4, R.OPEN_BAD_SCALAR)
    assert want[k + 3] == R.status_word(0, R.OPEN_R) and want[k + 4] == want[k + 5] == 0 and found == [len(cases), len(cases) - 2]
    got = parse(check("run", K.write_case(tmp_path / "forged.txt", keys[1], op.ballot_size, slots, cases)))
    assert got["STATUS"] == want and got["FOUND"] == found
    # with check 1 compiled out, r + l passes: the range check is the only guard against the second form of an opening
    i = [j for j in names if names[j] == "forge_r_plus_l"][0]
    assert got["NOGUARD"][i] == 0 and got["STATUS"][i] != 0
    assert [w for j, w in enumerate(got["NOGUARD"]) if j not in (i, 4, k + 2)] == [w for j, w in enumerate(want) if j not in (i, 4, k + 2)]


@pytest.mark.parametrize("alias", [0, 1])
def test_lane_functions_never_read_ballots_that_do_not_participate(oracle, keys, group, check, tmp_path, alias):
    op, slots, true, cases, names, k = planted(oracle, keys)
    status_in = [0] * len(cases)
    for b, word in ((1, 2 | 7 << 8), (5, 14), (k + 4, 16 | 1 << 8), (len(cases) - 1, 6)):
        status_in[b] = word
    want, found = K.model(group, cases, slots, status_in)
    assert [want[b] for b in (1, 5, k + 4)] == [2 | 7 << 8, 14, 16 | 1 << 8] and found[0] == len(cases) - 4
    got = parse(check("run", K.write_case(tmp_path / f"part{alias}.txt", keys[1], op.ballot_size, slots, cases, status_in, alias=bool(alias))))
    assert got["STATUS"] == want and got["FOUND"] == found


def test_hostcheck_layout_against_a_direct_count(check):
    def up(x):
        return (x + 255) // 256 * 256

    for n, n_slots in ((0, 5), (1, 1), (1, 5), (63, 5), (64, 16), (65, 33), (1000, 40), (1 << 20, 5), ((1 << 31) - 1, 1)):
        out = check("layout", n, n_slots)
        assert out.splitlines()[0] == f"LAYOUT words 0 total {up(4 * n * n_slots)}", (n, n_slots)


def test_hostcheck_argument_rules(check):
    def why(n, mask, n_slots, quads=0, w64=0, w32=0):
        return check("refuse", n, mask, n_slots, quads, w64, w32).splitlines()[0]

    assert why(0, 0, 5) == "REFUSE -" and why(1000, 31, 5) == "REFUSE -" and why((1 << 31) - 1, 31, 1) == "REFUSE -"
    assert why(1 << 31, 31, 1) == "REFUSE n is 2^31 or more"
    for missing in range(5):
        assert "null ballots, values, rand, status_out or found" in why(1, 31 & ~(1 << missing), 5)
    assert "n x n_slots is above EG_OPEN_ITEMS_MAX" in why(1 << 30, 31, 3) and why(1 << 30, 31, 2) == "REFUSE -"
    assert "16-byte aligned" in why(1, 31, 5, quads=8) and "8-byte aligned" in why(1, 31, 5, w64=4) and "4-byte aligned" in why(1, 31, 5, w32=2)


# ------------------------------------------------------------------ refusals of the library without a GPU
def test_every_refusal_that_needs_no_gpu():
    lib = eg._load()
    buf = C.create_string_buffer(4096)
    a = C.addressof(buf)
    a += -a % 256
    err = lambda: lib.eg_last_error().decode() if hasattr(lib, "eg_last_error") else ""
    lib.eg_last_error.restype = C.c_char_p
    for prefix in ("choice", "qv"):
        host, dev, size = getattr(lib, f"eg_{prefix}_open_check"), getattr(lib, f"eg_{prefix}_open_check_device"), getattr(lib, f"eg_{prefix}_open_check_scratch_bytes")
        assert size(None, 5) == 0
        assert host(None, 1 << 31, a, None, a, a, a, a) == BAD_ARG and "2^31" in err()
        assert dev(None, 1 << 31, a, None, a, a, a, a, a, None) == BAD_ARG and "2^31" in err()
        for missing in range(5):
            args = [a, a, a, a, a]
            args[missing] = None
            assert host(None, 1, args[0], None, args[1], args[2], args[3], args[4]) == BAD_ARG and "null ballots" in err(), missing
            assert dev(None, 1, args[0], None, args[1], args[2], args[3], args[4], a, None) == BAD_ARG and "null ballots" in err(), missing
        assert dev(None, 1, a + 8, None, a, a, a, a, a, None) == BAD_ARG and "16-byte" in err()
        assert dev(None, 1, a, None, a, a, a, a, a + 8, None) == BAD_ARG and "16-byte" in err()
        assert dev(None, 1, a, None, a + 4, a, a, a, a, None) == BAD_ARG and "8-byte" in err()
        for k in range(4):                                         # rand, status_in, status_out, found
            ptrs = [a, a, a, a]
            ptrs[k] += 2
            assert dev(None, 1, a, ptrs[1], a, ptrs[0], ptrs[2], ptrs[3], a, None) == BAD_ARG and "4-byte" in err(), k
        assert host(None, 1, a, None, a, a, a, a) == BAD_ARG and "null params" in err()
        assert dev(None, 1, a, None, a, a, a, a, a, None) == BAD_ARG and "null params" in err()
        assert host(None, 0, None, None, None, None, None, None) == BAD_ARG and "null params" in err()      # n == 0 still needs a params object
    for fn, lead in ((lib.eg_choice_open_batch, (None, 1, 0)), (lib.eg_qv_open_batch, (None, 1, 0))):
        tail = (0, 0) if fn is lib.eg_choice_open_batch else (0,)
        assert fn(lead[0], lead[1], lead[2], 1 << 31, *tail, None, a, a) == BAD_ARG and "2^31" in err()
        assert fn(lead[0], lead[1], lead[2], 1, *tail, None, None, a) == BAD_ARG and "null values_out or rand_out" in err()
        assert fn(lead[0], lead[1], lead[2], 1, *tail, None, a, None) == BAD_ARG and "null values_out or rand_out" in err()
        assert fn(lead[0], lead[1], lead[2], 1, *tail, None, a, a) == BAD_ARG and "null params" in err()
    for fn, tail in ((lib.eg_choice_open_batch_device, (0, 0)), (lib.eg_qv_open_batch_device, (0,))):
        assert fn(None, 1, 0, 1 << 31, *tail, None, a, a, None) == BAD_ARG and "2^31" in err()
        assert fn(None, 1, 0, 1, *tail, None, None, a, None) == BAD_ARG and "null values_out" in err()
        assert fn(None, 1, 0, 1, *tail, None, a + 4, a, None) == BAD_ARG and "8-byte" in err()
        assert fn(None, 1, 0, 1, *tail, None, a, a + 2, None) == BAD_ARG and "4-byte" in err()
        assert fn(None, 1, 0, 1, *tail, None, a, a, None) == BAD_ARG and "null params" in err()
