"""The batched share combination (eg_combine_shares_batch*, csrc/share_combine_kernels.cuh, csrc/share_combine_host.hpp) without a GPU.

* tests/share_combine_ref.py - lagrange_coefficients and combine_shares restated on the oracle - gives [x]R for Shamir key sets.
* The three entry points are declared, exported, bound in Python and mirrored in C++; ABI version 7; the header stays plain C; no knob.
* Every refusal that needs no GPU, from both entries, and a loud failure without one.
* tests/hostcheck/sharecombinecheck.cpp: the lane functions of the three stages, -DEG_BOUNDCHECK under ASan + UBSan: (a) coefficients
  against the restatement; (b) the whole pipeline over oracle-made shares, rejected, transplanted, wrong and undecodable shares;
  (c) the scratch layout against a direct count.
Every expected value comes from the CPU oracle."""
import ctypes as C
import itertools
import random
import re
import subprocess
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg
import share_combine_ref as R
from elastic_elgamal_amd import tally as T

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
BAD_ARG = -3
SIZE, DEVICE, HOST = "eg_combine_shares_batch_scratch_bytes", "eg_combine_shares_batch_device", "eg_combine_shares_batch"
sc = R.sc


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shares_n,threshold", [(1, 1), (3, 2), (10, 7), (64, 64)])
def test_restatement_gives_the_shared_keys_decryption(oracle, shares_n, threshold):
    """combine_shares of the restatement over t shares of a Shamir key set is [x]R for the shared secret x, whatever subset of the
    participants and whatever order"""
    ks = R.KeySet(oracle, shares_n, threshold, 2024 + shares_n)
    rnd = random.Random(shares_n)
    Rs = [oracle.point_mul_generator(sc(rnd.randrange(1, R.L))) for _ in range(2)]
    subsets = [list(range(threshold)), list(range(shares_n - threshold, shares_n))[::-1]]
    subsets += [rnd.sample(range(shares_n), threshold) for _ in range(3)]
    for Re in Rs:
        want = oracle.point_multi_mul(sc(ks.secret), Re)
        for subset in subsets:
            given = [(i, ks.dh(oracle, i, Re)) for i in subset]
            assert R.combine_shares(oracle, shares_n, threshold, given) == want, subset
            assert R.combine_shares(oracle, shares_n, threshold, given + given[:1]) == want          # .take(threshold)
            assert R.combine_shares(oracle, shares_n, threshold, given[:-1]) is None
    if threshold < shares_n:          # one share of t replaced by a wrong element: another result
        given = [(i, ks.dh(oracle, i, Rs[0])) for i in subsets[0]]
        given[0] = (given[0][0], Rs[1])
        assert R.combine_shares(oracle, shares_n, threshold, given) != oracle.point_multi_mul(sc(ks.secret), Rs[0])


# ------------------------------------------------------------------ surface
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for name, ret, restype, nargs in ((SIZE, "size_t", C.c_size_t, 2), (DEVICE, "int", C.c_int, 16), (HOST, "int", C.c_int, 13)):
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in eg.exported_symbols()
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    # in the tally-stage section, directly behind the entry it batches
    at = header.index(SIZE + "(")
    assert header.index("int eg_combine_shares(") < at < header.index("int eg_dlog_table_create(")
    assert re.search(r"^#define EG_COMBINE_SHARES_MAX 64\b", header, re.M) and T.COMBINE_SHARES_MAX == 64
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert lib.eg_abi_version() == 7


def test_python_and_cpp_mirrors_exist(tmp_path):
    assert callable(T.combine_shares_batch) and callable(T.combine_shares_batch_device) and callable(T.decrypt_tallies)
    assert callable(T.combine_shares_batch_scratch_bytes)
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count("inline CombinedShares combine_shares_batch(") == 1 and hpp.count("inline DecryptedTallies decrypt_tallies(") == 1
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace NS;
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element key{};
            CombinedShares a = combine_shares_batch(ctx, 3, 2, Bytes(), {0, 1}, Bytes());
            CombinedShares b = combine_shares_batch(ctx, 3, 2, Bytes(), {0, 1}, Bytes(), std::vector<uint32_t>());
            combine_shares_batch_device(ctx, 3, 2, 0, nullptr, {0, 1}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            combine_shares_batch_device(ctx, 3, 2, 0, nullptr, {0, 1}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            DecryptionShares v0(ctx, key, 3, 2, 0, key), v1(ctx, key, 3, 2, 1, key);
            DiscreteLogSolver solver(ctx);
            DecryptedTallies d = decrypt_tallies(ctx, 3, 2, Bytes(), {{0, &v0}, {1, &v1}}, {Bytes(), Bytes()}, solver, 0, 100);
            return (int)(a.dh.size() + b.plain.size() + a.combined.size() + b.used.size() + d.values.size() + d.combined.size() + d.used.size() +
                         combine_shares_batch_scratch_bytes(2, 5));
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
    src.write_text('#include "eg_hip.h"\nint main(void) { return eg_combine_shares_batch && eg_combine_shares_batch_device && '
                   'eg_combine_shares_batch_scratch_bytes && EG_COMBINE_SHARES_MAX == 64 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_new_environment_knob():
    src = (CSRC / "eg_hip.hip").read_text()
    a, b = src.index("static Knobs read_knobs()"), src.index("// Fault points:")
    assert len(set(re.findall(r'"(EG_[A-Z_]+)"', src[a:b]))) == 16
    a, b = src.index("static int combine_batch_check("), src.index("// DiscreteLogTable (src/encryption.rs:260-298)")
    assert "getenv" not in src[a:b] and "EG_LOCK" not in src[a:b] and "ws_acquire" not in src[a:b]      # stateless: no knob, no lock, no workspace
    a = src.index("int eg_combine_shares_batch_device(")
    device = src[a:src.index("// host buffers, staged into device memory of the call's own")]
    assert "hipMalloc" not in device and "Synchronize" not in device                                      # allocates nothing, never waits
    for f in ("share_combine_kernels.cuh", "share_combine_host.hpp"):
        assert "getenv" not in (CSRC / f).read_text()


# ------------------------------------------------------------------ refusals that need no GPU
def _entries():
    lib = eg._load()
    buf = C.create_string_buffer(4096 + 64)
    p = (C.addressof(buf) + 63) // 64 * 64            # a 64-byte aligned host address: alignment rules pass, nothing is ever launched

    def device(shares, threshold, m, k, indexes, cts=p, items=p, status=p, dh=p, plain=p, combined=p, used=p, bad=p, scratch=p):
        idx = None if indexes is None else (C.c_uint64 * max(len(indexes), 1))(*indexes)
        rc = lib.eg_combine_shares_batch_device(None, shares, threshold, m, cts, k, idx, items, status, dh, plain, combined, used, bad, scratch, None)
        return rc, lib.eg_last_error()

    def host(shares, threshold, m, k, indexes, cts=p, items=p, status=p, dh=p, plain=p, combined=p, used=p, **_):
        idx = None if indexes is None else (C.c_uint64 * max(len(indexes), 1))(*indexes)
        rc = lib.eg_combine_shares_batch(None, shares, threshold, m, cts, k, idx, items, status, dh, plain, combined, used)
        return rc, lib.eg_last_error()

    return (("device", device), ("host", host)), p


def test_refusals_of_the_host_and_device_entries_without_a_gpu():
    """argument checks come before any device work and before the context is looked at; arguments that pass them fail on the missing
    context; the scratch size of a refused call is 0"""
    entries, p = _entries()
    for name, call in entries:
        for shares in (0, 65, 1 << 40):
            rc, msg = call(shares, 1, 5, 1, [0])
            assert rc == BAD_ARG and b"EG_COMBINE_SHARES_MAX" in msg, (name, shares)
        for shares, threshold in ((3, 0), (3, 4), (64, 65), (1, 2)):
            rc, msg = call(shares, threshold, 5, 1, [0])
            assert rc == BAD_ARG and b"threshold is outside 1..shares" in msg, (name, shares, threshold)
        for k in (-1, 4, 1 << 20):
            rc, msg = call(3, 2, 5, k, [0, 1, 2, 0])
            assert rc == BAD_ARG and b"k is outside 0..shares" in msg, (name, k)
        for indexes in ([0, 3], [3, 0], [0, 1 << 63], [64, 1]):
            rc, msg = call(3, 2, 5, 2, indexes)
            assert rc == BAD_ARG and b"index exceeds" in msg, (name, indexes)
        for indexes in ([1, 1], [0, 2, 0], [2, 1, 1]):
            rc, msg = call(3, 2, 5, len(indexes), indexes)
            assert rc == BAD_ARG and b"duplicate share index" in msg, (name, indexes)
        assert call(64, 64, 5, 64, list(range(63)) + [0])[1] == b"share combine: duplicate share index"
        for m in (1 << 31, 1 << 40):
            rc, msg = call(3, 2, m, 2, [0, 1])
            assert rc == BAD_ARG and b"2^31" in msg, (name, m)
        rc, msg = call(3, 2, 5, 2, None)
        assert rc == BAD_ARG and b"null indexes" in msg, name
        for missing in ("cts", "items", "combined") + (("bad",) if name == "device" else ()):
            rc, msg = call(3, 2, 5, 2, [0, 1], **{missing: None})
            assert rc == BAD_ARG and b"null" in msg and b"pointer" in msg, (name, missing)
        # what passes the argument rules fails on the missing context, loudly
        for args, kw in (((3, 2, 5, 2, [0, 1]), {}), ((3, 2, 5, 1, [2]), {}), ((3, 2, 5, 0, []), dict(items=None)), ((3, 2, 0, 2, [0, 1]), {}),
                         ((3, 2, 0, 0, None), dict(cts=None, items=None, combined=None, bad=None, scratch=None, dh=None, plain=None, used=None, status=None)),
                         ((64, 64, (1 << 31) - 1, 64, list(range(64))), {}), ((1, 1, 1, 1, [0]), {}),
                         ((10, 7, 5, 10, list(range(10))), dict(status=None, dh=None, plain=None, used=None))):
            rc, msg = call(*args, **kw)
            assert rc == BAD_ARG and msg == b"share combine: null context", (name, args, kw, msg)
    device = entries[0][1]
    rc, msg = device(3, 2, 5, 2, [0, 1], scratch=None)
    assert rc == BAD_ARG and b"null scratch" in msg
    for arg in ("cts", "items", "status", "dh", "plain", "combined", "bad", "scratch"):
        for off in (1, 4, 8):
            rc, msg = device(3, 2, 5, 2, [0, 1], **{arg: p + off})
            assert rc == BAD_ARG and b"16-byte aligned" in msg, (arg, off)
    for off in (1, 4):
        rc, msg = device(3, 2, 5, 2, [0, 1], used=p + off)
        assert rc == BAD_ARG and b"8-byte aligned" in msg
    assert device(3, 2, 5, 2, [0, 1], used=p + 8)[1] == b"share combine: null context"
    size = eg._load().eg_combine_shares_batch_scratch_bytes
    for t, m in ((0, 5), (65, 5), (7, 1 << 31), (7, 0)):
        assert size(t, m) == 0 == T.combine_shares_batch_scratch_bytes(t, m), (t, m)
    assert size(7, 5) > 0


def test_missing_gpu_is_loud():
    """what a caller without a context gets: an error, never a result"""
    ct, item = bytes(64), bytes(128)
    with pytest.raises(eg.EgError, match="null context"):
        T.combine_shares_batch(None, 3, 2, ct, [0, 1], item * 2)
    with pytest.raises(eg.EgError, match="null context"):
        T.combine_shares_batch(None, 3, 2, ct, [0, 1], item * 2, [0, 0])
    with pytest.raises(eg.EgError, match="null context"):
        T.combine_shares_batch_device(None, 3, 2, 1, 64, [0, 1], 64, 0, 64, 64, 64)
    with pytest.raises(eg.EgError, match="duplicate share index"):
        T.combine_shares_batch(None, 3, 2, ct, [1, 1], item * 2)
    with pytest.raises(eg.EgError, match="threshold"):
        T.combine_shares_batch(None, 3, 4, ct, [0, 1], item * 2)
    with pytest.raises(ValueError):
        T.combine_shares_batch(None, 3, 2, ct, [0, 1], item)
    with pytest.raises(ValueError):
        T.combine_shares_batch(None, 3, 2, ct, [0, 1], item * 2, [0])
    with pytest.raises(ValueError):
        T.combine_shares_batch(None, 3, 2, ct[:-1], [0, 1], item * 2)
    with pytest.raises(ValueError):
        T.decrypt_tallies(None, 3, 2, ct, [], [], solver=None, table=None)


# ------------------------------------------------------------------ the host check program
@pytest.fixture(scope="module")
def check():
    exe, src = HERE / "sharecombinecheck", HERE / "sharecombinecheck.cpp"
    deps = [src, *CSRC.glob("*.cuh"), *CSRC.glob("*.hpp"), CSRC / "plan.h"]
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", str(exe), str(src)])

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]
        return r.stdout

    return run


def _coeff_cases(check, oracle, tmp_path, cases):
    """cases: [(column indexes, mask)] -> the lane function's scalars equal scale / denominator_i of the restatement, column by column"""
    (tmp_path / "coeffs.txt").write_text("".join(f"{len(idx)} {mask} {' '.join(map(str, idx))}\n" for idx, mask in cases))
    rows = re.findall(r"^COEF((?: [0-9a-f]{64})+)$", check("coeffs", tmp_path / "coeffs.txt"), re.M)
    assert len(rows) == len(cases)
    for (idx, mask), row in zip(cases, rows):
        chosen = [i for j, i in enumerate(idx) if (mask >> j) & 1]
        assert [bytes.fromhex(x) for x in row.split()] == R.scaled_coefficients(oracle, chosen), (idx, mask)


def test_coefficients_of_every_subset_of_small_key_sets(check, oracle, tmp_path):
    """(a) every 3-subset of the 5 columns of a 3-of-5 key set, under the identity and under two other assignments of participants to
    columns; every subset of 2-of-3 and 1-of-1 .. 1-of-3"""
    cases = []
    for idx in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 4, 1, 0, 2]):
        for cols in itertools.combinations(range(5), 3):
            cases.append((idx, sum(1 << j for j in cols)))
    for idx in ([0, 1, 2], [2, 0, 1]):
        for t in (1, 2, 3):
            for cols in itertools.combinations(range(3), t):
                cases.append((idx, sum(1 << j for j in cols)))
    cases.append(([0], 1))
    _coeff_cases(check, oracle, tmp_path, cases)


def test_coefficients_of_random_subsets_up_to_64_of_64(check, oracle, tmp_path):
    """(a) random subsets of random sizes in random column orders, index sets containing 0 and 63, and t = 1, 8, 9, 16, 17 (both sides of
    the chunk seam) and 10, 11, 20, 21 (both sides of the seam of the small-factor products), up to all 64 of 64"""
    rnd = random.Random(64)
    cases = []
    for t in (1, 8, 9, 10, 11, 16, 17, 20, 21, 33, 63, 64):
        for trial in range(2):
            k = rnd.randint(t, 64)
            idx = rnd.sample(range(64), k)
            cols = sorted(rnd.sample(range(k), t))
            if trial == 0 and t >= 2:          # the extreme participants, chosen
                for want, col in ((0, cols[0]), (63, cols[-1])):
                    if want in idx:
                        idx[idx.index(want)] = idx[col]
                    idx[col] = want
                assert len(set(idx)) == k
            cases.append((idx, sum(1 << j for j in cols)))
    cases.append((list(range(64)), (1 << 64) - 1))
    cases.append((list(range(63, -1, -1)), (1 << 64) - 1))
    cases.append(([63], 1))
    cases.append(([0, 63], 3))
    _coeff_cases(check, oracle, tmp_path, cases)


# ------------------------------------------------------------------ the whole pipeline, serially
def _write_case(path, shares_n, threshold, cts, indexes, columns, status, want_plain=True):
    m, k = len(cts), len(indexes)
    lines = [f"{shares_n} {threshold} {m} {k} {int(status is not None)} {int(want_plain)}", " ".join(map(str, indexes))]
    for c in range(m):
        lines.append(cts[c].hex())
        for j in range(k):
            lines.append(f"{0 if status is None else status[j][c]} {columns[j][c].hex()}")
    path.write_text("\n".join(lines) + "\n")


def _report(out):
    bad = tuple(int(x) for x in re.search(r"^BAD (\d+) (\d+) (\d+)$", out, re.M).groups())
    rows = re.findall(r"^CT \d+ (\d) (\d+) ([0-9a-f]{64}) ([0-9a-f]{64})$", out, re.M)
    return ([bytes.fromhex(r[2]) for r in rows], [bytes.fromhex(r[3]) for r in rows], [int(r[0]) for r in rows], [int(r[1]) for r in rows], bad)


def _run(check, tmp_path, oracle, shares_n, threshold, cts, indexes, columns, status, want_plain=True):
    _write_case(tmp_path / "case.txt", shares_n, threshold, cts, indexes, columns, status, want_plain)
    got = _report(check("run", tmp_path / "case.txt"))
    want = R.expected(oracle, shares_n, threshold, cts, indexes, columns, status, want_plain)
    assert len(got[0]) == len(cts)
    return got, want


@pytest.fixture(scope="module")
def corpus(oracle):
    """40 ciphertexts of known counts (0 included) under a 7-of-10 key, and all ten participants' oracle-proven share items, the
    columns in a shuffled order of participants"""
    ks = R.KeySet(oracle, 10, 7, 77)
    counts = [0, 1, 2, 59, 60] + list(range(100, 135))
    cts = R.ciphertexts(oracle, ks, counts, 5)
    indexes = random.Random(3).sample(range(10), 10)
    rng = oracle.rng_from_u64(9)
    columns = [[ks.item(oracle, i, ct[:32], rng) for ct in cts] for i in indexes]
    for j, i in enumerate(indexes):
        assert oracle.decryption_share_verify(ks.part_keys[i], 10, 7, ks.shared_key, i, columns[j][0]) == 0
    return ks, counts, cts, indexes, columns


def _all_ok(k, m):
    return [[0] * m for _ in range(k)]


def test_pipeline_on_the_host_opens_every_ciphertext(check, oracle, corpus, tmp_path):
    """(b) select, coefficients, combine, finish - the lane functions of the kernels, serially: dh = [x]R and plain = [count]G for all
    40 ciphertexts (32 zero bytes for the count 0, with combined = 1), used = the first seven columns' participants; the same with no
    status words, with seven columns only, and - every combined 0 - with six"""
    ks, counts, cts, indexes, columns = corpus
    m = len(cts)
    x_R = [oracle.point_multi_mul(sc(ks.secret), ct[:32]) for ct in cts]
    plains = [oracle.point_mul_generator(sc(v)) for v in counts]
    first7 = sum(1 << i for i in indexes[:7])
    for k, status in ((10, _all_ok(10, m)), (10, None), (7, _all_ok(7, m))):
        got, want = _run(check, tmp_path, oracle, 10, 7, cts, indexes[:k], columns[:k], status)
        assert got == want
        assert got[0] == x_R and got[1] == plains and got[1][0] == bytes(32) and got[2] == [1] * m and got[3] == [first7] * m and got[4] == (0, 0, 0)
    got, want = _run(check, tmp_path, oracle, 10, 7, cts[:5], indexes[:6], [col[:5] for col in columns[:6]], None)
    assert got == want and got[2] == [0] * 5 and got[3] == [0] * 5 and got[0] == got[1] == [bytes(32)] * 5
    got, want = _run(check, tmp_path, oracle, 10, 7, cts[:5], indexes, [col[:5] for col in columns], None, want_plain=False)
    assert got == want and got[0] == x_R[:5] and got[1] == [bytes(32)] * 5


@pytest.mark.parametrize("shares_n,threshold", [(1, 1), (3, 2), (8, 8), (12, 9), (20, 17), (64, 64)])
def test_pipeline_on_the_host_at_other_key_sets(check, oracle, tmp_path, shares_n, threshold):
    """(b) both sides of the chunk seam (8 | 9, 16 | 17) and the largest key set: three ciphertexts each, columns in shuffled order,
    proof-less items (the pass reads R and dh of an item, nothing else)"""
    ks = R.KeySet(oracle, shares_n, threshold, 100 + shares_n)
    counts = [0, 7, 1 << 40]
    cts = R.ciphertexts(oracle, ks, counts, shares_n)
    indexes = random.Random(shares_n).sample(range(shares_n), shares_n)
    columns = [[ks.plain_item(oracle, i, ct[:32]) for ct in cts] for i in indexes]
    got, want = _run(check, tmp_path, oracle, shares_n, threshold, cts, indexes, columns, None)
    assert got == want
    assert got[0] == [oracle.point_multi_mul(sc(ks.secret), ct[:32]) for ct in cts]
    assert got[1] == [oracle.point_mul_generator(sc(v)) for v in counts] and got[2] == [1] * 3 and got[4] == (0, 0, 0)
    assert got[3] == [sum(1 << i for i in indexes[:threshold])] * 3


def test_pipeline_on_the_host_steps_over_rejected_shares(check, oracle, corpus, tmp_path):
    """(b) a rejected status in column 0, in the last needed column, and in enough columns to drop below 7: the walk takes the next
    usable columns, the result is still [x]R, the used mask says which; four rejected columns of ten leave combined = 0.  Items of
    rejected columns are never read (the check program fails if they are)."""
    ks, counts, cts, indexes, columns = corpus
    m = 8
    cts, columns = cts[:m], [col[:m] for col in columns]
    status = _all_ok(10, m)
    status[0][1] = 5                                   # column 0
    status[6][2] = 0x10003                             # the last needed column
    status[0][3] = status[3][3] = status[6][3] = 9     # three: columns 0..9 still hold seven
    for j in (1, 4, 8, 9):
        status[j][4] = 1                               # four: below the threshold
    for j in range(10):
        status[j][5] = 2                               # none at all
    got, want = _run(check, tmp_path, oracle, 10, 7, cts, indexes, columns, status)
    assert got == want and got[4] == (0, 0, 0)
    mask = lambda cols: sum(1 << indexes[j] for j in cols)
    assert got[3] == [mask(range(7)), mask(range(1, 8)), mask([0, 1, 2, 3, 4, 5, 7]), mask([1, 2, 4, 5, 7, 8, 9]), 0, 0, mask(range(7)), mask(range(7))]
    assert got[2] == [1, 1, 1, 1, 0, 0, 1, 1]
    for c in (0, 1, 2, 3, 6, 7):
        assert got[0][c] == oracle.point_multi_mul(sc(ks.secret), cts[c][:32]) and got[1][c] == oracle.point_mul_generator(sc(counts[c]))
    assert got[0][4] == got[1][4] == got[0][5] == got[1][5] == bytes(32)


def test_pipeline_on_the_host_counts_hostile_inputs(check, oracle, corpus, tmp_path, rejections):
    """(b) shares marked accepted that no verifier accepted: one carrying another ciphertext's R (bad[0], skipped, the result still
    [x]R), one with a decodable but wrong dh (the restatement over exactly the first seven usable columns, not [x]R), a dh and a B the
    reference itself rejects (bad[1], bad[2]: combined = 0 and zero bytes); the same things behind the seventh usable column or under a
    rejected status are never looked at"""
    ks, counts, cts, indexes, columns = corpus
    non_element = bytes.fromhex(rejections["non_element"]["hex"])
    assert oracle.point_roundtrip(non_element) is None
    m = 8
    cts, columns = list(cts[:m]), [list(col[:m]) for col in columns]
    status = _all_ok(10, m)
    columns[2][1] = columns[2][0]                                          # ciphertext 1, column 2: a true share of ciphertext 0
    wrong = ks.dh(oracle, indexes[4], cts[0][:32])
    columns[4][2] = columns[4][2][:32] + wrong + columns[4][2][64:]        # ciphertext 2, column 4: R right, dh of another ciphertext
    columns[5][3] = columns[5][3][:32] + non_element + columns[5][3][64:]  # ciphertext 3, column 5: dh does not decode
    cts[4] = cts[4][:32] + non_element                                     # ciphertext 4: B does not decode
    columns[8][5] = columns[8][0]                                          # behind the seventh usable column: never met
    columns[9][5] = columns[9][5][:32] + non_element + bytes(64)
    columns[1][6] = columns[1][0]                                          # under a rejected status: never read
    status[1][6] = 3
    got, want = _run(check, tmp_path, oracle, 10, 7, cts, indexes, columns, status)
    assert got == want and got[4] == (1, 1, 1)
    x_R = [oracle.point_multi_mul(sc(ks.secret), ct[:32]) for ct in cts]
    mask = lambda cols: sum(1 << indexes[j] for j in cols)
    assert got[2] == [1, 1, 1, 0, 0, 1, 1, 1]
    assert got[0][1] == x_R[1] and got[3][1] == mask([0, 1, 3, 4, 5, 6, 7])
    given = [(indexes[j], columns[j][2][32:64]) for j in range(7)]
    assert got[0][2] == R.combine_shares(oracle, 10, 7, given) != x_R[2] and got[3][2] == mask(range(7))
    assert got[0][3] == got[1][3] == got[0][4] == got[1][4] == bytes(32) and got[3][3] == got[3][4] == 0
    assert got[0][5] == x_R[5] and got[0][6] == x_R[6] and got[3][6] == mask([0, 2, 3, 4, 5, 6, 7])
    # without a place for plain, B is not decoded: bad[2] stays 0 and ciphertext 4 is combined
    got, want = _run(check, tmp_path, oracle, 10, 7, cts, indexes, columns, status, want_plain=False)
    assert got == want and got[4] == (1, 1, 0) and got[2][4] == 1 and got[0][4] == x_R[4]


# ------------------------------------------------------------------ scratch layout
@pytest.mark.parametrize("t,m", [(1, 1), (7, 5), (7, 256), (7, 257), (8, 50000), (9, 50000), (33, 1 << 17), (64, (1 << 17) + 1), (7, 1 << 20),
                                 (64, (1 << 31) - 1)])
def test_scratch_layout_against_a_direct_count(check, t, m):
    """(c) per lane of a slab - m rounded up to whole blocks of 256, at most 2^17 - one 8-byte mask, t scalars of 32 bytes and
    min(t, 8) tables of 8 entries of 144 bytes, every part 256-byte aligned; the size function gives the total"""
    row = check("layout", t, m)
    v = dict(zip(*[iter(re.search(r"^LAYOUT (.*)$", row, re.M).group(1).split())] * 2))
    v = {k: int(x) for k, x in v.items()}
    up = lambda x: -(-x // 256) * 256
    lanes = min(up(m), 1 << 17)
    assert (v["lanes"], v["chunk"], v["mask"]) == (lanes, min(t, 8), 0)
    assert v["coef"] == up(8 * lanes) and v["tables"] == v["coef"] + up(32 * t * lanes)
    assert v["total"] == v["tables"] + up(1152 * min(t, 8) * lanes) == v["bytes"] == eg._load().eg_combine_shares_batch_scratch_bytes(t, m)
