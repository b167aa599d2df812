"""The fused square-and-subtract, the chain doubling, the comb product with the sign on the accumulator and the fixed comb's zero-digit
path, on the host compilation of the device headers.

tests/hostcheck/dblchaincheck.cpp is a stand-alone program (its own main), built here with -DEG_BOUNDCHECK and
-fsanitize=address,undefined: every fe carries its class, every operation asserts its precondition, and the sanitizers watch the
arithmetic and the buffers.  The records and scalars, and the reference on Python integers, are in tests/dbl_chain_cases.py.
"""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dbl_chain_cases as dc
import limb_cases as lc

HERE = Path(__file__).resolve().parent / "hostcheck"
CSRC = HERE.parent.parent / "elastic_elgamal_amd" / "csrc"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dblchaincheck") / "dblchaincheck"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEG_BOUNDCHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), str(HERE / "dblchaincheck.cpp")])
    return exe


def run(prog, *args, ok=True):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(prog), *map(str, args)], capture_output=True, text=True, timeout=600, env=env)
    if ok:
        assert r.returncode == 0, (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def run_records(prog, tmp_path, b):
    """the output records (n x 80 words) of the host program for a batch"""
    inp, out = tmp_path / f"{b.name}.in", tmp_path / f"{b.name}.out"
    inp.write_bytes(b.records())
    r = run(prog, "records", b.op, inp, out)
    assert r.stdout.strip() == f"records {len(b)}"
    return np.frombuffer(out.read_bytes(), dtype=np.uint32).reshape(len(b), lc.WORDS)


@pytest.mark.parametrize("name", list(dc.OPS))
def test_records_against_the_integer_reference(prog, tmp_path, name):
    """value mod p, output classes (F and the fused result: class 1), aliasing, and ge_dbl_chain = ge_dbl mod p on every coordinate;
    the program itself re-checks the class-1 outputs with fe_check_values and aborts on any precondition a case would break"""
    b = dc.batch(name)
    fams = set(b.names)
    assert {"top", "slack", "near", "hair", "zero", "unreduced", "onehot", "random"} <= fams
    b.check(run_records(prog, tmp_path, b))


def test_the_class_limit_is_the_column_bound():
    """2 class(f)^2 <= 12.5: at class 2.5 (with the slack fe_check_values admits, and g anywhere below class 4) every column sum of the
    model stays below 2^64 and the corner families come within 5 % of it; the final carry stays below 2^36, so limb 1 is the usual
    hair above its width; with every limb at the top of class 2.6 a column sum passes 2^64.  That the model is the code
    (it gives the very limbs of the build) is test_model_limbs_are_the_builds."""
    b = dc.batch("sq2_sub")
    peak_at_limit = 0
    for row, classes, fam in zip(b.rows, b.classes, b.names):
        limbs, peak, carry, wrap = dc.model_sq2_sub(row[0:9], row[9:18])
        assert peak < 2**64 and carry < 2**36 and wrap <= lc.HAIR_BOUND, (fam, classes, peak / 2**64)
        assert lc.value(limbs) % lc.P == (2 * lc.value(row[0:9]) ** 2 - lc.value(row[9:18])) % lc.P
        if classes[0] == dc.F_LIMIT and fam in lc.CORNER:
            assert peak >= 0.95 * 2**64, (fam, classes, peak / 2**64)
            peak_at_limit = max(peak_at_limit, peak)
    assert 0.975 * 2**64 <= peak_at_limit < 0.98 * 2**64
    over = [lc.top(2.6, i) for i in range(9)]
    assert dc.model_sq2_sub(over, [0] * 9)[1] >= 2**64
    assert 2 * dc.F_LIMIT**2 == 12.5 and max(c[0] for c in b.classes) == dc.F_LIMIT and max(c[1] for c in b.classes) == dc.G_LIMIT


def test_model_limbs_are_the_builds(prog, tmp_path):
    b = dc.batch("sq2_sub")
    out = run_records(prog, tmp_path, b).tolist()
    for r, row in enumerate(b.rows):
        assert dc.model_sq2_sub(row[0:9], row[9:18])[0] == out[r][0:9], (r, b.names[r], b.classes[r])


def test_a_case_outside_the_precondition_is_refused(prog):
    """f at the top of class 2.5 runs; at class 2.6 the bound-check build aborts before the squaring (a child process: the abort is
    the expected end of it)"""
    ok = run(prog, "outside", 2.5)
    assert ok.stdout.startswith("ran ")
    bad = run(prog, "outside", 2.6, ok=False)
    assert bad.returncode == -6 and "fe_sq2_sub: 2 * class(f)^2 > 12.5" in bad.stderr and "ran" not in bad.stdout, (bad.returncode, bad.stderr)


def test_scalar_list_reaches_its_corners():
    sc = dc.comb_scalars()
    by = {}
    for name, k in sc:
        by.setdefault(name, []).append(k)
    assert all(k < 2**253 for _, k in sc) and len(by["random"]) == 200
    for k in by["equal signs"]:                               # nothing but the first doubling negates the accumulator
        neg = dc.column_negations(k)
        assert neg[0] is False and all(neg[1:]), hex(k)
    for name in ("0x55", "0xAA", "0x55 even", "0xAA odd"):
        neg = dc.column_negations(by[name][0])
        flips = sum(a != b for a, b in zip(neg, neg[1:]))
        assert flips >= 45, (name, flips)                       # 50 adjacent pairs; the top columns of a 252-bit pattern are fixed
    neg = dc.column_negations(dc.M55)
    assert all(a != b for a, b in zip(neg[4:], neg[5:]))      # the sign flips in EVERY column under the top of the 251-bit pattern
    assert all(k % 2 == 0 for k in by["even"]) and all(k % 2 == 1 for k in by["odd"])


def test_comb_with_the_sign_on_the_accumulator(prog, tmp_path, oracle):
    """ge_teeth_mul against the entry-negating form with the unfused doubling (compared inside the program, on the Ristretto encoding,
    for the 5 x 51 and the 6 x 43 shape, on a packed host-array table), and against the oracle's [k]P"""
    sc = [k for _, k in dc.comb_scalars()]
    inp, out = tmp_path / "comb.in", tmp_path / "comb.out"
    inp.write_bytes(dc.scalar_bytes(sc))
    r = run(prog, "comb", inp, out)
    assert r.stdout.strip() == f"comb {len(sc)} scalars x 2 shapes", (r.stdout, r.stderr)
    raw = out.read_bytes()
    assert len(raw) == 2 * 32 * (1 + len(sc))
    zero = bytes(32)
    for shape in range(2):
        enc = [raw[32 * (shape * (1 + len(sc)) + i) :][:32] for i in range(1 + len(sc))]
        p = enc[0]
        assert p == oracle.point_mul_generator((2**40 + 12345).to_bytes(32, "little"))
        for k, got in zip(sc, enc[1:]):
            assert got == oracle.point_double_mul_generator((k % dc.L).to_bytes(32, "little"), p, zero), (shape, hex(k))


def test_fixed_comb_zero_digits(prog, tmp_path, oracle):
    """ge_fixed_mul_add (identity selected only where a zero digit occurs) against the always-select form, inside the program, and
    against the oracle's [k]G; the scalars have their zero digits where their names say"""
    named = dc.fixed_scalars()
    zeros = {name: [w for w, d in enumerate(dc.comb_digits(k)) if d == 0] for name, k in named if name != "random"}
    assert zeros["every window"] == list(range(13)) and zeros["first"] == [0] and zeros["middle"] == [6] and zeros["last"] == [12]
    assert zeros["first and last"] == [0, 12] and zeros["none"] == [] and zeros["zero by carry"] == [3]
    sc = [k for _, k in named]
    inp, out = tmp_path / "fixed.in", tmp_path / "fixed.out"
    inp.write_bytes(dc.scalar_bytes(sc))
    r = run(prog, "fixed", inp, out)
    assert r.stdout.startswith(f"fixed {len(sc)} scalars, zero digits seen in windows 0x1fff of 13"), (r.stdout, r.stderr)
    raw = out.read_bytes()
    assert len(raw) == 32 * len(sc)
    for i, k in enumerate(sc):
        assert raw[32 * i :][:32] == oracle.point_mul_generator((k % dc.L).to_bytes(32, "little")), hex(k)


def test_work_model_counts_are_unchanged(prog):
    """a doubling is 4 squarings + 3 multiplications (the fused square-and-subtract counts as ONE squaring), a 5 x 51 comb product 200
    squarings + 551 multiplications: what hc_op_counts and bench.py's OPS model say"""
    lines = dict(ln.split(" ", 1) for ln in run(prog, "counts").stdout.strip().splitlines())
    assert lines == {"dbl_chain": "sq 4 mul 3", "dbl_chain_sgn": "sq 4 mul 3", "dbl": "sq 4 mul 3", "comb5": "sq 200 mul 551"}


def test_the_chain_doubling_is_where_the_issue_puts_it():
    """the table builder, the comb columns and the shared-chain product double with the fused form; ge_dbl itself is untouched"""
    src = (CSRC / "ge25519.cuh").read_text()
    body = lambda name, end: src[src.index(name) : src.index(end, src.index(name))]
    build = body("EG_HD void ge_teeth_tables_build(", "// (Y+X, Y-X, 2Z, 2dT) -> the same point")
    assert build.count("ge_dbl_chain(") == 3 and "ge_dbl(" not in build
    mul = body("EG_HD void ge_teeth_mul(", "// acc = sum_t [k_t]P_t")
    assert "ge_dbl_chain_sgn(" in mul and "ge_dbl(" not in mul and "ge_cached_cneg" not in mul
    multi = body("EG_HD void ge_teeth_mul_multi(", "// ---- fixed-base scalar multiplication")
    assert "ge_dbl_chain(" in multi and "ge_dbl(" not in multi
    dbl = body("EG_HD void ge_dbl(", "// The doubling of the chains")
    assert "fe_sq(b2, Z); fe_add(b2, b2, b2);" in dbl and "fe_carry(r.T);" in dbl
