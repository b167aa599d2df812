"""Field, point and scalar arithmetic at the corners of the limb-bound discipline, on the host build of the device headers.

Every batch of tests/limb_cases.py (raw limb vectors at the top of the class each precondition allows) runs through the
-DEG_BOUNDCHECK + UBSan build of tests/hostcheck (entry hc_limb_ops, shared with the HIP build through tests/devcheck/limb_ops.cuh) and
is compared bit for bit with the operation on Python integers.  The bound-check build proves that callers respect the stated
preconditions; these cases prove that the preconditions are sufficient - a 64-bit column sum that wraps is no undefined behaviour,
only a wrong value.
"""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import limb_cases as lc
from test_hostcheck import HERE, hc  # noqa: F401  (the one host build, shared)


def run_host(hc, b, rows=None):
    inp = b.inp if rows is None else np.ascontiguousarray(b.inp[rows])
    cls = b.cls if rows is None else np.ascontiguousarray(b.cls[rows])
    out = np.full_like(inp, 0xA5A5A5A5)
    hc.hc_limb_ops.restype = None
    hc.hc_limb_ops(C.c_int(b.op), C.c_int(len(inp)), inp.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p),
                   out.ctypes.data_as(C.c_void_p))
    return out


def test_operation_numbers_match_the_header(hc):
    assert hc.hc_limb_op_count() == len(lc.OPS) == len(lc.MATRIX)
    src = (HERE.parent / "devcheck" / "limb_ops.cuh").read_text()
    assert lc.WORDS == 80 and "#define LIMB_WORDS 80" in src and "#define LIMB_SLOTS 8" in src and "#define LIMB_EXTRA 72" in src


def test_layout_and_reference_constants():
    assert lc.POS == [0, 29, 57, 85, 114, 142, 170, 199, 227] and lc.value(lc.P_LIMBS) == lc.P
    assert all(lc.POS[i] + lc.POS[j] - lc.dbl(i, j) == lc.POS[i + j] for i in range(9) for j in range(9) if i + j < 9)
    assert all(lc.POS[i] + lc.POS[j] - lc.dbl(i, j) == lc.POS[i + j - 9] + 255 for i in range(9) for j in range(9) if i + j >= 9)
    assert lc.SQRTM1 * lc.SQRTM1 % lc.P == lc.P - 1 and (lc.D * 121666 + 121665) % lc.P == 0
    consts = (HERE.parent.parent / "elastic_elgamal_amd" / "csrc" / "eg_constants.cuh").read_text()
    for name, v in (("EG_FE_2D", lc.D2), ("EG_FE_SQRTM1", lc.SQRTM1)):
        line = next(ln for ln in consts.splitlines() if ln.startswith(f"#define {name} "))
        limbs = [int(t.strip().rstrip("u"), 16) for t in line[line.index("(") + 1 : line.rindex(")")].split(",")]
        assert lc.value(limbs) == v, name


@pytest.mark.parametrize("name", lc.MATRIX)
def test_every_case_against_the_integer_reference(hc, name):
    b = lc.batch(name)
    assert len(b) >= 4096 and len(b) % 64 != 0
    b.check(run_host(hc, b))


def test_the_model_is_the_code_and_the_cases_reach_their_edge(hc):
    """The column model of limb_cases (unbounded integers) gives the limbs the build gives, so what it says about the accumulators holds
    for the code.  For every class pair whose product is 12 the corner families (all limbs at the top of their class, the same with
    the slack fe_check_values admits, top minus small amounts, limb 1 a hair above) drive a column sum to at least 0.93 * 2^64, for
    products 12.25 .. 12.5 and fe_sq at class 3.5 to at least 0.95 * 2^64; no admitted case reaches 2^64, and the final carry stays
    below 2^36.  The model's largest wrap into limb 1 is the HAIR that every class-1 result is checked against."""
    wrap_max = 0
    for name, model in (("mul", lambda r: lc.model_mul(r[0:9], r[9:18])), ("sq", lambda r: lc.model_sq(r[0:9]))):
        b = lc.batch(name)
        out = run_host(hc, b).tolist()
        reached = {}
        for r, (row, classes, fam) in enumerate(zip(b.rows, b.classes, b.names)):
            limbs, peak, carry, wrap = model(row)
            assert limbs == out[r][0:9], (name, r, fam, classes)
            assert peak < 2**64 and carry < 2**36, (name, r, fam, classes, peak / 2**64, carry.bit_length())
            wrap_max = max(wrap_max, wrap)
            product = classes[0] * classes[-1]
            if fam in lc.CORNER and product >= 12:
                assert peak >= (0.95 if product >= 12.25 else 0.93) * 2**64, (name, fam, classes, peak / 2**64)
                reached.setdefault(classes, set()).add(fam)
        assert all(fams == set(lc.CORNER) for fams in reached.values()), reached
        want = {c for c in lc.MUL_PAIRS if c[0] * c[1] >= 12} if name == "mul" else {(3.5,)}
        assert set(reached) == want and len(want) >= (8 if name == "mul" else 1)
    assert wrap_max == lc.HAIR <= lc.HAIR_BOUND == 2432


def test_every_precondition_is_approached():
    """the batches go right up to the preconditions of fe25519.cuh: each limit appears as a class (sum / product) of some case"""
    cl = lambda name: set(lc.batch(name).classes)
    assert max(a * b for a, b in cl("mul")) == 12.5 and max(max(c) for c in cl("mul")) == 7.9
    assert max(c[0] for c in cl("sq")) == 3.5 and max(c[0] for c in cl("sqn")) == 3.5
    assert max(lc.f32(a) + lc.f32(b) for a, b in cl("add")) == pytest.approx(7.9) and max(c[0] for c in cl("carry")) == 7.9
    assert max(a for a, _ in cl("sub")) == 5.9 and {b for _, b in cl("sub")} == {1}
    assert max(a for a, _ in cl("sub4")) == 3.9 and max(b for _, b in cl("sub4")) == 3.9
    assert max(max(c) for c in cl("canon")) == 7.9
    for name in lc.MATRIX:
        if lc.OPS[name] < lc.OPS["sc_muladd"] and name != "from_words":
            fams = set(lc.batch(name).names)
            assert {"top", "slack", "near", "hair", "onehot", "alternating", "zero", "unreduced", "random"} <= fams, (name, fams)


_CHILD = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import limb_cases as lc
hc = C.CDLL(sys.argv[1])
classes = (float(sys.argv[3]), float(sys.argv[4]))
inp = np.zeros((1, lc.WORDS), dtype=np.uint32)
inp[0, 0:9] = [lc.top(classes[0], i) for i in range(9)]
inp[0, 9:18] = [lc.top(classes[1], i) for i in range(9)]
cls = np.ones((1, lc.SLOTS), dtype=np.float32)
cls[0, 0:2] = classes
out = np.zeros_like(inp)
hc.hc_limb_ops(C.c_int(lc.OPS[sys.argv[5]]), C.c_int(1), inp.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
print("ran", lc.value(out[0, 0:9].tolist()) % lc.P == lc.value(inp[0, 0:9].tolist()) * lc.value(inp[0, 9:18].tolist()) % lc.P)
"""


def _child(hc, classes, op="mul"):
    return subprocess.run([sys.executable, "-c", _CHILD, hc._name, str(HERE.parent), str(classes[0]), str(classes[1]), op],
                          capture_output=True, text=True, timeout=120)


def test_a_case_outside_the_precondition_is_refused(hc):
    """class product 12.6 (4.2 x 3, all limbs at the top of their class): the bound-check build aborts instead of running it; the same
    child runs the class pair 4 x 3 to the end.  (At 4.2 x 3 the model's column sum is still below 2^64: the stated limit of 12.5,
    with the 0.1 % slack of fe_check_values, is what the build enforces, and the first class product whose all-top case wraps is
    above 12.7.)"""
    ok = _child(hc, (4, 3))
    assert ok.returncode == 0 and ok.stdout.strip() == "ran True", (ok.returncode, ok.stdout, ok.stderr)
    bad = _child(hc, (4.2, 3))
    assert bad.returncode == -6 and "fe_mul: class product > 12.5" in bad.stderr and "ran" not in bad.stdout, (bad.returncode, bad.stderr)
    bad = _child(hc, (3.6, 1), "sq")
    assert bad.returncode == -6 and "fe_sq: operand class > 3.5" in bad.stderr, (bad.returncode, bad.stderr)
    limbs = [lc.top(4.2, i) for i in range(9)], [lc.top(3, i) for i in range(9)]
    assert lc.model_mul(*limbs)[1] < 2**64
    limbs = [lc.top(4.3, i) for i in range(9)], [lc.top(3, i) for i in range(9)]
    assert lc.model_mul(*limbs)[1] >= 2**64
